/*
 * clibd_hip_simclr.h — the SimCLR image-only pre-training entries of libclibd_hip.so (gfx950): the NT-Xent loss and
 * Adam with coupled L2 (reference: bioscanclip/util/simclr.py:64-92 info_nce_loss + CrossEntropyLoss, and the
 * torch.optim.Adam(weight_decay=...) of scripts/unimodel/unimodel_training_for_image_encoder.py).
 *
 * A second header beside clibd_hip.h: the same library, the same conventions (extern "C", caller-owned device buffers,
 * `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message, shapes validated on the host before
 * any launch).  The addition is purely additive — no entry of clibd_hip.h changes its signature or its arithmetic — so
 * the ABI version stays 7.  The Python binding keeps these symbols under this header's name in clibd_amd._lib.HEADERS.
 */
#ifndef CLIBD_HIP_SIMCLR_H
#define CLIBD_HIP_SIMCLR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * NT-Xent over N = 2b rows (n_views = 2), one pass over similarity tiles, online row statistics; no N x N array anywhere.
 *   fh = f / max(||f||, 1e-12)          S = fh fh^T * inv_temperature
 *   lse_i = log sum_{j != i} exp S_ij   p(i) = (i + N/2) mod N      loss = mean_i (lse_i - S_{i,p(i)})
 *   top1_hits = #{ i : S_{i,p(i)} >= max_{j != i, j != p(i)} S_ij }   (the reference's accuracy(logits, labels) top-1 count)
 * The product runs on bf16 MFMA with split operands (fh = hi + lo; hi.hi + hi.lo + lo.hi, ~2^-16 relative).
 * N even and >= 4, any D >= 1 (zero padded to the MFMA K step internally).  The workspace (16-byte aligned, at least
 * what clibd_ntxent_workspace_bytes answers, which grows as O(N * D)) carries the operand images and row statistics from fwd to bwd.
 * Both results are written in a fixed order: they repeat bit for bit.
 */
size_t clibd_ntxent_workspace_bytes(int N, int D);
int clibd_ntxent_fwd(const float* f /*[N,D] raw tower outputs*/, int N, int D, float inv_temperature,
                     float* loss /*device scalar, overwritten*/, int* top1_hits /*optional device scalar, overwritten*/,
                     void* workspace, size_t workspace_bytes, void* stream);
/* d loss / d f (normalisation included), times *dloss when given.  Must follow clibd_ntxent_fwd on the same workspace with the same
 * f, N, D and inv_temperature.  With P_ij = exp(S_ij - lse_i) off the diagonal and T the partner indicator,
 *   d loss / d fh_i = inv_temperature * sum_j W_ij fh_j,   W_ij = (exp(S_ij - lse_i) + exp(S_ij - lse_j) - 2 T_ij) / N,  W_ii = 0
 * (S is symmetric: a row block's gradient needs only its own rows of W, so there is no transposed accumulation and no atomic). */
int clibd_ntxent_bwd(const float* f, int N, int D, float inv_temperature, const float* dloss /*optional device scalar, NULL = 1*/,
                     float* df /*[N,D], overwritten*/, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * torch.optim.Adam on a flat fp32 bucket: weight decay is L2 added to the gradient (NOT AdamW's decoupled shrink),
 *   g' = grad_scale * g + weight_decay * p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
 *   p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
 */
int clibd_adam_l2_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int step, float grad_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_SIMCLR_H */
