/*
 * clibd_hip_classifier.h — the linear-probe classifier of libclibd_hip.so (gfx950): the head, its cross-entropy and the softmax
 * top-k of the reference's second seen/unseen method (scripts/method_linear.py: ViTWIthExtraLayer's nn.Linear(output_dim,
 * n_seen_species), nn.CrossEntropyLoss(), torch.topk(F.softmax(output, dim=-1), 5)).
 *
 * A fourth header beside clibd_hip.h, clibd_hip_simclr.h and clibd_hip_views.h: the same library, the same conventions (extern "C",
 * caller-owned device buffers and workspaces, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message, nothing
 * allocates or synchronises, arguments validated on the host before any launch).  The addition is purely additive — no entry of the
 * other three headers changes its signature or its arithmetic — so the ABI version stays 7.  The Python binding keeps these symbols under this
 * header's name in clibd_amd._lib.HEADERS.
 *
 * No float atomics: every output element and every sum has one fixed order, so results repeat bit for bit.
 */
#ifndef CLIBD_HIP_CLASSIFIER_H
#define CLIBD_HIP_CLASSIFIER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The head at the loss path's accuracy.  The confidences of this classifier are compared with `>` against a grid of thresholds and its
 * top-5 class indices are scored under `==`, so the product runs on the split-bf16 operands of K9 (clibd_softce_rows_fwd): x = hi + lo,
 * w = hi + lo (bf16 each), x w^T ~ hi·hi + hi·lo + lo·hi as ONE clibd_gemm_bf16_nt with K = 3D (relative error ~2^-16, not 2^-8).
 *   x fp32 [B, D], w fp32 [C, D], bias fp32 [C] or NULL; D % 64 == 0; any B >= 1, C >= 1 (below 2^24); x, w, dx, dw 16-byte aligned.
 * workspace: clibd_linear_f32_workspace_bytes(B, C, D) bytes, 16-byte aligned; the same size serves forward and backward, and the
 * backward does not depend on what a forward left there (it splits x and w again).
 *
 * clibd_linear_f32_fwd: out[B, ld_out] (ld_out >= C; columns C.. are not written) = x w^T + bias, the bias in the GEMM's epilogue.
 * clibd_linear_f32_bwd: dout fp32 [B, C] dense.  Each of dx [B, D] = dout w, dw [C, D] = dout^T x, db [C] = the column sums of dout
 *   (fixed order: the workspace form of clibd_batch_sum_f32) may be NULL; the outputs are overwritten, not accumulated.
 */
size_t clibd_linear_f32_workspace_bytes(int B, int C, int D);
int clibd_linear_f32_fwd(const float* x, const float* w, const float* bias, int B, int C, int D, float* out, int ld_out,
                         void* workspace, size_t workspace_bytes, void* stream);
int clibd_linear_f32_bwd(const float* dout, const float* x, const float* w, int B, int C, int D, float* dx, float* dw, float* db,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * nn.CrossEntropyLoss() (mean reduction, integer targets) over logits fp32 [B, ld] (ld >= C), target int64 [B].
 * clibd_ce_rows_fwd: one wave per row, online max and sum in one pass: lse[i] = log sum_j exp(logit[i, j]);
 *   *loss = (1 / B) sum_i (lse[i] - logit[i, target[i]]), the per-row terms summed by one workgroup in a fixed order (overwrites *loss).
 *   A target outside [0, C) reads nothing for it, contributes 0 to the sum (the divisor stays B) and ORs bit 0 into the device word
 *   *err (uint32; the caller zeroes it when it wants a fresh report; NULL: not reported).
 *   workspace: clibd_ce_rows_workspace_bytes(B) bytes, 16-byte aligned.
 * clibd_ce_rows_bwd: dlogits[i, j] = g / B * (exp(logit[i, j] - lse[i]) - [j == target[i]]), j < C, with g = *dloss (a device scalar)
 *   or 1 when dloss is NULL; a row with a bad target is zero.  dlogits [B, ld_d], ld_d >= C; columns C.. are not written.
 */
size_t clibd_ce_rows_workspace_bytes(int B);
int clibd_ce_rows_fwd(const float* logits, int ld, const int64_t* target, int B, int C, float* lse, float* loss, uint32_t* err,
                      void* workspace, size_t workspace_bytes, void* stream);
int clibd_ce_rows_bwd(const float* logits, int ld, const int64_t* target, const float* lse, int B, int C, const float* dloss,
                      float* dlogits, int ld_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * torch.topk(F.softmax(logits, -1), k, sorted=True): conf[B, k] fp32 = exp(l - max) / sum_j exp(l_j - max), idx[B, k] int64, by
 * descending value, equal values by ascending index.  1 <= k <= 8 and k <= C.  One wave per row: every lane keeps its own k best in
 * registers, then k rounds of a wave arg-max pick the output.
 */
int clibd_softmax_topk(const float* logits, int ld, int B, int C, int k, float* conf, int64_t* idx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_CLASSIFIER_H */
