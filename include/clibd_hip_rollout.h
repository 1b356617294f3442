/*
 * clibd_hip_rollout.h — the attention rollout of libclibd_hip.so (gfx950): the arithmetic behind the reference's
 * scripts/result/representation_visualization/{image,dna}_representation_visualization.py (`rollout`, after jacobgil/vit-explain):
 * per layer the heads' softmax probabilities fused by mean / max / min, the lowest `discard_ratio` of each fused map zeroed, and the
 * maps chained.  No figure is drawn here or anywhere in the project.
 *
 * A sixth header beside clibd_hip.h, clibd_hip_simclr.h, clibd_hip_views.h, clibd_hip_classifier.h and clibd_hip_analysis.h: the same
 * library, the same conventions (extern "C", caller-owned device buffers and workspaces, `void* stream`, 0 / negative CLIBD_E* status,
 * clibd_last_error for the message, nothing allocates or synchronises, arguments validated on the host before any launch).  The addition
 * is purely additive — no entry of the other five headers changes — so the ABI version stays 7.  The Python binding keeps these symbols
 * under this header's name in clibd_amd._lib.HEADERS.
 *
 * No float atomics: every output has one summation order, so two runs agree bit for bit.  A batch is B independent maps.
 */
#ifndef CLIBD_HIP_ROLLOUT_H
#define CLIBD_HIP_ROLLOUT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIBD_FUSE_MEAN 0
#define CLIBD_FUSE_MAX 1
#define CLIBD_FUSE_MIN 2

/* ------------------------------------------------------------------------------------------------
 * The fused attention map of one layer: out[b, i, j] = fuse_h softmax_j(q_hi . k_hj / 8), no key mask, no dropout (what a forward hook
 * on the attention dropout sees in eval mode).
 *   qkv    bf16 [B * S, 3 H], H = 64 * heads, 16-byte aligned: the packed operand of clibd_attention_fwd (q | k | v, head h at columns
 *          64 h of each third); v is not read.
 *   1 <= S <= 256, heads >= 1, fusion one of CLIBD_FUSE_*.
 *   out    fp32 [B, S, ld], ld >= S and ld % 4 == 0, 16-byte aligned.  Columns S .. ld - 1 are written with zeros or left alone; no
 *          entry of this header reads them.
 * The per-head probabilities stay in registers (S * ld floats leave per image, not heads * S * S).  The mean is the sum in head order
 * divided by `heads`, so over one head all three fusions give the same bits.
 */
int clibd_attn_fused_maps(const void* qkv, int B, int S, int heads, int fusion, float* out, int ld, void* stream);

/* ------------------------------------------------------------------------------------------------
 * In place on maps fp32 [B, S, ld] (ld >= S): per map, the k smallest of the S * S logical entries are set to 0, except flat index 0
 * (entry [0, 0]), which still counts among the k.  0 <= k <= S * S; 1 <= S <= 256.
 * The selection is exact (a radix select on the bit patterns: the entries must be non-negative and not NaN, which the host cannot
 * check).  Ties: every entry below the k-th smallest value t is zeroed; entries equal to t are zeroed in ascending flat index i * S + j
 * until k are taken.
 * workspace: clibd_rollout_discard_workspace_bytes(B) bytes (0 for B <= 0), 16-byte aligned: per map four uint32 — the bits of t, the
 * number of entries below t, the number of entries equal to t that were taken, k — left there as the record of the selection.
 */
size_t clibd_rollout_discard_workspace_bytes(int B);
int clibd_rollout_discard(float* maps, int B, int S, int ld, int k, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The chain.  maps fp32 [L, B, S, ld] in the reference's order of application (index 0 first), out fp32 [B, S - 1]:
 *   r_l[j] = (sum_k F_l[j, k] + 1) / 2;  a_l[i, j] = (F_l[i, j] + [i == j]) / 2
 *   v <- e_0;  for l = L - 1 .. 0:  v[j] <- (sum_i v[i] a_l[i, j]) / r_l[j]      (column j over the sum of ROW j: the reference's broadcast)
 *   out = v[1:] / max(v[1:])
 * which is row 0 of the reference's matrix product.  fp32, every sum in one fixed order.  L >= 1, 2 <= S <= 256, ld >= S.
 */
int clibd_rollout_chain(const float* maps, int L, int B, int S, int ld, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_ROLLOUT_H */
