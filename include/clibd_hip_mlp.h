/*
 * clibd_hip_mlp.h — the fp32-grade linear layers of the pre-extracted-feature towers of libclibd_hip.so (gfx950): the reference's
 * MLPEncoder (bioscanclip/model/mlp.py: Linear, ReLU, Linear, ReLU, Linear over `image_features` / `dna_features` rows), one launch per
 * role and layer.
 *
 * An eighth header beside clibd_hip.h and the six additive ones: the same library, the same conventions (extern "C", caller-owned device
 * buffers, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message, nothing allocates or synchronises, arguments
 * validated on the host before any launch).  The addition is purely additive — no entry of the other headers changes its signature or
 * its arithmetic — so the ABI version stays 7.  The Python binding keeps these symbols under this header's name in clibd_amd._lib.HEADERS.
 *
 * Arithmetic.  Every operand is fp32 in memory.  A workgroup splits the tiles it loads on their way into LDS, v = hi + lo with
 * hi = bf16(v), lo = bf16(v - hi), and accumulates hi·hi + hi·lo + lo·hi on the bf16 MFMA in fp32 (relative error ~2^-16, the
 * accuracy of clibd_linear_f32_fwd): no operand images in memory, no transposes, no workspace.  No float atomics: every output element
 * is one workgroup's sum in one order, so results repeat bit for bit.
 *
 * Shapes (one layer: B rows, K input features, N output features):  B >= 1 (at most 2^21);  K a positive multiple of 4;  N a positive
 * multiple of 16;  K, N <= 4096.  x, w, dy are 16-byte aligned; every matrix is dense row-major.
 */
#ifndef CLIBD_HIP_MLP_H
#define CLIBD_HIP_MLP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[B, N] = act(x[B, K] · w[N, K]^T + bias[N]);  bias may be NULL;  relu != 0: act = max(., 0) (NaN stays NaN), else the identity */
int clibd_mlp_linear_fwd(const float* x, const float* w, const float* bias, int B, int N, int K, int relu, float* out, void* stream);

/* dx[B, K] = (dy[B, N] · w[N, K]) ⊙ [h[B, K] > 0];  h = the post-ReLU activation the forward wrote (NULL: no mask).  h > 0 is
 * torch's ReLU backward: an activation of exactly 0 passes no gradient. */
int clibd_mlp_linear_dgrad(const float* dy, const float* w, const float* h, int B, int N, int K, float* dx, void* stream);

/* dw[N, K] (+)= dy[B, N]^T · x[B, K];  db[N] (+)= the column sums of dy (db may be NULL);  accumulate != 0 adds to what dw / db hold.
 * The contraction over B runs inside one workgroup per output tile, in row order; db is summed, in fp32 from the fp32 dy, by the
 * workgroups that own the first column tile of each row block, per-thread partials in a fixed assignment and a fixed final order. */
int clibd_mlp_linear_wgrad(const float* dy, const float* x, int B, int N, int K, float* dw, float* db, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_MLP_H */
