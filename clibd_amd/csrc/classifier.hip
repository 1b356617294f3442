// The linear-probe classifier (reference: scripts/method_linear.py) for gfx950: the head at the loss path's accuracy, the
// cross-entropy of integer targets and the softmax top-k that the seen/unseen threshold sweep consumes.
//
//   logits = x w^T + bias         x: [B,D] encoder features, w: [C,D], C = the number of seen species (916 in the reference)
//   loss   = mean_i ( LSE_j(logits[i,:]) - logits[i, target_i] )
//   conf, idx = topk(softmax(logits), k)
//
// The confidences are compared with `>` against 1 001 thresholds and the class indices are scored under `==`, so the head does not
// run at the towers' bf16 accuracy: the product is the split-bf16 module's (split3.hip, shared with K9) — x = hi + lo, w = hi + lo,
// x w^T ~ hi·hi + hi·lo + lo·hi as ONE NT GEMM with K = 3D over [hi|hi|lo] and [hi|lo|hi] — and so do both backward products:
//     dx = [Ghi | Ghi | Glo] . [Whi^T | Wlo^T | Whi^T]^T          dw = [Ghi^T | Glo^T | Ghi^T] . [Xhi^T | Xhi^T | Xlo^T]^T      (G = dout)
// with every contraction zero padded to whole 64-wide K tiles.  Row statistics use one wave64 per row with the DPP / permlane
// reductions of common.h.  No float atomics: every sum has one order, so loss, gradients, confidences and indices repeat bit for bit.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_classifier.h"
#include "host_util.h"
#include "split3.h"

namespace clibd {

// bias16[j] = bias[j] (j < C, bias given), 0 otherwise: the GEMM's epilogue reads all C16 columns
__global__ __launch_bounds__(256) void pad_bias_kernel(const float* __restrict__ bias, int C, int C16, float* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < C16) out[j] = (bias != nullptr && j < C) ? bias[j] : 0.f;
}

// out[r, c] = S[r, c], c < C: the GEMM's [B, C16] block into the caller's [B, ld_out]
__global__ __launch_bounds__(256) void copy_cols_kernel(const float* __restrict__ S, int ldS, int R, int C, float* __restrict__ out, int ld_out) {
    const size_t total = (size_t)R * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / C;
        const int c = (int)(i - r * C);
        out[r * (size_t)ld_out + c] = S[r * (size_t)ldS + c];
    }
}

// one wave per row: online max and sum in one pass; VEC = 16-byte loads (ld % 4 == 0 and a 16-byte aligned base)
template <bool VEC>
__global__ __launch_bounds__(256) void ce_rows_fwd_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                          int B, int C, float* __restrict__ lse, float* __restrict__ row_loss,
                                                          unsigned* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* lr = logits + (size_t)row * ld;
    float m = -3.0e38f, s = 0.f;
    int j0 = 0;
    if (VEC) {
        const int nq = C >> 2;
        for (int q = lane; q < nq; q += 64) {
            const float4 v = *(const float4*)(lr + 4 * q);
            const float vm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
            const float mn = fmaxf(m, vm);
            s = s * __expf(m - mn) + ((__expf(v.x - mn) + __expf(v.y - mn)) + (__expf(v.z - mn) + __expf(v.w - mn)));
            m = mn;
        }
        j0 = nq << 2;
    }
    for (int j = j0 + lane; j < C; j += 64) online_lse_add(m, s, lr[j]);
    const float mw = wave_max(m);
    s = wave_sum(s * __expf(m - mw));
    if (lane == 0) {
        const float l = mw + __logf(s);
        lse[row] = l;
        const int64_t t = target[row];
        float term = 0.f;
        if (t >= 0 && t < (int64_t)C) {
            term = l - lr[t];
        } else if (err != nullptr) {
            atomicOr(err, 1u);   // an integer flag, not a sum: its value does not depend on the order
        }
        row_loss[row] = term;
    }
}

// dlogits[i, j] = g / B * (exp(logit - lse_i) - [j == target_i]); a row with a bad target is zero
__global__ __launch_bounds__(256) void ce_rows_bwd_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                          const float* __restrict__ lse, int B, int C, const float* __restrict__ dloss,
                                                          float* __restrict__ dlogits, int ld_d) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* lr = logits + (size_t)row * ld;
    float* dr = dlogits + (size_t)row * ld_d;
    const int64_t t = target[row];
    const bool ok = t >= 0 && t < (int64_t)C;
    const float g = (dloss != nullptr ? *dloss : 1.0f) / (float)B;
    const float l = lse[row];
    for (int j = lane; j < C; j += 64) {
        float d = 0.f;
        if (ok) d = g * (__expf(lr[j] - l) - ((int64_t)j == t ? 1.0f : 0.0f));
        dr[j] = d;
    }
}

constexpr int TOPK_MAX = 8;

// one wave per row.  Every lane keeps the 8 best (value, index) pairs of its stride-64 share in registers — the insertion is a fully
// unrolled compare-exchange chain, so the slots stay named registers (no indexed local array, scratch 0) — together with the online max
// and sum of the softmax.  Then k rounds: the wave's best head wins (wave_max of the values, then the lowest index among the lanes that
// hold it — an index below 2^24 is exact in fp32, so the same DPP reduction serves), its lane pops it.
__global__ __launch_bounds__(256) void softmax_topk_kernel(const float* __restrict__ logits, int ld, int B, int C, int k,
                                                           float* __restrict__ conf, int64_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* lr = logits + (size_t)row * ld;
    constexpr float NEG = -__builtin_huge_valf();
    constexpr int NOIDX = 0x7fffffff;
    float v0 = NEG, v1 = NEG, v2 = NEG, v3 = NEG, v4 = NEG, v5 = NEG, v6 = NEG, v7 = NEG;
    int i0 = NOIDX, i1 = NOIDX, i2 = NOIDX, i3 = NOIDX, i4 = NOIDX, i5 = NOIDX, i6 = NOIDX, i7 = NOIDX;
    float m = -3.0e38f, s = 0.f;
#define CLIBD_CEX(V, I)                       \
    if (ranks_before(cv, ci, V, I)) {         \
        const float tv = V; const int ti = I; \
        V = cv; I = ci; cv = tv; ci = ti;     \
    }
    for (int j = lane; j < C; j += 64) {
        const float x = lr[j];
        online_lse_add(m, s, x);
        float cv = x;
        int ci = j;
        CLIBD_CEX(v0, i0) CLIBD_CEX(v1, i1) CLIBD_CEX(v2, i2) CLIBD_CEX(v3, i3)
        CLIBD_CEX(v4, i4) CLIBD_CEX(v5, i5) CLIBD_CEX(v6, i6) CLIBD_CEX(v7, i7)
    }
#undef CLIBD_CEX
    const float mw = wave_max(m);
    const float inv = 1.0f / wave_sum(s * __expf(m - mw));
    for (int r = 0; r < k; ++r) {
        const float best = wave_max(v0);
        const float cand = (v0 == best && i0 != NOIDX) ? (float)i0 : 3.0e38f;
        const int win = (int)(-wave_max(-cand));
        if (lane == 0) {
            conf[(size_t)row * k + r] = __expf(best - mw) * inv;
            idx[(size_t)row * k + r] = (int64_t)win;
        }
        if (i0 == win) {
            v0 = v1; i0 = i1; v1 = v2; i1 = i2; v2 = v3; i2 = i3; v3 = v4; i3 = i4;
            v4 = v5; i4 = i5; v5 = v6; i5 = i6; v6 = v7; i6 = i7; v7 = NEG; i7 = NOIDX;
        }
    }
}

struct ClsWs {
    Split3Ws p;           // x: [B,D] (M = B), y = w: [C,D] (N = C), g = dout
    float *bias16, *S;    // [C16],  [B,C16]: the GEMM's output block
    float* bsum;          // clibd_batch_sum_f32's partials
    size_t bsum_bytes, total;
};

static ClsWs carve(void* base, int B, int C, int D) {
    ClsWs w;
    Carver c(base);
    w.p.carve(c, B, C, D);
    w.bias16 = c.take<float>(pad16(C));
    w.S = c.take<float>((size_t)B * pad16(C));
    w.bsum_bytes = clibd_batch_sum_workspace_bytes(B, (size_t)C);
    w.bsum = (float*)c.take<char>(w.bsum_bytes);
    w.total = c.total();
    return w;
}

constexpr int kMaxClasses = 1 << 24;   // class indices travel through fp32 in softmax_topk_kernel; nothing near it is in sight

static int linear_check(const char* op, const float* x, const float* w, int B, int C, int D, const void* ws, size_t ws_bytes) {
    if (!x || !w || !ws) return fail(op, "null pointer");
    if (B <= 0 || C <= 0 || D <= 0) return fail(op, "non-positive shape");
    if (C > kMaxClasses) return fail(op, "C too large");
    if (D % 64 != 0) return fail(op, "D must be a multiple of 64");
    if (!aligned16(x) || !aligned16(w)) return fail(op, "x and w must be 16-byte aligned");
    if (!aligned16(ws) || ws_bytes < carve(nullptr, B, C, D).total)
        return fail(op, "workspace too small or misaligned (clibd_linear_f32_workspace_bytes)");
    return 0;
}

static int rows_check(const char* op, const float* logits, int ld, int B, int C) {
    if (!logits) return fail(op, "null pointer");
    if (B <= 0 || C <= 0) return fail(op, "non-positive shape");
    if (C > kMaxClasses) return fail(op, "C too large");
    if (ld < C) return fail(op, "ld must be >= C");
    if (((uintptr_t)logits & 3u) != 0) return fail(op, "logits must be 4-byte aligned");
    return 0;
}

}  // namespace clibd

using namespace clibd;

extern "C" size_t clibd_linear_f32_workspace_bytes(int B, int C, int D) {
    if (B <= 0 || C <= 0 || D <= 0) return 0;
    return carve(nullptr, B, C, D).total;
}

extern "C" int clibd_linear_f32_fwd(const float* x, const float* w, const float* bias, int B, int C, int D, float* out, int ld_out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = linear_check("linear_f32_fwd", x, w, B, C, D, workspace, workspace_bytes)) return e;
    if (!out) return set_error(CLIBD_EINVAL, "linear_f32_fwd: null pointer");
    if (ld_out < C) return set_error(CLIBD_EINVAL, "linear_f32_fwd: ld_out must be >= C");
    const ClsWs ws = carve(workspace, B, C, D);
    hipStream_t st = (hipStream_t)stream;
    const int C16 = pad16(C);
    hipLaunchKernelGGL(pad_bias_kernel, dim3((C16 + 255) / 256), dim3(256), 0, st, bias, C, C16, ws.bias16);
    if (int e = split3_forward(x, w, B, C, D, ws.bias16, ws.S, ws.p, grid_for((size_t)B * D), grid_for((size_t)C * D), "linear_f32_fwd",
                               "linear_f32_fwd split", st))
        return e;
    hipLaunchKernelGGL(copy_cols_kernel, dim3(grid_for((size_t)B * C)), dim3(256), 0, st, ws.S, C16, B, C, out, ld_out);
    return check_launch("linear_f32_fwd copy");
}

extern "C" int clibd_linear_f32_bwd(const float* dout, const float* x, const float* w, int B, int C, int D, float* dx, float* dw,
                                    float* db, void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = linear_check("linear_f32_bwd", x, w, B, C, D, workspace, workspace_bytes)) return e;
    if (!dout) return set_error(CLIBD_EINVAL, "linear_f32_bwd: null pointer");
    if ((dx && !aligned16(dx)) || (dw && !aligned16(dw))) return set_error(CLIBD_EINVAL, "linear_f32_bwd: dx and dw must be 16-byte aligned");
    const ClsWs ws = carve(workspace, B, C, D);
    hipStream_t st = (hipStream_t)stream;
    if (db != nullptr) {
        if (hipMemsetAsync(db, 0, (size_t)C * 4, st) != hipSuccess) return set_error(CLIBD_ELAUNCH, "linear_f32_bwd: memset failed");
        if (int e = clibd_batch_sum_f32(dout, B, (size_t)C, db, ws.bsum, ws.bsum_bytes, stream)) return e;
    }
    if (dx == nullptr && dw == nullptr) return CLIBD_OK;
    const int Cp = pad64(C);   // a multiple of 64: every K segment of the backward GEMMs is whole K-tiles
    if (int e = split3_image(dout, C, B, C, Cp, SPLIT3_X, ws.p.G, grid_for((size_t)B * Cp), "linear_f32_bwd split", st)) return e;
    if (dx != nullptr) {   // dx[i,:] = sum_c dout[i,c] w[c,:]: only this product reads the image of w
        if (int e = split3_image(w, D, C, D, D, SPLIT3_Y, ws.p.y3, grid_for((size_t)C * D), "linear_f32_bwd split w", st)) return e;
        if (int e = split3_grad_left(dx, false, B, C, D, ws.p, st)) return e;
    }
    if (dw != nullptr) {   // dw[c,:] = sum_i dout[i,c] x[i,:]: only this product reads the image of x
        if (int e = split3_image(x, D, B, D, D, SPLIT3_X, ws.p.x3, grid_for((size_t)B * D), "linear_f32_bwd split x", st)) return e;
        if (int e = split3_grad_right(dw, false, B, C, D, ws.p, st)) return e;
    }
    return CLIBD_OK;
}

extern "C" size_t clibd_ce_rows_workspace_bytes(int B) {
    if (B <= 0) return 0;
    return align_up((size_t)B * sizeof(float), 256);   // the per-row loss terms
}

extern "C" int clibd_ce_rows_fwd(const float* logits, int ld, const int64_t* target, int B, int C, float* lse, float* loss,
                                 uint32_t* err, void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = rows_check("ce_rows_fwd", logits, ld, B, C)) return e;
    if (!target || !lse || !loss || !workspace) return set_error(CLIBD_EINVAL, "ce_rows_fwd: null pointer");
    if (!aligned16(workspace) || workspace_bytes < clibd_ce_rows_workspace_bytes(B))
        return set_error(CLIBD_EINVAL, "ce_rows_fwd: workspace too small or misaligned (clibd_ce_rows_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    float* rows = (float*)workspace;
    const dim3 grid((B + 3) / 4), block(256);
    if (ld % 4 == 0 && aligned16(logits))
        hipLaunchKernelGGL(ce_rows_fwd_kernel<true>, grid, block, 0, st, logits, ld, target, B, C, lse, rows, (unsigned*)err);
    else
        hipLaunchKernelGGL(ce_rows_fwd_kernel<false>, grid, block, 0, st, logits, ld, target, B, C, lse, rows, (unsigned*)err);
    if (int e = check_launch("ce_rows_fwd")) return e;
    hipLaunchKernelGGL(row_sum_kernel<true>, dim3(1), dim3(256), 0, st, rows, B, loss);
    return check_launch("ce_rows_fwd (loss mean)");
}

extern "C" int clibd_ce_rows_bwd(const float* logits, int ld, const int64_t* target, const float* lse, int B, int C, const float* dloss,
                                 float* dlogits, int ld_d, void* stream) {
    if (int e = rows_check("ce_rows_bwd", logits, ld, B, C)) return e;
    if (!target || !lse || !dlogits) return set_error(CLIBD_EINVAL, "ce_rows_bwd: null pointer");
    if (ld_d < C) return set_error(CLIBD_EINVAL, "ce_rows_bwd: ld_d must be >= C");
    hipLaunchKernelGGL(ce_rows_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, target, lse, B, C, dloss,
                       dlogits, ld_d);
    return check_launch("ce_rows_bwd");
}

extern "C" int clibd_softmax_topk(const float* logits, int ld, int B, int C, int k, float* conf, int64_t* idx, void* stream) {
    if (int e = rows_check("softmax_topk", logits, ld, B, C)) return e;
    if (!conf || !idx) return set_error(CLIBD_EINVAL, "softmax_topk: null pointer");
    if (k < 1 || k > TOPK_MAX) return set_error(CLIBD_EINVAL, "softmax_topk: k must be in 1..8");
    if (k > C) return set_error(CLIBD_EINVAL, "softmax_topk: k larger than the number of classes (selected index k out of range)");
    hipLaunchKernelGGL(softmax_topk_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, B, C, k, conf, idx);
    return check_launch("softmax_topk");
}
