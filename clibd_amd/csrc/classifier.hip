// The linear-probe classifier (reference: scripts/method_linear.py) for gfx950: the head at the loss path's accuracy, the
// cross-entropy of integer targets and the softmax top-k that the seen/unseen threshold sweep consumes.
//
//   logits = x w^T + bias         x: [B,D] encoder features, w: [C,D], C = the number of seen species (916 in the reference)
//   loss   = mean_i ( LSE_j(logits[i,:]) - logits[i, target_i] )
//   conf, idx = topk(softmax(logits), k)
//
// The confidences are compared with `>` against 1 001 thresholds and the class indices are scored under `==`, so the head does not
// run at the towers' bf16 accuracy: the product uses the split-bf16 operands of K9 (loss.hip, split3.h) — x = hi + lo, w = hi + lo,
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

// the x-side image [hi | hi | lo] of in[R, C] (row stride ld_in), each segment zero padded to Cp columns: out [R, 3 Cp]
__global__ __launch_bounds__(256) void split3_pad_kernel(const float* __restrict__ in, int ld_in, int R, int C, int Cp,
                                                         unsigned short* __restrict__ out) {
    const size_t total = (size_t)R * Cp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / Cp;
        const int c = (int)(i - r * Cp);
        const float v = c < C ? in[r * (size_t)ld_in + c] : 0.f;
        const unsigned short hi = f2bf(v);
        unsigned short* o = out + r * 3 * (size_t)Cp;
        o[c] = hi;
        o[Cp + c] = hi;
        o[2 * Cp + c] = f2bf(v - bf2f(hi));
    }
}

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

__device__ __forceinline__ void online_add(float& m, float& s, float v) {
    if (v > m) {
        s = s * __expf(m - v) + 1.0f;
        m = v;
    } else {
        s += __expf(v - m);
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
    for (int j = j0 + lane; j < C; j += 64) online_add(m, s, lr[j]);
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

// out[0] = (sum_i v[i]) / n, one workgroup, the summation order of loss.hip's reduce_rows_add_kernel (thread t takes i = t, t + 256, ...;
// then an LDS tree)
__global__ __launch_bounds__(256) void mean_rows_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
    __shared__ float part[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += v[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0] / (float)n;
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

// (a, ia) ranks before (b, ib): the larger value, equal values by the lower index
__device__ __forceinline__ bool ranks_before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

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
        online_add(m, s, x);
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
    unsigned short *x3, *w3;   // [B,3D] = [hi|hi|lo],  [C16,3D] = [hi|lo|hi] (rows C.. zero)
    float *bias16, *S;         // [C16],  [B,C16]: the GEMM's output block
    unsigned short *G, *GT;    // dout: [B,3Cp] = [hi|hi|lo],  [C,3Bp] = [hi^T|lo^T|hi^T]
    unsigned short *xT, *wT;   // [D,3Bp] = [hi^T|hi^T|lo^T],  [D,3Cp] = [hi^T|lo^T|hi^T]
    float* bsum;               // clibd_batch_sum_f32's partials
    size_t bsum_bytes, total;
};

static ClsWs carve(void* base, int B, int C, int D) {
    ClsWs w;
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* q = p ? p + off : nullptr;
        off += align_up(bytes, 256);
        return q;
    };
    const int C16 = pad16(C), Cp = pad64(C), Bp = pad64(B);
    w.x3 = (unsigned short*)take((size_t)B * 3 * D * 2);
    w.w3 = (unsigned short*)take((size_t)C16 * 3 * D * 2);
    w.bias16 = (float*)take((size_t)C16 * 4);
    w.S = (float*)take((size_t)B * C16 * 4);
    w.G = (unsigned short*)take((size_t)B * 3 * Cp * 2);
    w.GT = (unsigned short*)take((size_t)C * 3 * Bp * 2);
    w.xT = (unsigned short*)take((size_t)D * 3 * Bp * 2);
    w.wT = (unsigned short*)take((size_t)D * 3 * Cp * 2);
    w.bsum_bytes = clibd_batch_sum_workspace_bytes(B, (size_t)C);
    w.bsum = (float*)take(w.bsum_bytes);
    w.total = off;
    return w;
}

constexpr int kMaxClasses = 1 << 24;   // class indices travel through fp32 in softmax_topk_kernel; nothing near it is in sight

static int linear_check(const char* op, const float* x, const float* w, int B, int C, int D, const void* ws, size_t ws_bytes) {
    char msg[kErrBufLen];
    auto fail = [&](const char* what) {
        snprintf(msg, sizeof msg, "%s: %s", op, what);
        return set_error(CLIBD_EINVAL, msg);
    };
    if (!x || !w || !ws) return fail("null pointer");
    if (B <= 0 || C <= 0 || D <= 0) return fail("non-positive shape");
    if (C > kMaxClasses) return fail("C too large");
    if (D % 64 != 0) return fail("D must be a multiple of 64");
    if (!aligned16(x) || !aligned16(w)) return fail("x and w must be 16-byte aligned");
    if (!aligned16(ws) || ws_bytes < carve(nullptr, B, C, D).total)
        return fail("workspace too small or misaligned (clibd_linear_f32_workspace_bytes)");
    return 0;
}

static int rows_check(const char* op, const float* logits, int ld, int B, int C) {
    char msg[kErrBufLen];
    auto fail = [&](const char* what) {
        snprintf(msg, sizeof msg, "%s: %s", op, what);
        return set_error(CLIBD_EINVAL, msg);
    };
    if (!logits) return fail("null pointer");
    if (B <= 0 || C <= 0) return fail("non-positive shape");
    if (C > kMaxClasses) return fail("C too large");
    if (ld < C) return fail("ld must be >= C");
    if (((uintptr_t)logits & 3u) != 0) return fail("logits must be 4-byte aligned");
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
    hipLaunchKernelGGL(split3_kernel, dim3(grid_for((size_t)B * D)), dim3(256), 0, st, x, B, D, 1, ws.x3);
    hipLaunchKernelGGL(split3_kernel, dim3(grid_for((size_t)C * D)), dim3(256), 0, st, w, C, D, 0, ws.w3);
    hipLaunchKernelGGL(pad_bias_kernel, dim3((C16 + 255) / 256), dim3(256), 0, st, bias, C, C16, ws.bias16);
    if (int e = check_launch("linear_f32_fwd split")) return e;
    if (C16 != C && hipMemsetAsync(ws.w3 + (size_t)C * 3 * D, 0, (size_t)(C16 - C) * 3 * D * 2, st) != hipSuccess)
        return set_error(CLIBD_ELAUNCH, "linear_f32_fwd: memset failed");
    clibd_gemm_epilogue ep = {};
    ep.bias = ws.bias16;
    ep.out_f32 = ws.S;
    ep.ld_out_f32 = C16;
    ep.split_k = 1;
    if (int e = clibd_gemm_bf16_nt(ws.x3, 3 * D, ws.w3, 3 * D, B, C16, 3 * D, &ep, nullptr, 0, stream)) return e;
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
    const int Cp = pad64(C), Bp = pad64(B);   // multiples of 64: every K segment of the backward GEMMs is whole K-tiles
    if (db != nullptr) {
        if (hipMemsetAsync(db, 0, (size_t)C * 4, st) != hipSuccess) return set_error(CLIBD_ELAUNCH, "linear_f32_bwd: memset failed");
        if (int e = clibd_batch_sum_f32(dout, B, (size_t)C, db, ws.bsum, ws.bsum_bytes, stream)) return e;
    }
    if (dx == nullptr && dw == nullptr) return CLIBD_OK;
    hipLaunchKernelGGL(split3_pad_kernel, dim3(grid_for((size_t)B * Cp)), dim3(256), 0, st, dout, C, B, C, Cp, ws.G);
    if (int e = check_launch("linear_f32_bwd split")) return e;
    clibd_gemm_epilogue ep = {};
    ep.split_k = 1;
    ep.ld_out_f32 = D;
    if (dx != nullptr) {   // dx[i,:] = sum_c dout[i,c] w[c,:]
        hipLaunchKernelGGL(split3_kernel, dim3(grid_for((size_t)C * D)), dim3(256), 0, st, w, C, D, 0, ws.w3);
        if (int e = check_launch("linear_f32_bwd split w")) return e;
        if (int e = launch_transpose3(ws.w3, C, D, D, /*hi, lo, hi*/ 0 | (1 << 2) | (2 << 4), ws.wT, Cp, st)) return e;
        ep.out_f32 = dx;
        if (int e = clibd_gemm_bf16_nt(ws.G, 3 * Cp, ws.wT, 3 * Cp, B, D, 3 * Cp, &ep, nullptr, 0, stream)) return e;
    }
    if (dw != nullptr) {   // dw[c,:] = sum_i dout[i,c] x[i,:]
        hipLaunchKernelGGL(split3_kernel, dim3(grid_for((size_t)B * D)), dim3(256), 0, st, x, B, D, 1, ws.x3);
        if (int e = check_launch("linear_f32_bwd split x")) return e;
        if (int e = launch_transpose3(ws.G, B, Cp, C, /*hi, lo, hi*/ 0 | (2 << 2) | (0 << 4), ws.GT, Bp, st)) return e;
        if (int e = launch_transpose3(ws.x3, B, D, D, /*hi, hi, lo*/ 0 | (1 << 2) | (2 << 4), ws.xT, Bp, st)) return e;
        ep.out_f32 = dw;
        if (int e = clibd_gemm_bf16_nt(ws.GT, 3 * Bp, ws.xT, 3 * Bp, C, D, 3 * Bp, &ep, nullptr, 0, stream)) return e;
    }
    return CLIBD_OK;
}

extern "C" size_t clibd_ce_rows_workspace_bytes(int B) {
    if (B <= 0) return 0;
    return align_up((size_t)B * sizeof(float), 256);
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
    hipLaunchKernelGGL(mean_rows_kernel, dim3(1), dim3(256), 0, st, rows, B, loss);
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
