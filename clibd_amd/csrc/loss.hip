// K9: all-pairs similarity + soft-target (label-equality) cross-entropy, row-block form, for gfx950.
//
//   S[i,j] = scale * <x_i, y_j>          x: [Nx,D] rows owned by this rank (global row offset row0), y: [N,D] all rows
//   T[i,j] = (labels[row0+i] == labels[j])                    (never materialised)
//   loss   = sum_i ( LSE_j(S[i,:]) * sum_j T[i,j]  -  sum_j T[i,j] S[i,j] )      == sum_i CE(S[i,:], T[i,:])
//
// The similarity runs on the bf16 MFMA GEMM with the split-bf16 trick: x = hi + lo, y = hi + lo (both bf16),
// S ~ hi·hi + hi·lo + lo·hi, expressed as ONE NT GEMM with K = 3D over the images [hi|hi|lo] and [hi|lo|hi]
// (error ~2^-16 relative instead of 2^-8: the reference evaluates this product in fp32, loss_func.py:189-190).
// Row statistics use one wave64 per row with DPP / permlane reductions.  The Nx x N similarity block of THIS rank's rows is
// the kernel's fp32 scratch (caller-owned workspace: 16 MiB at Nx = N = 2048, 32 MiB at Nx = 1024, N = 8192); what is never
// materialised is the N x N target matrix, the log-softmax temporaries and the second (transposed) logits of the reference.
// Backward forms the coefficient matrix G = w * (tsum_i * softmax(S)_ij - T_ij) once, split like the forward operands
// (G = Ghi + Glo), and feeds it to the same GEMM with the K-concatenated images
//     dX = scale * [Ghi | Ghi | Glo] . [Yhi | Ylo | Yhi]^T          dY = scale * [Ghi^T | Glo^T | Ghi^T] . [Xhi | Xhi | Xlo]^T
// so the feature gradients carry the forward's ~2^-16 relative accuracy (the reference computes loss and gradients in fp32).
#include "common.h"
#include "../../include/clibd_hip.h"
#include "host_util.h"
#include "split3.h"   // the split-bf16 product module: operand images, forward product, both gradient products

namespace clibd {

struct RowStat {
    float m, s, tsum, tdot;
};

// one wave per row: online log-sum-exp + target sums
__global__ __launch_bounds__(256) void softce_rows_fwd_kernel(const float* __restrict__ S, int ldS, int Nx, int N,
                                                              const int64_t* __restrict__ labels, int row0,
                                                              const float* __restrict__ scale_ptr,
                                                              float* __restrict__ lse, float* __restrict__ tsum_out,
                                                              float* __restrict__ row_loss) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Nx) return;
    const int64_t lab = labels[row0 + row];
    const float scale = *scale_ptr;
    const float* sr = S + (size_t)row * ldS;
    float m = -3.0e38f, s = 0.f, ts = 0.f, td = 0.f;
    for (int j = lane; j < N; j += 64) {
        const float v = sr[j] * scale;
        online_lse_add(m, s, v);
        if (labels[j] == lab) {
            ts += 1.0f;
            td += v;
        }
    }
    const float mw = wave_max(m);
    s = wave_sum(s * __expf(m - mw));
    ts = wave_sum(ts);
    td = wave_sum(td);
    if (lane == 0) {
        const float l = mw + __logf(s);
        lse[row] = l;
        tsum_out[row] = ts;
        row_loss[row] = l * ts - td;   // summed in a fixed order by row_sum_kernel (round 6: no float atomics on the loss path)
    }
}

// The loss value and the temperature gradient are fixed-order sums of per-row terms (row_sum_kernel<false>, common.h): one float atomic per
// row (rounds 1-5) changed their last bits, and through AdamW the trajectory, from launch to launch.
// g_ij = w * (tsum_i * exp(scale*R_ij - lse_i) - T_ij) with R = raw similarities;
// scale * g_ij = hi + lo (bf16 each) is written as the row image [hi | hi | lo] of width 3 * Np (zero padded past N);
// row_ds[i] = sum_j g_ij * R_ij   (dscale += their fixed-order sum, row_sum_kernel)
__global__ __launch_bounds__(256) void softce_rows_bwd_kernel(const float* __restrict__ S, int ldS, int Nx, int N,
                                                              const int64_t* __restrict__ labels, int row0,
                                                              const float* __restrict__ lse, const float* __restrict__ tsum,
                                                              float w, const float* __restrict__ wscale_ptr,
                                                              const float* __restrict__ scale_ptr,
                                                              unsigned short* __restrict__ G,
                                                              int Np, float* __restrict__ row_ds) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Nx) return;
    const int64_t lab = labels[row0 + row];
    const float l = lse[row], ts = tsum[row];
    const float scale = *scale_ptr;
    if (wscale_ptr != nullptr) w *= *wscale_ptr;
    const float* sr = S + (size_t)row * ldS;
    unsigned short* gr = G + (size_t)row * 3 * Np;
    float ds = 0.f;
    for (int j = lane; j < Np; j += 64) {
        float g = 0.f;
        if (j < N) {
            const float v = sr[j];
            g = w * (ts * __expf(v * scale - l) - (labels[j] == lab ? 1.0f : 0.0f));
            ds += g * v;
        }
        const float gs = g * scale;
        const unsigned short hi = f2bf(gs);
        gr[j] = hi;
        gr[Np + j] = hi;
        gr[2 * Np + j] = f2bf(gs - bf2f(hi));
    }
    ds = wave_sum(ds);
    if (lane == 0) row_ds[row] = ds;
}

struct LossWs {
    Split3Ws p;               // x: [Nx,D] (M = Nx), y: [N,D]; p.G is written by softce_rows_bwd_kernel
    float *S, *lse, *tsum;    // [Nx,pad16(N)] (ld = pad16(N), columns N.. ignored), [Nx], [Nx]
    float *rows;              // [Nx]: per-row loss terms (forward), then per-row d(scale) terms (backward)
    size_t total;
};

static LossWs carve(void* base, int Nx, int N, int D) {
    LossWs w;
    Carver c(base);
    w.p.carve(c, Nx, N, D);
    w.S = c.take<float>((size_t)Nx * pad16(N));
    w.lse = c.take<float>(Nx);
    w.tsum = c.take<float>(Nx);
    w.rows = c.take<float>(Nx);
    w.total = c.total();
    return w;
}

static int loss_check(const float* x, const float* y, const int64_t* labels, int Nx, int N, int D, int row0) {
    if (!x || !y || !labels) return set_error(CLIBD_EINVAL, "softce: null pointer");
    if (Nx <= 0 || N <= 0 || D <= 0) return set_error(CLIBD_EINVAL, "softce: non-positive shape");
    if (D % 64 != 0) return set_error(CLIBD_EINVAL, "softce: D must be a multiple of 64");
    if (row0 < 0 || row0 + Nx > N) return set_error(CLIBD_EINVAL, "softce: row block outside the global batch");
    return 0;
}

}  // namespace clibd

using namespace clibd;

extern "C" size_t clibd_softce_workspace_bytes(int Nx, int N, int D) {
    if (Nx <= 0 || N <= 0 || D <= 0) return 0;
    return carve(nullptr, Nx, N, D).total;
}

extern "C" int clibd_softce_rows_fwd(const float* x, const float* y, const int64_t* labels, int Nx, int N, int D, int row0,
                                     const float* scale, float* loss_sum, void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = loss_check(x, y, labels, Nx, N, D, row0)) return e;
    if (!loss_sum || !workspace || !scale) return set_error(CLIBD_EINVAL, "softce_fwd: null pointer");
    if (!aligned16(workspace)) return set_error(CLIBD_EINVAL, "softce_fwd: workspace must be 16-byte aligned");
    const LossWs w = carve(workspace, Nx, N, D);
    if (workspace_bytes < w.total) return set_error(CLIBD_EINVAL, "softce_fwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    // w.S = the raw similarities <x_i, y_j>
    if (int e = split3_forward(x, y, Nx, N, D, nullptr, w.S, w.p, 1024, 1024, "softce_fwd", "softce split", st)) return e;
    hipLaunchKernelGGL(softce_rows_fwd_kernel, dim3((Nx + 3) / 4), dim3(256), 0, st, w.S, pad16(N), Nx, N, labels, row0, scale,
                       w.lse, w.tsum, w.rows);
    if (int e = check_launch("softce_rows_fwd")) return e;
    hipLaunchKernelGGL(row_sum_kernel<false>, dim3(1), dim3(256), 0, st, w.rows, Nx, loss_sum);
    return check_launch("softce_rows_fwd (loss sum)");
}

// Must follow clibd_softce_rows_fwd on the same workspace (reuses its similarity matrix and row statistics).
extern "C" int clibd_softce_rows_bwd(const int64_t* labels, int Nx, int N, int D, int row0, const float* scale, float weight,
                                     const float* weight_scale, float* dx, float* dy, float* dscale, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    if (!labels || !dx || !dy || !workspace || !scale) return set_error(CLIBD_EINVAL, "softce_bwd: null pointer");
    if (Nx <= 0 || N <= 0 || D <= 0 || D % 64 != 0 || row0 < 0 || row0 + Nx > N)
        return set_error(CLIBD_EINVAL, "softce_bwd: bad shape");
    if (!aligned16(workspace) || !aligned16(dx) || !aligned16(dy)) return set_error(CLIBD_EINVAL, "softce_bwd: alignment");
    const LossWs w = carve(workspace, Nx, N, D);
    if (workspace_bytes < w.total) return set_error(CLIBD_EINVAL, "softce_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    // the image of G is pad64(N) wide: every K segment of the backward GEMMs is whole K-tiles
    hipLaunchKernelGGL(softce_rows_bwd_kernel, dim3((Nx + 3) / 4), dim3(256), 0, st, w.S, pad16(N), Nx, N, labels, row0, w.lse,
                       w.tsum, weight, weight_scale, scale, w.p.G, pad64(N), w.rows);
    if (int e = check_launch("softce_rows_bwd")) return e;
    if (dscale != nullptr) {
        hipLaunchKernelGGL(row_sum_kernel<false>, dim3(1), dim3(256), 0, st, w.rows, Nx, dscale);
        if (int e = check_launch("softce_rows_bwd (dscale sum)")) return e;
    }
    // dx[i,:] += sum_j G[i,j] y[j,:] and dy[j,:] += sum_i G[i,j] x[i,:], accumulated in place
    if (int e = split3_grad_left(dx, true, Nx, N, D, w.p, st)) return e;
    return split3_grad_right(dy, true, Nx, N, D, w.p, st);
}
