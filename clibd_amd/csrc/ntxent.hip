// NT-Xent (SimCLR) loss for gfx950: one pass over similarity tiles with online row statistics, no N x N array in memory.
//
//   fh = f / max(||f||, 1e-12)      S = fh fh^T / tau      lse_i = log sum_{j != i} exp S_ij      p(i) = (i + N/2) mod N
//   loss = mean_i (lse_i - S_{i,p(i)})                     (reference: bioscanclip/util/simclr.py:64-92 + CrossEntropyLoss)
//
// Operands are K9's split bf16 (loss.hip): fh = hi + lo, S ~ hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16, ~2^-16 relative
// (1/tau ~ 14 multiplies whatever error the product has).  Every tile is computed TRANSPOSED, X[j][i] = <fh_j, fh_i> with A = the
// column block's rows and B = the row block's rows: the accumulator then has the loss row i on the lane (lane & 31) and 16 columns
// j in its registers (j = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so
//   forward:  the running max / sum / partner logit of row i live in ONE lane and no cross-lane step is needed per tile;
//   backward: W^T (same layout) is, converted in place to bf16, the A operand of the next product  G[i][d] = sum_j W_ij fh_j[d]
//             — that product sums over the tile's ROW index, which needs no lane movement.  S is symmetric, so
//             W_ij = (exp(S_ij - lse_i) + exp(S_ij - lse_j) - 2 T_ij) / N  holds both the row and the column softmax term:
//             a row block's gradient needs only its own rows, no transposed accumulation, no atomic, a fixed summation order.
// The k order of an accumulator used as an operand is permuted (element e of lane half h of k-step s is tile row
// 16 s + 8 (e >> 2) + 4 h + (e & 3)); the transposed operand image fT[d][j] is written in that order within every group of 32 j,
// so the B fragment of the second product is one 16-byte load.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_simclr.h"
#include "host_util.h"

namespace clibd {

constexpr float NTX_NEG = -3.0e38f;   // "no value yet": finite, so that differences of two of them stay finite
constexpr int NTX_FWD_SLICES = 8;     // column slices of the forward (gridDim.y): 8 x more waves to hide the fragment loads' latency
constexpr int NTX_BWD_NSUB = 2;       // 32-wide output column tiles per wave of the backward (4 waves: 256 columns per workgroup)

// one wave per row r < Np: inverse norm, normalised row as padded hi / lo bf16 images [Np, Dp] (zeros past N and past D)
__global__ __launch_bounds__(256) void ntxent_prep_kernel(const float* __restrict__ f, int N, int Np, int D, int Dp,
                                                          unsigned short* __restrict__ fhi, unsigned short* __restrict__ flo,
                                                          float* __restrict__ inv_norm, float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= Np) return;
    float inv = 0.f;
    const float* fr = f + (size_t)row * D;
    if (row < N) {
        float ss = 0.f;
        for (int c = lane; c < D; c += 64) ss += fr[c] * fr[c];
        ss = wave_sum(ss);
        inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);   // F.normalize(eps = 1e-12)
    }
    for (int c = lane; c < Dp; c += 64) {
        const float v = (row < N && c < D) ? fr[c] * inv : 0.f;
        const unsigned short hi = f2bf(v);
        fhi[(size_t)row * Dp + c] = hi;
        flo[(size_t)row * Dp + c] = f2bf(v - bf2f(hi));
    }
    if (lane == 0) {
        inv_norm[row] = inv;
        if (row >= N) lse[row] = 0.f;   // the backward reads whole tiles of lse
    }
}

// X[j][i] for one 32 x 32 tile: A = rows j0.. (this lane: row j0 + (lane & 31), k = 8 (lane >> 5) ..), B = rows i0..
__device__ __forceinline__ f32x16 ntxent_tile(const unsigned short* __restrict__ ahi, const unsigned short* __restrict__ alo,
                                              const unsigned short* __restrict__ bhi, const unsigned short* __restrict__ blo, int Dp) {
    f32x16 acc = {};
    // four k-steps' fragments (16 loads of 16 bytes) in flight per round trip: the loop is bound by load latency, not by the MFMA
#pragma unroll 4
    for (int k = 0; k < Dp; k += 16) {
        const bf16x8 ah = *(const bf16x8*)(ahi + k), al = *(const bf16x8*)(alo + k);
        const bf16x8 bh = *(const bf16x8*)(bhi + k), bl = *(const bf16x8*)(blo + k);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    }
    return acc;
}

// one workgroup per 32 loss rows (blockIdx.x) and column slice (blockIdx.y of gridDim.y): its 4 waves take the 32-column tiles
// 4 blockIdx.y + wave, + 4 gridDim.y, ...; part[blockIdx.y][i] = (running max, sum, partner logit, best negative) of row i over the slice
__global__ __launch_bounds__(256) void ntxent_fwd_kernel(const unsigned short* __restrict__ fhi, const unsigned short* __restrict__ flo,
                                                         int N, int Np, int Dp, float inv_t, float4* __restrict__ part) {
    __shared__ float4 st[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int i = blockIdx.x * 32 + c;
    int partner = i + (N >> 1);
    if (partner >= N) partner -= N;
    const size_t boff = (size_t)i * Dp + 8 * h;
    float m = NTX_NEG, s = 0.f, ps = NTX_NEG, mn = NTX_NEG;
    for (int j0 = (blockIdx.y * 4 + wave) * 32; j0 < N; j0 += 128 * gridDim.y) {
        const size_t aoff = (size_t)(j0 + c) * Dp + 8 * h;
        const f32x16 acc = ntxent_tile(fhi + aoff, flo + aoff, fhi + boff, flo + boff, Dp);
        float v[16], tmax = NTX_NEG;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float x = acc[r] * inv_t;
            const bool valid = j < N && j != i;
            if (j == partner) ps = x;
            if (valid && j != partner) mn = fmaxf(mn, x);
            v[r] = valid ? x : NTX_NEG;
            tmax = fmaxf(tmax, v[r]);
        }
        const float mnew = fmaxf(m, tmax);
        float add = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) add += v[r] > -1.0e38f ? __expf(v[r] - mnew) : 0.f;
        s = s * __expf(m - mnew) + add;
        m = mnew;
    }
    st[threadIdx.x] = make_float4(m, s, ps, mn);
    __syncthreads();
    if (threadIdx.x < 32 && i < N) {
        // the 8 partial statistics of row i (4 waves x 2 lane halves), combined in a fixed order
        float M = NTX_NEG, P = NTX_NEG, Mn = NTX_NEG, S = 0.f;
        for (int q = 0; q < 8; ++q) M = fmaxf(M, st[q * 32 + c].x);
        for (int q = 0; q < 8; ++q) {
            const float4 e = st[q * 32 + c];
            S += e.y * __expf(e.x - M);
            P = fmaxf(P, e.z);
            Mn = fmaxf(Mn, e.w);
        }
        part[(size_t)blockIdx.y * Np + i] = make_float4(M, S, P, Mn);
    }
}

// Row statistics from the column slices' partials, in slice order; lse[i] for the backward; loss = sum_i (lse_i - pos_i) / N and
// top1 = #{i : pos_i >= best negative}: one workgroup, a fixed order (thread t takes i = t, t + 256, ...; then block_tree_sum)
struct NtxTotals {
    float loss;
    int top1;
    __device__ NtxTotals& operator+=(const NtxTotals& o) { loss += o.loss; top1 += o.top1; return *this; }
};

__global__ __launch_bounds__(256) void ntxent_reduce_kernel(const float4* __restrict__ stat, int nslice, int N, int Np,
                                                            float* __restrict__ lse, float* __restrict__ loss, int* __restrict__ top1) {
    __shared__ NtxTotals part[256];
    NtxTotals t = {0.f, 0};
    for (int i = threadIdx.x; i < N; i += 256) {
        float M = NTX_NEG, P = NTX_NEG, Mn = NTX_NEG, S = 0.f;
        for (int q = 0; q < nslice; ++q) M = fmaxf(M, stat[(size_t)q * Np + i].x);
        for (int q = 0; q < nslice; ++q) {
            const float4 e = stat[(size_t)q * Np + i];
            S += e.y * __expf(e.x - M);
            P = fmaxf(P, e.z);
            Mn = fmaxf(Mn, e.w);
        }
        const float l = M + __logf(S);
        lse[i] = l;
        t.loss += l - P;
        t.top1 += P >= Mn ? 1 : 0;
    }
    t = block_tree_sum(t, part);
    if (threadIdx.x == 0) {
        loss[0] = t.loss / (float)N;
        if (top1 != nullptr) top1[0] = t.top1;
    }
}

// fT[d][j0 + q] = f[j0 + jl(q)][d] for both images, q = 8 (2 s + h) + e  <->  jl = 16 s + 8 (e >> 2) + 4 h + (e & 3):
// the k order of an accumulator tile used as an MFMA operand (file header).  32 x 32 tiles through LDS.
__global__ __launch_bounds__(256) void ntxent_transpose_kernel(const unsigned short* __restrict__ fhi, const unsigned short* __restrict__ flo,
                                                               int Np, int Dp, unsigned short* __restrict__ fthi,
                                                               unsigned short* __restrict__ ftlo) {
    __shared__ unsigned short th[32][34], tl[32][34];
    const int j0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    for (int idx = threadIdx.x; idx < 1024; idx += 256) {
        const int jl = idx >> 5, dl = idx & 31;
        th[jl][dl] = fhi[(size_t)(j0 + jl) * Dp + d0 + dl];
        tl[jl][dl] = flo[(size_t)(j0 + jl) * Dp + d0 + dl];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 1024; idx += 256) {
        const int dl = idx >> 5, q = idx & 31;
        const int sh = q >> 3, e = q & 7;
        const int jl = 16 * (sh >> 1) + 8 * (e >> 2) + 4 * (sh & 1) + (e & 3);
        fthi[(size_t)(d0 + dl) * Np + j0 + q] = th[jl][dl];
        ftlo[(size_t)(d0 + dl) * Np + j0 + q] = tl[jl][dl];
    }
}

// g[i][d] = sum_j W_ij fh_j[d] for 32 rows i (blockIdx.x) and 256 columns d (blockIdx.y; wave w owns 64 of them).
// Per 128 columns j: every wave recomputes one 32 x 32 similarity tile, forms W^T in registers, leaves it in LDS as bf16 hi / lo
// A fragments; after the barrier every wave multiplies all four into its own output columns.
__global__ __launch_bounds__(256) void ntxent_bwd_kernel(const unsigned short* __restrict__ fhi, const unsigned short* __restrict__ flo,
                                                         const unsigned short* __restrict__ fthi, const unsigned short* __restrict__ ftlo,
                                                         const float* __restrict__ lse, int N, int Np, int Dp, float inv_t,
                                                         float* __restrict__ g) {
    __shared__ bf16x8 wl[4][2][2][64];   // [tile][k-step][hi, lo][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * 32, i = i0 + c;
    const int dbase = blockIdx.y * (128 * NTX_BWD_NSUB) + wave * (32 * NTX_BWD_NSUB);
    int partner = i + (N >> 1);
    if (partner >= N) partner -= N;
    const float lse_i = lse[i];
    const float inv_n = 1.0f / (float)N;
    const size_t boff = (size_t)i * Dp + 8 * h;
    f32x16 z[NTX_BWD_NSUB];
#pragma unroll
    for (int n = 0; n < NTX_BWD_NSUB; ++n) z[n] = (f32x16){};
    for (int js = 0; js < N; js += 128) {
        const int j0 = js + wave * 32;
        float w[16];
        if (j0 < N) {
            const size_t aoff = (size_t)(j0 + c) * Dp + 8 * h;
            const f32x16 acc = ntxent_tile(fhi + aoff, flo + aoff, fhi + boff, flo + boff, Dp);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 lj = *(const float4*)(lse + j0 + 8 * q + 4 * h);
                const float ljv[4] = {lj.x, lj.y, lj.z, lj.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * q + e;
                    const int j = j0 + 8 * q + 4 * h + e;
                    const float x = acc[r] * inv_t;
                    const float t = __expf(x - lse_i) + __expf(x - ljv[e]) - (j == partner ? 2.0f : 0.f);
                    w[r] = (i < N && j < N && j != i) ? t * inv_n : 0.f;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) w[r] = 0.f;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            unsigned hi4[4], lo4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = w[8 * s + 2 * e], b = w[8 * s + 2 * e + 1];
                const unsigned ph = pack2bf(a, b);
                const float ra = a - __builtin_bit_cast(float, ph << 16), rb = b - __builtin_bit_cast(float, ph & 0xffff0000u);
                hi4[e] = ph;
                lo4[e] = pack2bf(ra, rb);
            }
            wl[wave][s][0][lane] = __builtin_bit_cast(bf16x8, (uint4){hi4[0], hi4[1], hi4[2], hi4[3]});
            wl[wave][s][1][lane] = __builtin_bit_cast(bf16x8, (uint4){lo4[0], lo4[1], lo4[2], lo4[3]});
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (js + t * 32 < N) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 wh = wl[t][s][0][lane], wlo = wl[t][s][1][lane];
#pragma unroll
                    for (int n = 0; n < NTX_BWD_NSUB; ++n) {
                        const int d0 = dbase + 32 * n;
                        if (d0 < Dp) {
                            const size_t off = (size_t)(d0 + c) * Np + js + t * 32 + (2 * s + h) * 8;
                            const bf16x8 bh = *(const bf16x8*)(fthi + off), bl = *(const bf16x8*)(ftlo + off);
                            z[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, bh, z[n], 0, 0, 0);
                            z[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, bl, z[n], 0, 0, 0);
                            z[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, bh, z[n], 0, 0, 0);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int n = 0; n < NTX_BWD_NSUB; ++n) {
        const int d0 = dbase + 32 * n;
        if (d0 < Dp) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row < N) g[(size_t)row * Dp + d0 + c] = z[n][r];
            }
        }
    }
}

// one wave per row: df = s * inv_norm * (g - fh <g, fh>), s = (dloss ? *dloss : 1) / tau.  A row whose norm was clamped to eps has
// no projection term (F.normalize's clamp_min passes no gradient to the norm there).
__global__ __launch_bounds__(256) void ntxent_bwd_rows_kernel(const float* __restrict__ f, const float* __restrict__ g,
                                                              const float* __restrict__ inv_norm, int N, int D, int Dp, float inv_t,
                                                              const float* __restrict__ dloss, float* __restrict__ df) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float inv = inv_norm[row];
    const float* fr = f + (size_t)row * D;
    const float* gr = g + (size_t)row * Dp;
    float dot = 0.f;
    for (int c = lane; c < D; c += 64) dot += gr[c] * (fr[c] * inv);
    dot = wave_sum(dot);
    if (inv >= 1.0f / 1e-12f) dot = 0.f;
    const float sc = (dloss != nullptr ? dloss[0] : 1.0f) * inv_t * inv;
    for (int c = lane; c < D; c += 64) df[(size_t)row * D + c] = sc * (gr[c] - (fr[c] * inv) * dot);
}

struct NtxWs {
    unsigned short *fhi, *flo;     // [Np, Dp]
    unsigned short *fthi, *ftlo;   // [Dp, Np], j permuted within groups of 32 (backward)
    float* g;                      // [Np, Dp]: d loss / d fh * tau (backward)
    float *inv_norm, *lse;         // [Np]
    float4* part;                  // [nslice, Np]: per column slice (running max, sum, partner logit, best negative) of every row
    int Np, Dp, nslice;
    size_t total;
};

static NtxWs ntx_carve(void* base, int N, int D) {
    NtxWs w;
    w.Np = (N + 127) / 128 * 128;
    w.Dp = (D + 31) / 32 * 32;
    Carver c(base);
    const size_t nd = (size_t)w.Np * w.Dp;
    w.fhi = c.take<unsigned short>(nd);
    w.flo = c.take<unsigned short>(nd);
    w.fthi = c.take<unsigned short>(nd);
    w.ftlo = c.take<unsigned short>(nd);
    w.g = c.take<float>(nd);
    w.inv_norm = c.take<float>(w.Np);
    w.lse = c.take<float>(w.Np);
    w.nslice = w.Np / 128 < NTX_FWD_SLICES ? w.Np / 128 : NTX_FWD_SLICES;   // a function of N alone: the summation order is fixed
    w.part = c.take<float4>((size_t)w.nslice * w.Np);
    w.total = c.total();
    return w;
}

static int ntx_check(const char* op, const float* f, int N, int D, const void* ws, size_t ws_bytes) {
    const char* why = nullptr;
    if (!f) why = "null feature pointer";
    else if (N < 4) why = "N must be at least 4 (two views of two samples)";
    else if (N % 2 != 0) why = "N must be even (two views per sample)";
    else if (D < 1) why = "D must be at least 1";
    else if (N > (1 << 24) || D > (1 << 20)) why = "shape too large";
    else if (!ws) why = "null workspace pointer";
    else if (!aligned16(ws)) why = "workspace must be 16-byte aligned";
    else if (ws_bytes < ntx_carve(nullptr, N, D).total) why = "workspace too small (clibd_ntxent_workspace_bytes)";
    return why ? fail(op, why) : 0;
}

}  // namespace clibd

using namespace clibd;

extern "C" size_t clibd_ntxent_workspace_bytes(int N, int D) {
    if (N <= 0 || D <= 0) return 0;
    return ntx_carve(nullptr, N, D).total;
}

extern "C" int clibd_ntxent_fwd(const float* f, int N, int D, float inv_temperature, float* loss, int* top1_hits, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (int e = ntx_check("ntxent_fwd", f, N, D, workspace, workspace_bytes)) return e;
    if (!loss) return set_error(CLIBD_EINVAL, "ntxent_fwd: null loss pointer");
    if (!(inv_temperature > 0.f)) return set_error(CLIBD_EINVAL, "ntxent_fwd: inv_temperature must be positive");
    const NtxWs w = ntx_carve(workspace, N, D);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ntxent_prep_kernel, dim3(w.Np / 4), dim3(256), 0, st, f, N, w.Np, D, w.Dp, w.fhi, w.flo, w.inv_norm, w.lse);
    if (int e = check_launch("ntxent_fwd (prepare)")) return e;
    hipLaunchKernelGGL(ntxent_fwd_kernel, dim3((N + 31) / 32, w.nslice), dim3(256), 0, st, w.fhi, w.flo, N, w.Np, w.Dp, inv_temperature, w.part);
    if (int e = check_launch("ntxent_fwd")) return e;
    hipLaunchKernelGGL(ntxent_reduce_kernel, dim3(1), dim3(256), 0, st, w.part, w.nslice, N, w.Np, w.lse, loss, top1_hits);
    return check_launch("ntxent_fwd (mean)");
}

extern "C" int clibd_ntxent_bwd(const float* f, int N, int D, float inv_temperature, const float* dloss, float* df, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (int e = ntx_check("ntxent_bwd", f, N, D, workspace, workspace_bytes)) return e;
    if (!df) return set_error(CLIBD_EINVAL, "ntxent_bwd: null gradient pointer");
    if (!(inv_temperature > 0.f)) return set_error(CLIBD_EINVAL, "ntxent_bwd: inv_temperature must be positive");
    const NtxWs w = ntx_carve(workspace, N, D);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ntxent_transpose_kernel, dim3(w.Np / 32, w.Dp / 32), dim3(256), 0, st, w.fhi, w.flo, w.Np, w.Dp, w.fthi, w.ftlo);
    if (int e = check_launch("ntxent_bwd (transpose)")) return e;
    const int dchunk = 128 * NTX_BWD_NSUB;
    hipLaunchKernelGGL(ntxent_bwd_kernel, dim3((N + 31) / 32, (w.Dp + dchunk - 1) / dchunk), dim3(256), 0, st, w.fhi, w.flo, w.fthi, w.ftlo,
                       w.lse, N, w.Np, w.Dp, inv_temperature, w.g);
    if (int e = check_launch("ntxent_bwd")) return e;
    hipLaunchKernelGGL(ntxent_bwd_rows_kernel, dim3((N + 3) / 4), dim3(256), 0, st, f, w.g, w.inv_norm, N, D, w.Dp, inv_temperature, dloss, df);
    return check_launch("ntxent_bwd (rows)");
}
