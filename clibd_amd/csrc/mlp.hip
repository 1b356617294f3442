// The linear layers of the pre-extracted-feature towers (reference: bioscanclip/model/mlp.py, MLPEncoder) for gfx950, at the loss
// path's accuracy and one launch per role:
//
//   forward   out[B,N] = act(x[B,K] w[N,K]^T + bias)          dgrad   dx[B,K] = (dy[B,N] w[N,K]) * [h > 0]
//   wgrad     dw[N,K] (+)= dy[B,N]^T x[B,K],  db[N] (+)= sum_b dy[b,:]
//
// All three are C[m,n] = sum_c A(m,c) B(n,c) over fp32 operands.  A workgroup (256 threads, a 64 x 64 output tile, 32 of the
// contraction per step) reads fp32 tiles with 16-byte loads and splits them on the way into LDS: v = hi + lo, hi = bf16(v),
// lo = bf16(v - hi); the LDS images are [row][c] bf16 with the contraction innermost, which is what an MFMA fragment reads (8 consecutive
// c per lane, one ds_read_b128).  An operand whose contraction index is its ROW in memory (w in the dgrad, dy and x in the wgrad) is
// transposed by the same write pass: a thread loads two rows c, c + 1 of four columns and writes four packed pairs.  Each wave owns
// 32 x 32 of the tile (2 x 2 MFMA 16x16x32 tiles) and accumulates hi·hi + hi·lo + lo·hi in one fp32 accumulator.  The next step's
// global loads are issued before the current step's MFMAs.  Epilogues (bias, ReLU, the ReLU mask, accumulate) run on the accumulator
// registers.  No float atomics and no split of the contraction across workgroups: every output element has one summation order.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_mlp.h"
#include "host_util.h"

namespace clibd {

constexpr int MLP_T = 64;     // output tile edge
constexpr int MLP_BK = 32;    // contraction per step = one MFMA 16x16x32
constexpr int MLP_LD = 40;    // bf16 per LDS row: 80 bytes keep rows 16-byte aligned and spread 16 rows over all 16 slots of a bank row
constexpr int MLP_IMG = MLP_T * MLP_LD;   // one image (hi or lo of one operand), in bf16

enum MlpRole { MLP_FWD = 0, MLP_DGRAD = 1, MLP_WGRAD = 2 };

struct MlpArgs {
    const float* A; int lda;    // FWD: x [M,Kc]     DGRAD: dy [M,Kc]          WGRAD: dy [Kc,M] (contraction = its rows)
    const float* B; int ldb;    // FWD: w [N,Kc]     DGRAD: w [Kc,N] (rows)    WGRAD: x [Kc,N] (rows)
    int M, N, Kc;
    const float* aux;           // FWD: bias[N] or null    DGRAD: h [M,N] or null
    float* out;                 // [M,N], ld = N
    float* db;                  // WGRAD: [M] or null
    int flag;                   // FWD: relu    WGRAD: accumulate
};

// two fp32 -> the packed hi pair and the packed lo pair
__device__ __forceinline__ void mlp_split2(float a, float b, unsigned& hi, unsigned& lo) {
    hi = pack2bf(a, b);
    const float ha = __builtin_bit_cast(float, hi << 16), hb = __builtin_bit_cast(float, hi & 0xffff0000u);
    lo = pack2bf(a - ha, b - hb);
}

// One operand tile (64 rows x 32 of the contraction) as two float4 per thread (named registers: an indexed pair went to scratch);
// everything outside the matrix is zero.
// TR = false: memory is [row][c]; thread -> rows (tid >> 3) and + 32, c = 4 (tid & 7) .. + 3.
// TR = true:  memory is [c][row]; thread -> c = 2 (tid & 15), + 1, rows 4 (tid >> 4) .. + 3.
template <bool TR>
__device__ __forceinline__ void mlp_load(const float* __restrict__ src, int ld, int rows, int Kc, int r0, int c0, int tid, float4& v0, float4& v1) {
    v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!TR) {
        const int c = c0 + (tid & 7) * 4;   // Kc % 4 == 0: a float4 is inside or outside as a whole
        const int r = r0 + (tid >> 3);
        if (r < rows && c < Kc) v0 = *(const float4*)(src + (size_t)r * ld + c);
        if (r + 32 < rows && c < Kc) v1 = *(const float4*)(src + (size_t)(r + 32) * ld + c);
    } else {
        const int r = r0 + (tid >> 4) * 4;  // rows % 4 == 0
        const int c = c0 + 2 * (tid & 15);
        if (c < Kc && r < rows) v0 = *(const float4*)(src + (size_t)c * ld + r);
        if (c + 1 < Kc && r < rows) v1 = *(const float4*)(src + (size_t)(c + 1) * ld + r);
    }
}

template <bool TR>
__device__ __forceinline__ void mlp_store(unsigned short* __restrict__ hi, unsigned short* __restrict__ lo, int tid, const float4 v0, const float4 v1) {
    unsigned h0, l0, h1, l1;
    if (!TR) {
        const int off = (tid >> 3) * MLP_LD + (tid & 7) * 4;
        mlp_split2(v0.x, v0.y, h0, l0);
        mlp_split2(v0.z, v0.w, h1, l1);
        *(uint2*)(hi + off) = make_uint2(h0, h1);
        *(uint2*)(lo + off) = make_uint2(l0, l1);
        mlp_split2(v1.x, v1.y, h0, l0);
        mlp_split2(v1.z, v1.w, h1, l1);
        *(uint2*)(hi + off + 32 * MLP_LD) = make_uint2(h0, h1);
        *(uint2*)(lo + off + 32 * MLP_LD) = make_uint2(l0, l1);
    } else {
        const int off = (tid >> 4) * 4 * MLP_LD + 2 * (tid & 15);
        mlp_split2(v0.x, v1.x, h0, l0);
        *(unsigned*)(hi + off) = h0; *(unsigned*)(lo + off) = l0;
        mlp_split2(v0.y, v1.y, h0, l0);
        *(unsigned*)(hi + off + MLP_LD) = h0; *(unsigned*)(lo + off + MLP_LD) = l0;
        mlp_split2(v0.z, v1.z, h0, l0);
        *(unsigned*)(hi + off + 2 * MLP_LD) = h0; *(unsigned*)(lo + off + 2 * MLP_LD) = l0;
        mlp_split2(v0.w, v1.w, h0, l0);
        *(unsigned*)(hi + off + 3 * MLP_LD) = h0; *(unsigned*)(lo + off + 3 * MLP_LD) = l0;
    }
}

template <int ROLE>
__global__ __launch_bounds__(256) void mlp_linear_kernel(const MlpArgs a) {
    constexpr bool TRA = ROLE == MLP_WGRAD, TRB = ROLE != MLP_FWD;
    __shared__ __attribute__((aligned(16))) unsigned short lds[4 * MLP_IMG];   // A hi | A lo | B hi | B lo: 20 KiB
    unsigned short* const sAh = lds;
    unsigned short* const sAl = lds + MLP_IMG;
    unsigned short* const sBh = lds + 2 * MLP_IMG;
    unsigned short* const sBl = lds + 3 * MLP_IMG;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * MLP_T, n0 = blockIdx.x * MLP_T;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int fr = lane & 15, fq = lane >> 4;

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const bool want_db = ROLE == MLP_WGRAD && a.db != nullptr && blockIdx.x == 0;
    float4 dbs = make_float4(0.f, 0.f, 0.f, 0.f);   // WGRAD: this thread's share of sum_b dy[b, m0 + 4 (tid >> 4) ..], rows b = 2 (tid & 15), + 1 mod 32

    float4 va0, va1, vb0, vb1;
    mlp_load<TRA>(a.A, a.lda, a.M, a.Kc, m0, 0, tid, va0, va1);
    mlp_load<TRB>(a.B, a.ldb, a.N, a.Kc, n0, 0, tid, vb0, vb1);
    for (int c0 = 0; c0 < a.Kc; c0 += MLP_BK) {
        mlp_store<TRA>(sAh, sAl, tid, va0, va1);
        mlp_store<TRB>(sBh, sBl, tid, vb0, vb1);
        if (want_db) {
            dbs.x = (dbs.x + va0.x) + va1.x; dbs.y = (dbs.y + va0.y) + va1.y;
            dbs.z = (dbs.z + va0.z) + va1.z; dbs.w = (dbs.w + va0.w) + va1.w;
        }
        __syncthreads();
        if (c0 + MLP_BK < a.Kc) {
            mlp_load<TRA>(a.A, a.lda, a.M, a.Kc, m0, c0 + MLP_BK, tid, va0, va1);
            mlp_load<TRB>(a.B, a.ldb, a.N, a.Kc, n0, c0 + MLP_BK, tid, vb0, vb1);
        }
        bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ao = (wm + 16 * i + fr) * MLP_LD + 8 * fq, bo = (wn + 16 * i + fr) * MLP_LD + 8 * fq;
            ah[i] = *(const bf16x8*)(sAh + ao);
            al[i] = *(const bf16x8*)(sAl + ao);
            bh[i] = *(const bf16x8*)(sBh + bo);
            bl[i] = *(const bf16x8*)(sBl + bo);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            }
        __syncthreads();
    }

    // accumulator element r of tile (i, j): row m0 + wm + 16 i + 4 fq + r, column n0 + wn + 16 j + fr
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn + 16 * j + fr;
            if (n >= a.N) continue;
            const float bias = (ROLE == MLP_FWD && a.aux != nullptr) ? a.aux[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + 4 * fq + r;
                if (m >= a.M) continue;
                const size_t o = (size_t)m * a.N + n;
                float v = acc[i][j][r];
                if (ROLE == MLP_FWD) {
                    v += bias;
                    if (a.flag) v = v < 0.f ? 0.f : v;
                } else if (ROLE == MLP_DGRAD) {
                    if (a.aux != nullptr) v = a.aux[o] > 0.f ? v : 0.f;
                } else if (a.flag) {
                    v += a.out[o];
                }
                a.out[o] = v;
            }
        }

    if (ROLE == MLP_WGRAD && want_db) {
        // the loop's last barrier has passed: the operand images are dead.  red[kp][64] fp32 = 4 KiB over them.
        float* red = (float*)lds;
        *(float4*)(red + (tid & 15) * MLP_T + (tid >> 4) * 4) = dbs;
        __syncthreads();
        if (tid < MLP_T && m0 + tid < a.M) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s += red[k * MLP_T + tid];
            a.db[m0 + tid] = a.flag ? a.db[m0 + tid] + s : s;
        }
    }
}

constexpr int kMlpMaxDim = 4096, kMlpMaxRows = 1 << 21;

static int mlp_shape_check(const char* op, int B, int N, int K) {
    if (B <= 0 || N <= 0 || K <= 0) return fail(op, "non-positive shape");
    if (B > kMlpMaxRows) return fail(op, "B above 2^21");
    if (K % 4 != 0) return fail(op, "the input width K must be a multiple of 4");
    if (N % 16 != 0) return fail(op, "the output width N must be a multiple of 16");
    if (K > kMlpMaxDim || N > kMlpMaxDim) return fail(op, "K and N must be at most 4096");
    return 0;
}

template <int ROLE>
static int mlp_launch(const char* op, const MlpArgs& a, void* stream) {
    const dim3 grid((a.N + MLP_T - 1) / MLP_T, (a.M + MLP_T - 1) / MLP_T);
    hipLaunchKernelGGL(mlp_linear_kernel<ROLE>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return check_launch(op);
}

}  // namespace clibd

using namespace clibd;

extern "C" int clibd_mlp_linear_fwd(const float* x, const float* w, const float* bias, int B, int N, int K, int relu, float* out, void* stream) {
    if (int e = mlp_shape_check("mlp_linear_fwd", B, N, K)) return e;
    if (!x || !w || !out) return fail("mlp_linear_fwd", "null pointer");
    if (!aligned16(x) || !aligned16(w)) return fail("mlp_linear_fwd", "x and w must be 16-byte aligned");
    const MlpArgs a = {x, K, w, K, B, N, K, bias, out, nullptr, relu != 0};
    return mlp_launch<MLP_FWD>("mlp_linear_fwd", a, stream);
}

extern "C" int clibd_mlp_linear_dgrad(const float* dy, const float* w, const float* h, int B, int N, int K, float* dx, void* stream) {
    if (int e = mlp_shape_check("mlp_linear_dgrad", B, N, K)) return e;
    if (!dy || !w || !dx) return fail("mlp_linear_dgrad", "null pointer");
    if (!aligned16(dy) || !aligned16(w)) return fail("mlp_linear_dgrad", "dy and w must be 16-byte aligned");
    const MlpArgs a = {dy, N, w, K, B, K, N, h, dx, nullptr, 0};   // dx[B,K]: the contraction runs over N, the rows of w
    return mlp_launch<MLP_DGRAD>("mlp_linear_dgrad", a, stream);
}

extern "C" int clibd_mlp_linear_wgrad(const float* dy, const float* x, int B, int N, int K, float* dw, float* db, int accumulate,
                                      void* stream) {
    if (int e = mlp_shape_check("mlp_linear_wgrad", B, N, K)) return e;
    if (!dy || !x || !dw) return fail("mlp_linear_wgrad", "null pointer");
    if (!aligned16(dy) || !aligned16(x)) return fail("mlp_linear_wgrad", "dy and x must be 16-byte aligned");
    const MlpArgs a = {dy, N, x, K, N, K, B, nullptr, dw, db, accumulate != 0};   // dw[N,K]: the contraction runs over B, the rows of dy and x
    return mlp_launch<MLP_WGRAD>("mlp_linear_wgrad", a, stream);
}
