// The split-bf16 product module (split3.h) for gfx950: x · yᵀ at ~2^-16 relative accuracy on the bf16 MFMA GEMM, and both gradients, which
// split the coefficient matrix g like x and run on the K-concatenated transposed images, every contraction zero padded to whole 64-wide K tiles:
//        dx = [Ghi | Ghi | Glo] · [Yhi^T | Ylo^T | Yhi^T]^T          dy = [Ghi^T | Glo^T | Ghi^T] · [Xhi^T | Xhi^T | Xlo^T]^T
// Only the segment orders make the three cross terms pair up (a wrong one still gives a plausible number at bf16 accuracy), so they are
// named here and nowhere else.  Every product goes through clibd_gemm_bf16_nt with split_k = 1: one summation order.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "split3.h"

namespace clibd {

// which segment of a [R, 3W] source image each of the three transposed segments reads, 2 bits each
constexpr int seg_map(int k0, int k1, int k2) { return k0 | (k1 << 2) | (k2 << 4); }
constexpr int SEG_SAME = seg_map(0, 1, 2);     // the image's own order: x3 -> xT and y3 -> yT
constexpr int SEG_X_AS_Y = seg_map(0, 2, 0);   // [hi|hi|lo] read as hi, lo, hi: G -> GT, the y-side order that pairs with xT

// img3[r, 0:Cp] = hi, img3[r, Cp:2Cp] = MID, img3[r, 2Cp:3Cp] = LAST  with (MID,LAST) = (hi,lo) for x, (lo,hi) for y; zeros for c >= C
__global__ __launch_bounds__(256) void split3_image_kernel(const float* __restrict__ in, int ld_in, int R, int C, int Cp, int x_side,
                                                           unsigned short* __restrict__ out) {
    const size_t total = (size_t)R * Cp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / Cp;
        const int c = (int)(i - r * Cp);
        const float v = c < C ? in[r * (size_t)ld_in + c] : 0.f;
        const unsigned short hi = f2bf(v);
        const unsigned short lo = f2bf(v - bf2f(hi));
        unsigned short* o = out + r * 3 * (size_t)Cp;
        o[c] = hi;
        o[Cp + c] = x_side ? hi : lo;
        o[2 * Cp + c] = x_side ? lo : hi;
    }
}

// out[c, k * Rp + r] = in[r, seg(k) * W + c] for the three column segments of a [R, 3W] image (seg(k) = 2 bits of `map` each),
// c < C <= W, r < Rp with zeros for r >= R: the K-concatenated operand images of the backward GEMMs, transposed in one launch.
__global__ __launch_bounds__(256) void transpose3_bf16_kernel(const unsigned short* __restrict__ in, int R, int W, int C, int map,
                                                              unsigned short* __restrict__ out, int Rp) {
    __shared__ unsigned short tile[64][66];
    const int k = blockIdx.z;
    const int seg = (map >> (2 * k)) & 3;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < R && c < C) ? in[(size_t)r * 3 * W + (size_t)seg * W + c] : (unsigned short)0;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (c < C && r < Rp) out[(size_t)c * 3 * Rp + (size_t)k * Rp + r] = tile[tx][i];
    }
}

static int launch_transpose3(const unsigned short* in, int R, int W, int C, int map, unsigned short* out, int Rp, hipStream_t st) {
    hipLaunchKernelGGL(transpose3_bf16_kernel, dim3((C + 63) / 64, (Rp + 63) / 64, 3), dim3(256), 0, st, in, R, W, C, map, out, Rp);
    return check_launch("split-bf16 transpose3");
}

// out[M,N] (+)= A[M,K] · B[N,K]^T (+ bias[N])
static int product(const unsigned short* A, const unsigned short* B, int M, int N, int K, const float* bias, float* out, bool accumulate,
                   hipStream_t st) {
    clibd_gemm_epilogue ep = {};
    ep.split_k = 1;
    ep.bias = bias;
    ep.out_f32 = out;
    ep.ld_out_f32 = N;
    if (accumulate) { ep.residual_f32 = out; ep.ld_res = N; }   // in place through the residual path
    return clibd_gemm_bf16_nt(A, K, B, K, M, N, K, &ep, nullptr, 0, st);
}

void Split3Ws::carve(Carver& c, int M, int N, int D) {
    const size_t Np = pad64(N), Mp = pad64(M);
    x3 = c.take<unsigned short>((size_t)M * 3 * D);
    y3 = c.take<unsigned short>((size_t)pad16(N) * 3 * D);
    G = c.take<unsigned short>((size_t)M * 3 * Np);
    GT = c.take<unsigned short>((size_t)N * 3 * Mp);
    xT = c.take<unsigned short>((size_t)D * 3 * Mp);
    yT = c.take<unsigned short>((size_t)D * 3 * Np);
}

int split3_image(const float* in, int ld_in, int R, int C, int Cp, Split3Side side, unsigned short* out, unsigned grid, const char* what,
                 hipStream_t st) {
    hipLaunchKernelGGL(split3_image_kernel, dim3(grid), dim3(256), 0, st, in, ld_in, R, C, Cp, (int)side, out);
    return check_launch(what);
}

int split3_forward(const float* x, const float* y, int M, int N, int D, const float* bias16, float* out, const Split3Ws& ws, unsigned grid_x,
                   unsigned grid_y, const char* op, const char* what, hipStream_t st) {
    if (int e = split3_image(x, D, M, D, D, SPLIT3_X, ws.x3, grid_x, what, st)) return e;
    if (int e = split3_image(y, D, N, D, D, SPLIT3_Y, ws.y3, grid_y, what, st)) return e;
    const int N16 = pad16(N);   // the GEMM takes N in multiples of 16: rows N.. of the y image are zero
    if (N16 != N && hipMemsetAsync(ws.y3 + (size_t)N * 3 * D, 0, (size_t)(N16 - N) * 3 * D * 2, st) != hipSuccess) {
        snprintf(last_error_buf(), kErrBufLen, "%s: memset failed", op);
        return CLIBD_ELAUNCH;
    }
    return product(ws.x3, ws.y3, M, N16, 3 * D, bias16, out, false, st);
}

int split3_grad_left(float* dx, bool accumulate, int M, int N, int D, const Split3Ws& ws, hipStream_t st) {
    const int Np = pad64(N);
    if (int e = launch_transpose3(ws.y3, N, D, D, SEG_SAME, ws.yT, Np, st)) return e;
    return product(ws.G, ws.yT, M, D, 3 * Np, nullptr, dx, accumulate, st);
}

int split3_grad_right(float* dy, bool accumulate, int M, int N, int D, const Split3Ws& ws, hipStream_t st) {
    const int Np = pad64(N), Mp = pad64(M);
    if (int e = launch_transpose3(ws.G, M, Np, N, SEG_X_AS_Y, ws.GT, Mp, st)) return e;
    if (int e = launch_transpose3(ws.x3, M, D, D, SEG_SAME, ws.xT, Mp, st)) return e;
    return product(ws.GT, ws.xT, N, D, 3 * Mp, nullptr, dy, accumulate, st);
}

}  // namespace clibd
