// The split-bf16 operand images shared by the fp32-grade products (loss.hip: K9's similarity; classifier.hip: the linear-probe head).
//   v = hi + lo (bf16 each);  <x, y> ~ hi·hi + hi·lo + lo·hi  as ONE NT GEMM with K = 3D over [hi|hi|lo] (x side) and [hi|lo|hi] (y side).
// The kernels have internal linkage: each translation unit that includes this header carries its own copy of the host stubs.
#pragma once
#include "common.h"
#include "host_util.h"

namespace clibd {

// img3[r, 0:D] = hi, img3[r, D:2D] = MID, img3[r, 2D:3D] = LAST  with (MID,LAST) = (hi,lo) for x, (lo,hi) for y
static __global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ in, int R, int D, int x_side,
                                                            unsigned short* __restrict__ out) {
    const size_t total = (size_t)R * D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / D;
        const int c = (int)(i - r * D);
        const float v = in[i];
        const unsigned short hi = f2bf(v);
        const unsigned short lo = f2bf(v - bf2f(hi));
        unsigned short* o = out + r * 3 * (size_t)D;
        o[c] = hi;
        o[D + c] = x_side ? hi : lo;
        o[2 * D + c] = x_side ? lo : hi;
    }
}

// out[c, k * Rp + r] = in[r, seg(k) * W + c] for the three column segments of a [R, 3W] image (seg(k) = 2 bits of `map` each),
// c < C <= W, r < Rp with zeros for r >= R: the K-concatenated operand images of the backward GEMMs, transposed in one launch.
static __global__ __launch_bounds__(256) void transpose3_bf16_kernel(const unsigned short* __restrict__ in, int R, int W, int C, int map,
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

static inline int launch_transpose3(const unsigned short* in, int R, int W, int C, int map, unsigned short* out, int Rp, hipStream_t st) {
    dim3 grid((C + 63) / 64, (Rp + 63) / 64, 3);
    hipLaunchKernelGGL(transpose3_bf16_kernel, grid, dim3(256), 0, st, in, R, W, C, map, out, Rp);
    return check_launch("split-bf16 transpose3");
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int pad64(int v) { return (v + 63) / 64 * 64; }
static inline int pad16(int v) { return (v + 15) / 16 * 16; }

}  // namespace clibd
