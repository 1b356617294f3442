// Pass 1 of the gradient norm (include/clibd_hip_optim.h), shared by optim.hip and accum.hip: ONE source, so the partials of
// clibd_grad_norm and clibd_grad_norm_div are the same bits.  Each unit wraps grad_sumsq_chunk in a __global__ of its own name (two
// units cannot both define one kernel symbol); the wrapper adds nothing.
#pragma once
#include "common.h"

namespace clibd {

constexpr int OPT_THREADS = 256;
constexpr int OPT_WAVES = 4;
constexpr int NORM_F4_PER_THREAD = 16;
constexpr int NORM_CHUNK = OPT_THREADS * NORM_F4_PER_THREAD * 4;

static inline size_t norm_chunks(size_t n) { return (n + NORM_CHUNK - 1) / NORM_CHUNK; }

// Workgroup blockIdx.x owns the floats [blockIdx.x * NORM_CHUNK, + NORM_CHUNK): 16 float4 per thread (coalesced), fp32 fma accumulation,
// wave_sum, the four wave totals through LDS (`wave_tot`, OPT_WAVES floats) in order; one partial per chunk.
__device__ __forceinline__ void grad_sumsq_chunk(const float* __restrict__ g, size_t n, float* __restrict__ partials, float* wave_tot) {
    const size_t base = (size_t)blockIdx.x * NORM_CHUNK;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < NORM_F4_PER_THREAD; ++k) {
        const size_t i = base + ((size_t)k * OPT_THREADS + threadIdx.x) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i + 3 < n) {
            x = *(const float4*)(g + i);
        } else {   // the bucket's last float4, cut short by n
            if (i < n) x.x = g[i];
            if (i + 1 < n) x.y = g[i + 1];
            if (i + 2 < n) x.z = g[i + 2];
        }
        acc = fmaf(x.x, x.x, acc);
        acc = fmaf(x.y, x.y, acc);
        acc = fmaf(x.z, x.z, acc);
        acc = fmaf(x.w, x.w, acc);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((wave_tot[0] + wave_tot[1]) + wave_tot[2]) + wave_tot[3];
}

}  // namespace clibd
