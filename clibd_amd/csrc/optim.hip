// The optimizer beyond one plain update for gfx950 (clibd_hip_optim.h): the global gradient norm in a fixed order, the clip coefficient
// and skip decision in a device record, and AdamW / Adam(L2) with per-group lr and weight decay reading that record.
//
// Norm.  Pass 1 cuts the bucket into chunks of NORM_CHUNK floats, a constant: the partials, and so the bits of the result, do not depend
// on the grid or on the number of CUs.  One workgroup per chunk, 16 float4 per thread (coalesced: consecutive threads, consecutive
// float4), fp32 fma accumulation, wave_sum, the four wave totals through LDS in order.  Pass 2 is ONE workgroup: thread j adds partials
// j, j + 256, ... in fp64, a fixed LDS tree follows, thread 0 writes the record.  No atomics.
//
// Update.  adamw_kernel / adam_l2_kernel of elementwise.hip with the same per-element expressions; float4 accesses (4 read and 3 write
// streams, bandwidth-bound), the group of a float4 looked up from a by-value table (at most 7 compares; group starts are multiples of
// 64 floats, so a float4, and a whole 64-float granule, never straddles two groups).  The record is read once per thread (a uniform
// address): skip_now set returns before any store.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_optim.h"
#include "host_util.h"
#include "grad_norm_pass1.h"

namespace clibd {

static_assert(NORM_CHUNK == CLIBD_GRAD_NORM_CHUNK, "the chunk is part of the ABI");

struct GroupTable {
    unsigned long long first[CLIBD_OPTIM_MAX_GROUPS];
    float lr[CLIBD_OPTIM_MAX_GROUPS];
    float wd[CLIBD_OPTIM_MAX_GROUPS];
    int count;
};

__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, size_t n, float* __restrict__ partials) {
    __shared__ float wave_tot[OPT_WAVES];
    grad_sumsq_chunk(g, n, partials, wave_tot);   // grad_norm_pass1.h: the one source of pass 1, shared with accum.hip
}

__global__ __launch_bounds__(OPT_THREADS) void grad_norm_finish_kernel(const float* __restrict__ partials, unsigned chunks, float grad_scale,
                                                                       float max_norm, int skip_nonfinite,
                                                                       clibd_grad_record* __restrict__ rec) {
    __shared__ double part[OPT_THREADS];
    const int t = threadIdx.x;
    double s = 0.0;
    for (unsigned j = t; j < chunks; j += OPT_THREADS) s += (double)partials[j];
    part[t] = s;
    __syncthreads();
    for (int d = OPT_THREADS / 2; d > 0; d >>= 1) {
        if (t < d) part[t] = part[t] + part[t + d];
        __syncthreads();
    }
    if (t == 0) {
        const float total = (float)((double)grad_scale * sqrt(part[0]));
        float coef = 1.0f;
        if (max_norm > 0.f) {
            const float c = max_norm / (total + 1e-6f);
            coef = c < 1.0f ? c : (c != c ? c : 1.0f);   // torch's clamp(max=1): a NaN stays a NaN
        }
        const int skip = (skip_nonfinite != 0 && !(fabsf(total) <= 3.402823466e38f)) ? 1 : 0;
        rec->total_norm = total;
        rec->coef = coef;
        rec->skip_now = skip;
        rec->skipped_total = rec->skipped_total + skip;
    }
}

// The per-element operations of adamw_kernel / adam_l2_kernel (elementwise.hip).  Which a * b + c of those two kernels becomes one fma is
// the compiler's choice there (it depends on how their scalar loops were vectorised), and the same source inside a float4 loop is fused
// differently.  So contraction is off here and the fused operations are written out as the built kernels perform them: AdamW fuses only
// 1 - lr * wd; Adam(L2) fuses wd * p + g * grad_scale and p - (lr / bc1) * (m / denom).  Every other product and sum rounds on its own.
template <bool L2>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float lr, float beta1, float beta2, float eps, float wd,
                                            float bc1, float bc2_sqrt, float grad_scale) {
#pragma clang fp contract(off)
    float pi = p;
    float gi = g * grad_scale;
    if constexpr (L2) gi = fmaf(wd, pi, gi);
    else pi = pi * fmaf(-lr, wd, 1.0f);
    const float mi = beta1 * m + (1.0f - beta1) * gi;
    const float vi = beta2 * v + (1.0f - beta2) * gi * gi;
    m = mi;
    v = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    if constexpr (L2) p = fmaf(-(lr / bc1), mi / denom, pi);
    else p = pi - (lr / bc1) * (mi / denom);
}

template <bool L2>
__global__ __launch_bounds__(OPT_THREADS) void adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                  float* __restrict__ v, size_t n, GroupTable tab, float beta1, float beta2,
                                                                  float eps, float bc1, float bc2_sqrt, float grad_scale,
                                                                  const clibd_grad_record* __restrict__ rec) {
    if (rec != nullptr) {
        if (rec->skip_now != 0) return;   // a non-finite norm under skip: p, m and v keep their bits
        grad_scale = grad_scale * rec->coef;
    }
    const size_t units = (n + 3) / 4;
    for (size_t u = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x; u < units; u += (size_t)gridDim.x * OPT_THREADS) {
        const size_t i = u * 4;
        float lr = tab.lr[0], wd = tab.wd[0];
#pragma unroll
        for (int k = 1; k < CLIBD_OPTIM_MAX_GROUPS; ++k) {   // ascending starts: the last group that begins at or before i
            const bool in = k < tab.count && (unsigned long long)i >= tab.first[k];
            lr = in ? tab.lr[k] : lr;
            wd = in ? tab.wd[k] : wd;
        }
        if (i + 3 < n) {
            float4 p4 = *(const float4*)(p + i), m4 = *(const float4*)(m + i), v4 = *(const float4*)(v + i);
            const float4 g4 = *(const float4*)(g + i);
            adam_update<L2>(p4.x, g4.x, m4.x, v4.x, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale);
            adam_update<L2>(p4.y, g4.y, m4.y, v4.y, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale);
            adam_update<L2>(p4.z, g4.z, m4.z, v4.z, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale);
            adam_update<L2>(p4.w, g4.w, m4.w, v4.w, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale);
            *(float4*)(m + i) = m4;
            *(float4*)(v + i) = v4;
            *(float4*)(p + i) = p4;
        } else {   // n is no multiple of 4: the last one to three elements
            for (size_t e = i; e < n; ++e) {
                float pe = p[e], me = m[e], ve = v[e];
                adam_update<L2>(pe, g[e], me, ve, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale);
                m[e] = me;
                v[e] = ve;
                p[e] = pe;
            }
        }
    }
}

template <bool L2>
static int step_groups(const char* op, float* p, const float* g, float* m, float* v, size_t n, const clibd_optim_group* groups, int n_groups,
                       float beta1, float beta2, float eps, int step, float grad_scale, const void* record, void* stream) {
    if (!p || !g || !m || !v || !groups) return fail(op, "null pointer");
    if (step < 1) return fail(op, "step must be >= 1");
    if (n_groups < 1 || n_groups > CLIBD_OPTIM_MAX_GROUPS) return fail(op, "n_groups must be in 1..8");
    if (groups[0].first != 0) return fail(op, "the first group must start at 0");
    GroupTable tab;
    for (int k = 0; k < CLIBD_OPTIM_MAX_GROUPS; ++k) {
        const bool live = k < n_groups;
        if (live && groups[k].first % CLIBD_OPTIM_GROUP_ALIGN != 0) return fail(op, "group starts must be multiples of 64");
        if (live && k > 0 && groups[k].first <= groups[k - 1].first) return fail(op, "group starts must be strictly ascending");
        tab.first[k] = live ? (unsigned long long)groups[k].first : ~0ull;
        tab.lr[k] = live ? groups[k].lr : 0.f;
        tab.wd[k] = live ? groups[k].weight_decay : 0.f;
    }
    tab.count = n_groups;
    if (n == 0) return CLIBD_OK;
    if (groups[n_groups - 1].first >= n) return fail(op, "group starts must lie below n");
    if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || (((uintptr_t)record) & 3u) != 0)
        return fail(op, "misaligned pointer (p, g, m, v 16 bytes, the record 4 bytes)");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2 = 1.0f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adam_groups_kernel<L2>, dim3(grid_for((n + 3) / 4)), dim3(OPT_THREADS), 0, (hipStream_t)stream, p, g, m, v, n, tab, beta1,
                       beta2, eps, bc1, sqrtf(bc2), grad_scale, (const clibd_grad_record*)record);
    return check_launch(op);
}

}  // namespace clibd

using namespace clibd;

extern "C" size_t clibd_grad_norm_workspace_bytes(size_t n) {
    const size_t c = norm_chunks(n);
    return align_up((c < 1 ? 1 : c) * sizeof(float), 256);
}

extern "C" int clibd_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, int skip_nonfinite, void* record, void* workspace,
                               size_t workspace_bytes, void* stream) {
    const char* op = "grad_norm";
    if (!g || !record || (!workspace && workspace_bytes == 0)) return fail(op, "null pointer");
    if (!(max_norm >= 0.f)) return fail(op, "max_norm must be positive, or 0 for no clipping");
    if (norm_chunks(n) > 0x7fffffffu) return fail(op, "n too large");
    if (int e = check_workspace(op, "workspace", workspace, workspace_bytes, clibd_grad_norm_workspace_bytes(n), "clibd_grad_norm_workspace_bytes"))
        return e;
    if (!aligned16(g) || (((uintptr_t)record) & 3u) != 0) return fail(op, "misaligned pointer (g 16 bytes, the record 4 bytes)");
    if (n == 0) return CLIBD_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned chunks = (unsigned)norm_chunks(n);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(chunks), dim3(OPT_THREADS), 0, st, g, n, (float*)workspace);
    if (int e = check_launch("grad_norm (partials)")) return e;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, st, (const float*)workspace, chunks, grad_scale, max_norm,
                       skip_nonfinite, (clibd_grad_record*)record);
    return check_launch(op);
}

extern "C" int clibd_adamw_step_groups(float* p, const float* g, float* m, float* v, size_t n, const struct clibd_optim_group* groups,
                                       int n_groups, float beta1, float beta2, float eps, int step, float grad_scale, const void* record,
                                       void* stream) {
    return step_groups<false>("adamw_step_groups", p, g, m, v, n, groups, n_groups, beta1, beta2, eps, step, grad_scale, record, stream);
}

extern "C" int clibd_adam_l2_step_groups(float* p, const float* g, float* m, float* v, size_t n, const struct clibd_optim_group* groups,
                                         int n_groups, float beta1, float beta2, float eps, int step, float grad_scale, const void* record,
                                         void* stream) {
    return step_groups<true>("adam_l2_step_groups", p, g, m, v, n, groups, n_groups, beta1, beta2, eps, step, grad_scale, record, stream);
}
