// Gradient accumulation's device side for gfx950 (clibd_hip_accum.h): clibd_grad_norm with a divisor that lives on the device.
//
// A window of k micro-batches on W ranks leaves the SUM of their gradients in the flat bucket; the number it has to be divided by — the
// labelled positions of the whole window — is known only on the device (it rode in the bucket's spare slots through the all-reduce).
// Pass 1 is optim.hip's, from the one source in grad_norm_pass1.h: the same chunks, the same partials.  Pass 2 repeats
// grad_norm_finish_kernel's fp64 fixed-order sum and then divides: total_norm = (float)(grad_scale * sqrt(sum) / d), coef =
// clip(total_norm) / d, d = max(*divisor, 1).  The unchanged grouped updates multiply the gradient by grad_scale * coef, so they apply the
// averaged, clipped gradient with no kernel of their own.  x / 1 is x in fp64 and in fp32: with d == 1 the record is clibd_grad_norm's.
// No atomics.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_optim.h"
#include "../../include/clibd_hip_accum.h"
#include "host_util.h"
#include "grad_norm_pass1.h"

namespace clibd {

static_assert(NORM_CHUNK == CLIBD_GRAD_NORM_CHUNK, "the chunk is part of the ABI");

__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_div_kernel(const float* __restrict__ g, size_t n, float* __restrict__ partials) {
    __shared__ float wave_tot[OPT_WAVES];
    grad_sumsq_chunk(g, n, partials, wave_tot);
}

__global__ __launch_bounds__(OPT_THREADS) void grad_norm_div_finish_kernel(const float* __restrict__ partials, unsigned chunks, float grad_scale,
                                                                           float max_norm, int skip_nonfinite,
                                                                           const float* __restrict__ divisor,
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
        float d = 1.0f;
        if (divisor != nullptr) {
            const float x = *divisor;
            d = x > 1.0f ? x : 1.0f;   // max(x, 1), the rule of clibd_mlm_ce_bf16's n_valid; a NaN count divides by 1
        }
        const float total = (float)((double)grad_scale * sqrt(part[0]) / (double)d);
        float coef = 1.0f;
        if (max_norm > 0.f) {
            const float c = max_norm / (total + 1e-6f);
            coef = c < 1.0f ? c : (c != c ? c : 1.0f);   // torch's clamp(max=1): a NaN stays a NaN
        }
        coef = coef / d;
        const int skip = (skip_nonfinite != 0 && !(fabsf(total) <= 3.402823466e38f)) ? 1 : 0;
        rec->total_norm = total;
        rec->coef = coef;
        rec->skip_now = skip;
        rec->skipped_total = rec->skipped_total + skip;
    }
}

}  // namespace clibd

using namespace clibd;

extern "C" size_t clibd_grad_norm_div_workspace_bytes(size_t n) {
    const size_t c = norm_chunks(n);
    return align_up((c < 1 ? 1 : c) * sizeof(float), 256);
}

extern "C" int clibd_grad_norm_div(const float* g, size_t n, float grad_scale, float max_norm, int skip_nonfinite, const float* divisor,
                                   void* record, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "grad_norm_div";
    if (!g || !record || (!workspace && workspace_bytes == 0)) return fail(op, "null pointer");
    if (!(max_norm >= 0.f)) return fail(op, "max_norm must be positive, or 0 for no clipping");
    if (norm_chunks(n) > 0x7fffffffu) return fail(op, "n too large");
    if (int e = check_workspace(op, "workspace", workspace, workspace_bytes, clibd_grad_norm_div_workspace_bytes(n),
                                "clibd_grad_norm_div_workspace_bytes"))
        return e;
    if (!aligned16(g) || (((uintptr_t)record) & 3u) != 0 || (((uintptr_t)divisor) & 3u) != 0)
        return fail(op, "misaligned pointer (g 16 bytes, the record and the divisor 4 bytes)");
    if (n == 0) return CLIBD_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned chunks = (unsigned)norm_chunks(n);
    hipLaunchKernelGGL(grad_sumsq_div_kernel, dim3(chunks), dim3(OPT_THREADS), 0, st, g, n, (float*)workspace);
    if (int e = check_launch("grad_norm_div (partials)")) return e;
    hipLaunchKernelGGL(grad_norm_div_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, st, (const float*)workspace, chunks, grad_scale, max_norm,
                       skip_nonfinite, divisor, (clibd_grad_record*)record);
    return check_launch(op);
}
