/*
 * clibd_hip_optim.h — the optimizer's device side beyond one plain update in libclibd_hip.so (gfx950): the global L2 norm of the flat
 * gradient bucket in a fixed order, the clip coefficient and the non-finite skip decision it yields (a 16-byte device record), and the
 * AdamW / Adam(L2) update with per-group `lr` and `weight_decay` that reads that record.
 *
 * A thirteenth header beside clibd_hip.h and the eleven additive ones: the same library, the same conventions (extern "C", caller-owned
 * device buffers, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message prefixed by the entry's name, nothing
 * allocates or synchronises, arguments validated on the host before any launch).  The addition is purely additive — clibd_adamw_step and
 * clibd_adam_l2_step keep their signatures and their arithmetic — so the ABI version stays 7.  The Python binding keeps these symbols under this
 * header's name in clibd_amd._lib.HEADERS.
 *
 * There is no float atomic anywhere here: two runs on any box agree bit for bit, and deterministic mode needs no second form.
 *
 * Not here: norm types other than 2, clipping by value, per-group betas or eps, amsgrad, maximize, more than CLIBD_OPTIM_MAX_GROUPS groups,
 * LAMB / LARS, gradient accumulation, a device-side step counter.
 */
#ifndef CLIBD_HIP_OPTIM_H
#define CLIBD_HIP_OPTIM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIBD_OPTIM_MAX_GROUPS 8       /* the most parameter groups one update takes */
#define CLIBD_OPTIM_GROUP_ALIGN 64     /* every group starts on a multiple of this many floats (the optimizer's parameter alignment) */
#define CLIBD_GRAD_NORM_CHUNK 16384    /* floats per pass-1 partial: 256 threads x 16 float4, a constant of the ABI (not of the device) */

/* The record of one norm launch, 16 bytes in device memory, 4-byte aligned.  The caller zeroes it once: skipped_total accumulates. */
struct clibd_grad_record {
    float total_norm;       /* grad_scale * sqrt(sum g[i]^2): what clip_grad_norm_ returns for the averaged gradient */
    float coef;             /* max_norm > 0: min(1, max_norm / (total_norm + 1e-6)) in fp32, NaN where total_norm is NaN (torch's clamp);
                               max_norm == 0: 1 */
    int32_t skip_now;       /* 1 iff skip_nonfinite != 0 and total_norm is inf or NaN, else 0 */
    int32_t skipped_total;  /* += skip_now */
};

/* One parameter group: the elements [first, next group's first) of the bucket (the last group ends at n). */
struct clibd_optim_group {
    size_t first;
    float lr;
    float weight_decay;
};

/* ------------------------------------------------------------------------------------------------
 * The gradient norm, fixed order only.
 *   g           fp32 [n], 16-byte aligned.  n == 0 returns CLIBD_OK and leaves the record as it is.
 *   grad_scale  what the update multiplies the gradient by (1 / world_size after a SUM all-reduce).
 *   max_norm    > 0 (inf allowed): clip to this norm;  0: no clipping (coef = 1);  negative or NaN: CLIBD_EINVAL.
 *   record      struct clibd_grad_record in device memory.
 *   workspace   clibd_grad_norm_workspace_bytes(n) bytes, 16-byte aligned: one fp32 partial per chunk.  NULL, NULL with a size, a short or
 *               a misaligned workspace is CLIBD_EINVAL.
 * Pass 1: workgroup c owns the floats [c * CHUNK, (c + 1) * CHUNK) whatever the device: thread t adds g^2 of its float4 number
 * k * 256 + t of the chunk for k = 0 .. 15 (fma, x y z w in turn) in fp32; the 64 lanes of a wave are added pairwise (neighbours first),
 * the four wave totals in order; one partial per chunk.  Pass 2: ONE workgroup; thread j adds the partials j, j + 256, ... in fp64, an
 * LDS tree (stride 128, 64, ... 1) adds the 256 sums, thread 0 writes the record: total_norm = (float)(grad_scale * sqrt(sum)) .
 */
size_t clibd_grad_norm_workspace_bytes(size_t n);
int clibd_grad_norm(const float* g, size_t n, float grad_scale, float max_norm, int skip_nonfinite, void* record, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The grouped, clipped update: clibd_adamw_step / clibd_adam_l2_step operation for operation, with
 *   - lr and weight_decay of element i taken from the group that holds i.  `groups` is a HOST array of n_groups entries
 *     (1 .. CLIBD_OPTIM_MAX_GROUPS), read before the call returns and passed to the kernel by value: groups[0].first == 0, the firsts
 *     strictly ascending, multiples of CLIBD_OPTIM_GROUP_ALIGN and (n > 0) below n;
 *   - the gradient g[i] * (grad_scale * coef), coef read from `record` (the product of the two scalars is taken first, in fp32: with
 *     coef == 1 the factor IS grad_scale, and one group then gives clibd_adamw_step's bits).  record == NULL: coef = 1, no skip;
 *   - when record->skip_now is set the launch writes nothing: p, m and v keep their bits.
 * beta1, beta2, eps and step (>= 1) are shared by all groups; the bias corrections are computed on the host (powf) as in the plain entries.
 *   p, g, m, v  fp32 [n], 16-byte aligned (float4 accesses).  n == 0 returns CLIBD_OK.
 */
int clibd_adamw_step_groups(float* p, const float* g, float* m, float* v, size_t n, const struct clibd_optim_group* groups, int n_groups,
                            float beta1, float beta2, float eps, int step, float grad_scale, const void* record, void* stream);
int clibd_adam_l2_step_groups(float* p, const float* g, float* m, float* v, size_t n, const struct clibd_optim_group* groups, int n_groups,
                              float beta1, float beta2, float eps, int step, float grad_scale, const void* record, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_OPTIM_H */
