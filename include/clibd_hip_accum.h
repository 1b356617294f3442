/*
 * clibd_hip_accum.h — gradient accumulation's device side in libclibd_hip.so (gfx950): the gradient norm of clibd_hip_optim.h with a
 * divisor read from device memory, so that k micro-batches on W ranks, summed into one flat bucket, are applied as ONE batch of k W times
 * the size whose count of labelled positions the host never sees.
 *
 * A fourteenth header beside clibd_hip.h and the twelve additive ones: the same library, the same conventions (extern "C", caller-owned
 * device buffers, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message prefixed by the entry's name, nothing
 * allocates or synchronises, arguments validated on the host before any launch).  The addition is purely additive — clibd_grad_norm and
 * the grouped updates keep their signatures and their arithmetic — so the ABI version stays 7.  The Python binding keeps these symbols under this
 * header's name in clibd_amd._lib.HEADERS.
 *
 * There is no float atomic anywhere here: two runs on any box agree bit for bit.
 *
 * Not here: an update kernel (clibd_adamw_step_groups / clibd_adam_l2_step_groups of clibd_hip_optim.h read the record this entry
 * writes), accumulation of a contrastive loss, a device-side step counter.
 */
#ifndef CLIBD_HIP_ACCUM_H
#define CLIBD_HIP_ACCUM_H
#include <stddef.h>
#include <stdint.h>

#include "clibd_hip_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The gradient norm with a device divisor: clibd_grad_norm (same chunking CLIBD_GRAD_NORM_CHUNK, same pass 1 from the same source, same
 * fp64 fixed-order pass 2), then with d = max(*divisor, 1) in fp32 — the rule clibd_mlm_ce_bf16 applies to its n_valid; 0, a negative
 * value and NaN give 1 — it writes into the same struct clibd_grad_record:
 *   total_norm     (float)(grad_scale * sqrt(sum g[i]^2) / d), the product and the quotient in fp64: the norm of the averaged gradient;
 *   coef           clip(total_norm) / d in fp32, clip as in clibd_grad_norm (1 when max_norm == 0).  The grouped updates multiply the
 *                  gradient by grad_scale * coef: the average and the clip in one factor;
 *   skip_now, skipped_total   decided on total_norm as in clibd_grad_norm.
 *   divisor        fp32 [1] in device memory, 4-byte aligned, or NULL (d = 1).  With NULL or *divisor == 1 the record equals
 *                  clibd_grad_norm's bit for bit.  A count travels as fp32: exact up to 2^24.
 * Every other argument, the workspace rule (clibd_grad_norm_div_workspace_bytes(n) bytes, equal to clibd_grad_norm_workspace_bytes(n))
 * and every refusal are clibd_grad_norm's.  n == 0 returns CLIBD_OK and leaves the record as it is.
 */
size_t clibd_grad_norm_div_workspace_bytes(size_t n);
int clibd_grad_norm_div(const float* g, size_t n, float grad_scale, float max_norm, int skip_nonfinite, const float* divisor, void* record,
                        void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_ACCUM_H */
