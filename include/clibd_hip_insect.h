/*
 * clibd_hip_insect.h — the INSECT / BZSL workflow's two kernels of libclibd_hip.so (gfx950): the per-class mean of embedding rows (the
 * "class prototypes" of the reference's scripts/BZSL/extract_feature_for_insect_dataset.py and
 * supervised_fine_tune_bioscan_clip_model_on_insect.py) and the top-k of the logits themselves (torch.argsort(output, dim=1,
 * descending=True)[:, :k] of bioscanclip/epoch/fine_tuning_epoch.py).
 *
 * A seventh header beside clibd_hip.h, clibd_hip_simclr.h, clibd_hip_views.h, clibd_hip_classifier.h, clibd_hip_analysis.h and
 * clibd_hip_rollout.h: the same library, the same conventions (extern "C", caller-owned device buffers and workspaces, `void* stream`,
 * 0 / negative CLIBD_E* status, clibd_last_error for the message, nothing allocates or synchronises, arguments validated on the host
 * before any launch).  The addition is purely additive — no entry of the other six headers changes — so the ABI version stays 7.  The
 * Python binding keeps these symbols under this header's name in clibd_amd._lib.HEADERS.
 *
 * No float atomics: every output has one summation order, so two runs agree bit for bit and the result does not depend on the launch
 * shape.
 */
#ifndef CLIBD_HIP_INSECT_H
#define CLIBD_HIP_INSECT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The class means in numpy's order.  For class c with rows i1 < i2 < ... < in (labels[i] == c):
 *     mean[c, :] = fp32( fp32( ... fp32(x[i1, :] + x[i2, :]) ... + x[in, :]) / fp32(n) )
 * a plain fp32 add per row in ascending row order (no fma, no pairwise tree) and one correctly rounded fp32 divide: bit for bit what
 * `np.sum(list_of_float32_rows, axis=0) / len(list_of_float32_rows)` gives.
 *   x       fp32 [N, ld_x], ld_x >= D, 4-byte aligned; 16-byte loads are used when D % 4 == 0, ld_x % 4 == 0 and x is 16-byte aligned
 *   labels  int32 [N]; a label outside [0, C) is skipped and ORs bit 0 into *error (the caller zeroes the word when it wants a fresh
 *           report, as with clibd_ce_rows_fwd)
 *   mean    transposed == 0: fp32 [C, ld_mean], ld_mean >= D;  transposed == 1: fp32 [D, ld_mean], ld_mean >= C (the layout of the CSV
 *           table).  Padding columns are not written.  A class without rows gives a zero row.
 *   count   int32 [C]: the rows of each class (overwritten).  n is exact in fp32 below 2^24 rows per class: the caller checks `count`.
 *   N >= 1, D >= 1, 1 <= C <= 65536, N * D < 2^31.
 * The per-class row lists are built once: an integer histogram, an exclusive scan, a fill by integer atomics, and a sort of each class's
 * list back into ascending row order; then one thread per (class, column) walks its chain.
 * workspace: clibd_class_mean_workspace_bytes(N, C) bytes (0 for shapes out of range), 16-byte aligned.
 */
size_t clibd_class_mean_workspace_bytes(int N, int C);
int clibd_class_mean_f32(const float* x, int ld_x, const int32_t* labels, int N, int C, int D, float* mean, int ld_mean, int transposed,
                         int32_t* count, int32_t* error, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The k largest logits of every row and their class indices: val[B, k] fp32 (the logits themselves), idx[B, k] int64, the larger value
 * first, equal values by ascending index — torch.sort(logits, dim=1, descending=True, stable=True) cut to k columns.  -inf is a value
 * like any other; NaN is not supported.  logits fp32 [B, ld], ld >= C, 4-byte aligned; 1 <= k <= 8 and k <= C; C below 2^24.
 * One wave per row, registers only (the selection of clibd_softmax_topk without the softmax: confidences that underflow to equal
 * values cannot reorder what the logits distinguish).
 */
int clibd_logits_topk(const float* logits, int ld, int B, int C, int k, float* val, int64_t* idx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_INSECT_H */
