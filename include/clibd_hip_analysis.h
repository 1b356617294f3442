/*
 * clibd_hip_analysis.h — the embedding analysis of libclibd_hip.so (gfx950): the arithmetic behind the reference's result scripts
 * (scripts/result/distribution_of_similarities.py, scripts/result/create_confusion_matrix.py, and calculate_silhouette_score of
 * scripts/inference_and_eval.py): silhouette samples per labelling, the distance from a query to the nearest key of its own class, and
 * confusion-matrix counts.  No figure is drawn here or anywhere in the project.
 *
 * A fifth header beside clibd_hip.h, clibd_hip_simclr.h, clibd_hip_views.h and clibd_hip_classifier.h: the same library, the same
 * conventions (extern "C", caller-owned device buffers and workspaces, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for
 * the message, nothing allocates or synchronises, arguments validated on the host before any launch).  The addition is purely additive —
 * no entry of the other four headers changes its signature or its arithmetic — so the ABI version stays 7.  The Python binding keeps
 * these symbols under this header's name in clibd_amd._lib.HEADERS.
 *
 * Run offsets (`seg`) are given twice: a device copy that the kernels read and a host copy (`seg_host`, the same C + 1 values) that the
 * entry validates before it launches anything.  No float atomics: every sum has one fixed order, so results repeat bit for bit.
 */
#ifndef CLIBD_HIP_ANALYSIS_H
#define CLIBD_HIP_ANALYSIS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * sklearn.metrics.silhouette_samples(X, labels, metric="euclidean") for one labelling (reference: calculate_silhouette_score,
 * distribution_of_similarities.py:34-38, the same function in inference_and_eval.py and check_failure_cases.py).
 *   X fp32 [N, D] dense, 16-byte aligned, rows ordered so that cluster c is the run seg[c] .. seg[c + 1]; D % 32 == 0 (zero padded columns
 *   change no distance); seg int32 [C + 1] rising strictly from 0 to N; 2 <= C <= N - 1 (sklearn's condition), N <= 2^24.
 *   s fp32 [N] in the order of X's rows:
 *     d(i, j) = sqrt(max(|x_i|^2 + |x_j|^2 - 2 x_i.x_j, 0)), d(i, i) = 0;  a(i) = sum_{j in own} d(i, j) / (n_own - 1);
 *     b(i) = min over the other clusters of the mean of d(i, .) over the cluster;  s = (b - a) / max(a, b);  s = 0 in a singleton cluster
 *     (and where max(a, b) = 0).
 * The Gram product runs on the f32-input MFMA (exact fp32 operands, an fp32 fma chain over k) and the norms are the same chain, so
 * identical rows are at distance exactly 0.  A workgroup owns one (128-row tile, column chunk) pair; neither the N x N distances nor N x C
 * cluster sums are stored.  col_chunk: columns per chunk, a multiple of 64, 0 = the default (1024).
 * workspace: clibd_silhouette_workspace_bytes(N, col_chunk) bytes (0 for invalid arguments), 16-byte aligned:
 *   8 N + 16 N ceil(N / col_chunk) bytes and alignment.
 */
size_t clibd_silhouette_workspace_bytes(int N, int col_chunk);
int clibd_silhouette_samples(const float* X, int N, int D, const int32_t* seg, const int32_t* seg_host, int C, int col_chunk, float* s,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The distance from each query to the nearest key of its own class (reference: get_similarity_for_different_combination_of_modalities,
 * distribution_of_similarities.py:93-104, the inner loops of np.linalg.norm(query_feature - key_feature)).
 *   Q fp32 [Nq, ldq], K fp32 [Nk, ldk] (ld >= D), keys grouped by class: class c is the run seg[c] .. seg[c + 1], seg int32 [C + 1] rising
 *   from 0 to Nk (empty classes allowed); qclass int32 [Nq] in [0, C) or -1.
 *   dist fp32 [Nq] = min_j sqrt(sum_t (q_t - k_jt)^2), the sum in fp32 in the difference form; arg int32 [Nq] the key row, the lowest on
 *   a tie.  An empty class, or a qclass outside [0, C), gives +inf and -1.  One wave per query.
 */
int clibd_same_label_nearest(const float* Q, int ldq, const float* K, int ldk, int Nq, int Nk, int D, const int32_t* seg,
                             const int32_t* seg_host, int C, const int32_t* qclass, float* dist, int32_t* arg, void* stream);

/* ------------------------------------------------------------------------------------------------
 * sklearn.metrics.confusion_matrix(y_true, y_pred, labels=...) as counts (reference: create_confusion_matrix.py:61, 75).
 *   true_code, pred_code int32 [N]: class codes in [0, C), or -1 for a label outside `labels` (such a sample is skipped, as sklearn does);
 *   counts int32 [C, C], rows = true; the entry zeroes it.  Integer atomics: the result does not depend on the order.  C <= 46340.
 */
int clibd_confusion_counts(const int32_t* true_code, const int32_t* pred_code, size_t N, int C, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_ANALYSIS_H */
