/*
 * clibd_hip_mlm.h — masked-k-mer pre-training of the BarcodeBERT DNA tower in libclibd_hip.so (gfx950): the position sampler, the step
 * from "all token rows" to "the masked rows" and back, and the cross-entropy over the k-mer vocabulary on the bf16 logits the decoder
 * GEMM writes.  The objective is HF `BertForMaskedLM(input_ids, labels)` with labels = -100 outside the masked positions.
 *
 * A tenth header beside clibd_hip.h and the eight additive ones: the same library, the same conventions (extern "C", caller-owned device
 * buffers, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message prefixed by the entry's name, nothing allocates
 * or synchronises, arguments validated on the host before any launch).  The addition is purely additive — no entry of the other headers
 * changes its signature or its arithmetic — so the ABI version stays 7.  The Python binding keeps these symbols under this
 * header's name in clibd_amd._lib.HEADERS.
 *
 * No float atomics: every sum has one order, the two counters are integers, so two runs agree bit for bit.
 */
#ifndef CLIBD_HIP_MLM_H
#define CLIBD_HIP_MLM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIBD_MLM_IGNORE (-100) /* the target of a position that takes no part in the loss (torch's ignore_index) */

/* ------------------------------------------------------------------------------------------------
 * The sampler: n_mask positions of every sequence, chosen by a counter-based hash (a pure function of seed and position).
 *   ids        int64 [B, S], 2 <= S <= 256, B * S < 2^31.  Position 0 (the 0 the sequence pipeline prepends) is never chosen.
 *   key(b, s)  = (ids[b, s] == unk_id, lowbias32((b * S + s) ^ seed), s) for s >= 1 — the hash of the dropout masks, all 32 bits.
 *   The n_mask lexicographically smallest keys of a sequence are chosen, 1 <= n_mask <= S - 1: a padding k-mer (unk_id) ranks after
 *   every real one and is taken only when the real ones run out.
 *   masked     int64 [B, S]: mask_id at the chosen positions (always: no 80/10/10 replacement), ids elsewhere.
 *   rows       int32 [B * n_mask]: the flat index b * S + s of the chosen positions, sequence by sequence, ascending in s.
 *   targets    int64 [B * n_mask]: the original id, or CLIBD_MLM_IGNORE where it was unk_id.
 *   n_valid    int32 [1]: the number of targets that are not CLIBD_MLM_IGNORE.
 * ids, masked and targets are 8-byte aligned, rows and n_valid 4-byte aligned.  One wave per sequence ranks the keys by counting.
 */
int clibd_mlm_mask(const int64_t* ids, int B, int S, uint32_t seed, int n_mask, int64_t mask_id, int64_t unk_id, int64_t* masked,
                   int32_t* rows, int64_t* targets, int32_t* n_valid, void* stream);

/* ------------------------------------------------------------------------------------------------
 * out[i, :] = x[rows[i], :] for i < R.   x bf16 [M, H], out bf16 [R, H], dense, 16-byte aligned; H % 8 == 0; rows int32 [R].
 * An index outside [0, M) reads nothing and gives a zero row.
 */
int clibd_rows_gather_bf16(const void* x, int M, int H, const int32_t* rows, int R, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The transpose of the gather: out[rows[i], :] = src[i, :], and every row of out bf16 [M, H] that is not listed becomes zero — the call
 * writes all of out, so the caller needs no memset, and nothing accumulates.  The rows of one call must be distinct (the sampler's
 * are, by construction); a repeated index is a caller error that is not checked: which source row wins is then undefined.  An index
 * outside [0, M) is dropped.   M * (H / 8) < 2^31.
 */
int clibd_rows_scatter_bf16(const void* src, const int32_t* rows, int R, int M, int H, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cross-entropy of R rows over a vocabulary of V <= 8192 entries, forward and gradient in one call.
 *   logits   bf16 [R, ld], ld >= V, ld % 8 == 0, 16-byte aligned.  Columns V .. ld - 1 (the GEMM's padding) are never read.
 *   targets  int64 [R], each CLIBD_MLM_IGNORE or in [0, V).  Any other value sets bit 0 of *err (uint32, sticky, may be NULL) and the
 *            row is treated as ignored; nothing faults.
 *   n_valid  int32 [1] on the device (clibd_mlm_mask's count); the divisor is n = max(*n_valid, 1).
 *   row_loss fp32 [R] = log(sum_j exp(x_j - max)) + max - x_target, all statistics fp32;  0 for an ignored row.
 *   loss     fp32 [1] = (sum_i row_loss[i]) / n, one workgroup, one fixed order.
 *   correct  int32 [1] = the number of rows that are not ignored and whose argmax (the lowest index on ties) equals their target.
 *   On return logits holds the gradient (exp(x_j - max) / sum - [j == target]) / n as bf16; exactly 0 in an ignored row and in the
 *   columns V .. ld - 1.
 * One wave per row; the row is read three times (max, sum, gradient) and sits in L2 meanwhile.
 */
int clibd_mlm_ce_bf16(void* logits, int ld, const int64_t* targets, int R, int V, const int32_t* n_valid, float* row_loss, float* loss,
                      int32_t* correct, uint32_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_MLM_H */
