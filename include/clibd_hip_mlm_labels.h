/*
 * clibd_hip_mlm_labels.h — masked-LM pre-training with caller-made labels in libclibd_hip.so (gfx950): the step from HF-style
 * `labels [B, S]` (-100 = ignore, any number of labelled positions per sequence) to the `rows` / `targets` the vocabulary head of
 * clibd_hip_mlm.h runs on, and BERT's Bernoulli 80/10/10 sampler that makes such labels.
 *
 * A twelfth header beside clibd_hip.h and the ten additive ones: the same library, the same conventions (extern "C", caller-owned device
 * buffers, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message prefixed by the entry's name, nothing allocates
 * or synchronises, arguments validated on the host before any launch).  The addition is purely additive — no entry of the other headers
 * changes its signature or its arithmetic — so the ABI version stays 7.  The Python binding keeps these symbols under this
 * header's name in clibd_amd._lib.HEADERS.
 *
 * No float arithmetic at all: counts, prefix sums and hashes are integers, every output element has one writer, and the only atomics OR
 * a flag bit, so two runs agree bit for bit.
 *
 * The gather and the scatter of the compacted rows are clibd_rows_gather_bf16 / clibd_rows_scatter_bf16 of clibd_hip_mlm.h unchanged:
 * the padding rows carry the index CLIBD_MLM_PAD_ROW, which those two read as "outside [0, M)": a zero row gathered, nothing scattered.
 */
#ifndef CLIBD_HIP_MLM_LABELS_H
#define CLIBD_HIP_MLM_LABELS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIBD_MLM_PAD_ROW (-1)       /* rows[i] of a padding row: no row of [0, M) */
#define CLIBD_MLM_MAX_SPECIAL 8      /* the most special ids the sampler takes */
#define CLIBD_MLM_COMPACT_MAX_M (1 << 24)

/* ------------------------------------------------------------------------------------------------
 * Label compaction: the labelled positions of `labels`, ascending, at a capacity the host chooses.
 *   labels      int64 [M], 1 <= M <= 2^24: CLIBD_MLM_IGNORE (-100, clibd_hip_mlm.h) or a vocabulary id.  A position is LABELLED iff its
 *               label is not -100.  A labelled value outside [0, V) sets bit 0 of *err (uint32, sticky, may be NULL) — the word and the
 *               bit clibd_mlm_ce_bf16 reports the same condition in — and is passed through; the cross-entropy then ignores that row.
 *   r_cap       the capacity: a multiple of 64, >= 64 (the row granule of the head's GEMMs).
 *   rows        int32 [r_cap]: the flat indices of the first min(n, r_cap) labelled positions in ascending order, then CLIBD_MLM_PAD_ROW.
 *   targets     int64 [r_cap]: their labels, then CLIBD_MLM_IGNORE.
 *   n_labelled  int32 [1] = n, the number of labelled positions of all of `labels` (also when n > r_cap): the divisor of the mean.
 *   overflow    uint32 [1], sticky: bit 0 is set iff n > r_cap, and is never cleared here.  rows / targets then hold the correct prefix;
 *               nothing is written past r_cap.  The caller zeroes the word once and reads it when it may synchronise.
 *   workspace   clibd_mlm_compact_workspace_bytes(M) bytes, 16-byte aligned: one int32 per tile of 256 labels.
 * Three launches: per-tile counts; one workgroup's exclusive scan of the counts (which also writes n and the flag); per-tile ranks by
 * wave ballots, the writes, and the padding.  labels and targets are 8-byte aligned, the int32 / uint32 arrays 4-byte aligned.
 */
size_t clibd_mlm_compact_workspace_bytes(int M);
int clibd_mlm_compact_labels(const int64_t* labels, int M, int V, int r_cap, int32_t* rows, int64_t* targets, int32_t* n_labelled,
                             uint32_t* overflow, uint32_t* err, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BERT's sampler: every eligible position is chosen independently with probability p_choose, and a chosen position becomes mask_id
 * (p_mask), a uniformly drawn non-special id (p_random) or stays as it is (the rest).  Integer-only, one element per thread, a pure
 * function of (seed, flat index): the result does not depend on the launch shape.
 *   ids         int64 [B, S], S >= 1, B * S < 2^31.
 *   attn_mask   int32 [B, S] or NULL: zero = a padded position, never chosen.
 *   special     HOST array of n_special ids, 0 <= n_special <= CLIBD_MLM_MAX_SPECIAL, read before the call returns: a position whose id
 *               is one of them is never chosen.  Position 0 of every sequence is never chosen either.
 *   V           the vocabulary size, V > n_special: a random replacement is drawn from [n_special, V) (the specials are taken to be the
 *               first n_special ids of the vocabulary, as <MASK>, <CLS>, <UNK> are).
 *   The rule, with i = b * S + s, lowbias32 the hash of the dropout masks, T(p) = floor(p * 2^32 + 0.5) as a 64-bit integer:
 *     u0 = lowbias32(i ^ seed);  u1 = lowbias32(u0 + 0x9E3779B9);  u2 = lowbias32(u0 + 2 * 0x9E3779B9)   (mod 2^32)
 *     chosen  iff eligible and u0 < T(p_choose)
 *     masked  = mask_id                               if u1 < T(p_mask)
 *             = n_special + ((u2 * (V - n_special)) >> 32)   else if u1 < T(p_mask) + T(p_random)   (64-bit product and sum)
 *             = ids                                   otherwise
 *     labels  = ids where chosen, CLIBD_MLM_IGNORE elsewhere;  masked = ids where not chosen.
 *   p_choose, p_mask, p_random in [0, 1], p_mask + p_random <= 1 (+ 1e-9).
 *   masked, labels   int64 [B, S].  ids, masked and labels are 8-byte aligned, attn_mask 4-byte aligned.
 */
int clibd_mlm_mask_bert(const int64_t* ids, const int32_t* attn_mask, int B, int S, int V, uint32_t seed, double p_choose, double p_mask,
                        double p_random, int64_t mask_id, const int64_t* special, int n_special, int64_t* masked, int64_t* labels,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_MLM_LABELS_H */
