/*
 * clibd_hip_attn_wide.h — multi-head attention for 128- and 192-wide heads in libclibd_hip.so (gfx950): the newer BarcodeBERT towers
 * (hidden 768 with 6 or 4 heads).  clibd_attention_fwd / _bwd of clibd_hip.h stay specialised for 64-wide heads and are untouched.
 *
 * A ninth header beside clibd_hip.h and the other additive ones: the same library, the same conventions (extern "C", caller-owned device
 * buffers, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message, nothing allocates or synchronises, arguments
 * validated on the host before any launch).  The addition is purely additive — no entry of the other headers changes — so the ABI
 * version stays 7.  The Python binding keeps these symbols under this header's name in clibd_amd._lib.HEADERS.
 *
 * No atomics: the workgroup that owns a (sequence, head) writes its own columns, so two runs agree bit for bit.
 */
#ifndef CLIBD_HIP_ATTN_WIDE_H
#define CLIBD_HIP_ATTN_WIDE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Operands (both entries):
 *   qkv    bf16 [B * S, 3 H], H = nheads * head_dim, 16-byte aligned: head h holds its q, k and v at columns h * head_dim,
 *          H + h * head_dim and 2 H + h * head_dim.
 *   head_dim 128 or 192;  1 <= S <= 256 at 128, 1 <= S <= 192 at 192 (two [S rounded up to 32, head_dim] bf16 images must fit the
 *          160-KiB LDS of a compute unit);  B * nheads workgroups.
 *   No key mask, no query prefix, no e4m3 output: the 64-wide entries have those forms, these do not.
 *   Dropout on the probabilities: keep iff hash bits >= drop_thr16 (0 = off, at most 65535), kept values times drop_scale, element
 *   index (((b * nheads + h) * S + q) << 8) | key as in clibd_attention_fwd; with dropout on, B * nheads * S * 256 must stay below 2^32.
 *
 * Forward: out = (softmax(q k^T / sqrt(head_dim)) o F) v, bf16 [B * S, H], 16-byte aligned.
 *   lse (optional, may be NULL): fp32 [B * nheads, S], 4-byte aligned: per (head, query) c2 * max + log2(sum exp2(c2 s - c2 max)) of the
 *   un-dropped scores with c2 = log2(e) / sqrt(head_dim) — the log2 domain clibd_attention_fwd writes.  The backward needs it.
 */
int clibd_attention_wide_fwd(const void* qkv, int B, int S, int nheads, int head_dim, void* out, float* lse /* may be NULL */,
                             uint32_t drop_seed, int drop_thr16, float drop_scale, void* stream);

/* Backward: dqkv bf16 [B * S, 3 H] (16-byte aligned), every row and all three sections, from qkv, dout (bf16 [B * S, H], 16-byte
 * aligned) and the forward's lse (required).  The same dropout arguments as the forward reproduce its mask. */
int clibd_attention_wide_bwd(const void* qkv, const void* dout, const float* lse, int B, int S, int nheads, int head_dim, void* dqkv,
                             uint32_t drop_seed, int drop_thr16, float drop_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_ATTN_WIDE_H */
