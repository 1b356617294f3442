// The LDS "head image" of the attention kernels and what reads and writes it, shared by attention.hip (64-wide heads), attention_wide.hip
// (128 / 192) and rollout.hip (64, K only).  lora.hip keeps a private copy of the 64-wide layout (lwm_tile_off / lwm_tr_frag, the s = 0 case).
//
// Orientation ("key on the MFMA row, query on the lane"): S^T = K.Q^T via v_mfma_f32_16x16x32_bf16(A = K rows, B = Q rows) leaves each lane
// ONE query (lane & 15) and keys 16 kt + 4 (lane >> 4) + reg.  Packed to bf16 (pack_frag) those accumulators are directly the B operand of the
// next product that contracts over keys (P.V, dS.K) with the k-slot -> key map
//      kappa(g, j) = 32 s + 16 (j >> 2) + 4 g + (j & 3)        (g = lane >> 4, j = 0 .. 7)
// and the other operand (V^T / K^T rows = head dim) is fetched with ds_read_b64_tr_b16 using the same map (img_tr_frag).
//
// The image: [S_pad][DH] bf16, rows of 2 DH bytes, filled by 16-byte LDS-DMA with the swizzle on the per-lane SOURCE address.  Chunk ch (16 B)
// of row r sits at chunk ch ^ x(r):
//   128-B rows (DH = 64): x = r & 7.  Two rows share a 256-B bank row; eight consecutive rows put one chunk on eight different 16-B slots.
//   256-B rows (DH = 128): x = (r & 7) << 1.  A row starts on bank 0, so the 16-B slot of the 256-B bank row is ch ^ x.  The transposed read of a
//     32-lane half takes rows 8 n .. 8 n + 7 at one chunk pair: x >> 1 = r & 7 puts them on eight different 32-B slot pairs.  The ds_read_b128 row
//     read works in 16-lane groups of rows {0-3, 12-15} at chunk c and {4-11} at chunk c ^ 1 (or the reverse): even x, so the two sets take the
//     even and the odd slots, and within a set r & 7 differs.  Both conflict-free.
//   384-B rows (DH = 192): x = r & 6 (only the low three chunk bits move, so a chunk stays inside its aligned group of 8 of the 24).  Row r starts
//     half a bank row further when r is odd: slot = (8 (r & 1) + (ch ^ x)) mod 16.  (r & 1, x) differs over 8 consecutive rows -> eight slot pairs
//     for the transposed read; for the row read's two sets the parity of ch ^ x separates them and (r & 1, r & 6) differs within each.
// Rows S .. S_pad-1 of an image are copies of row S-1 (finite bytes); their scores are masked to NEG_BIG, output rows >= S are never written.
#pragma once
#include "common.h"
#include "host_util.h"

namespace clibd {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// A masked or padding score.  A power of two: NEG_BIG * c2 is then exact in fp32, so a row whose keys are ALL masked has
// fma(NEG_BIG, c2, -(NEG_BIG * c2)) = 0 and every probability exp2(0) = 1 (uniform weight, finite results).  With -1.0e30f the product rounds,
// the fused multiply-add returns the rounding error (8e20), exp2 of it is +inf and the row leaves as NaN.  For every other row nothing changes:
// a masked score's exponent argument stays finite and its exp2 underflows to exactly 0.
constexpr float NEG_BIG = -0x1p100f;

template <int DH>
__device__ __forceinline__ int img_swz(int row) {
    static_assert(DH == 64 || DH == 128 || DH == 192, "head width");
    return DH == 64 ? (row & 7) : DH == 128 ? ((row & 7) << 1) : (row & 6);
}
// byte offset of 16-byte chunk `ch` of row `row`
template <int DH>
__device__ __forceinline__ int img_off(int row, int ch) { return row * (2 * DH) + ((ch ^ img_swz<DH>(row)) << 4); }

// Stage rows [0, S_pad) x DH bf16 of one head (global row stride `ld` elements) into an LDS image; every LDS-DMA piece is 64 consecutive
// 16-B chunks, piece p goes to wave p mod nwaves.  Every source row index is clamped to S - 1, every destination lies in [0, S_pad * 2 DH).
template <int DH>
__device__ __forceinline__ void img_stage(char* img, const unsigned short* gbase, size_t ld, int S, int S_pad, int wave, int lane, int nwaves) {
    constexpr int CH = DH / 8;               // chunks per row
    const int npieces = (S_pad * CH) >> 6;   // S_pad % 32 == 0 (or 16 at DH = 64): whole pieces
    if constexpr (64 % (8 * CH) == 0) {
        // a piece covers whole rows and whole swizzle periods (DH = 64): the lane's row within the piece and its swizzled chunk do not depend on p
        const int prow = lane / CH;
        const int chunk = (lane % CH) ^ img_swz<DH>(prow);
        for (int p = wave; p < npieces; p += nwaves) {
            const int row = min(p * (64 / CH) + prow, S - 1);
            glds16(gbase + (size_t)row * ld + chunk * 8, img + p * 1024);
        }
    } else {
        for (int p = wave; p < npieces; p += nwaves) {
            const int L = p * 64 + lane;
            const int row = L / CH, pos = L - row * CH;
            glds16(gbase + (size_t)min(row, S - 1) * ld + ((pos ^ img_swz<DH>(row)) << 3), img + p * 1024);
        }
    }
}

// row fragment (ds_read_b128): elements 32 ks + 8 g .. + 7 of row `row`
template <int DH>
__device__ __forceinline__ bf16x8 img_row_frag(const char* img, int row, int ks, int g) {
    return *(const bf16x8*)(img + img_off<DH>(row, 4 * ks + g));
}

// transposed fragment: rows d = 16 dt + (lane & 15) of the image's transpose, k-slots (g, j) -> image rows kappa(g, j)
template <int DH>
__device__ __forceinline__ bf16x8 img_tr_frag(const char* img, int s, int dt, int lane) {
    const int g = lane >> 4, i = lane & 15;
    const int q = i >> 2, p = i & 3;
    const int r0 = 32 * s + 4 * g + q;
    const int ch = 2 * dt + (p >> 1);
    const int a0 = img_off<DH>(r0, ch) + 8 * (p & 1);
    const int a1 = img_off<DH>(r0 + 16, ch) + 8 * (p & 1);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + a0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + a1));
    return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// two accumulator quads (key tiles 2 s, 2 s + 1) -> the bf16 B operand of k-slot s
__device__ __forceinline__ bf16x8 pack_frag(const f32x4& a, const f32x4& b) {
    bf16x8 r;
    r[0] = (short)f2bf(a[0]); r[1] = (short)f2bf(a[1]); r[2] = (short)f2bf(a[2]); r[3] = (short)f2bf(a[3]);
    r[4] = (short)f2bf(b[0]); r[5] = (short)f2bf(b[1]); r[6] = (short)f2bf(b[2]); r[7] = (short)f2bf(b[3]);
    return r;
}

// One 16-row x 16 DT-column output tile of a wave: lane (i = lane & 15, g = lane >> 4) holds v[dt][r] = element (row i, column
// 16 dt + 4 g + r) — 8 bytes per (lane, dt).  Written that way (DT dwordx2 per lane) a store instruction covers 32-byte pieces and the output
// tail of the attention kernels is store-issue bound.  A v_permlane16_swap between the lane rows g and g ^ 1 (a 2 x 2 transpose of the
// (dt, dt + 1) chunks) leaves every lane 16 contiguous bytes, and each dwordx4 store of a tile pair then covers 64 contiguous bytes of all 16
// rows.  Every lane must call this (the swap is a full-wave operation); `on` guards the stores only (it is a function of the row, identical in
// the lanes that exchange).  Values, and so results, are unchanged.
__device__ __forceinline__ void permlane16_swap_u32(unsigned& a, unsigned& b) {   // common.h's swap on packed bf16 pairs
    float fa = __uint_as_float(a), fb = __uint_as_float(b);
    permlane16_swap(fa, fb);
    a = __float_as_uint(fa);
    b = __float_as_uint(fb);
}
template <int DT>
__device__ __forceinline__ void store_rows(unsigned short* row, const f32x4 (&v)[DT], float mul, bool on, int g) {
#pragma unroll
    for (int pr = 0; pr < DT / 2; ++pr) {
        unsigned a0 = pack2bf(v[2 * pr][0] * mul, v[2 * pr][1] * mul), a1 = pack2bf(v[2 * pr][2] * mul, v[2 * pr][3] * mul);
        unsigned b0 = pack2bf(v[2 * pr + 1][0] * mul, v[2 * pr + 1][1] * mul), b1 = pack2bf(v[2 * pr + 1][2] * mul, v[2 * pr + 1][3] * mul);
        permlane16_swap_u32(a0, b0);   // even g: (a, b) = columns 4g .. 4g+7 of tile dt = 2 pr;  odd g: columns 4(g-1) .. 4(g-1)+7 of dt = 2 pr + 1
        permlane16_swap_u32(a1, b1);
        if (on) *(uint4*)(row + 16 * (2 * pr + (g & 1)) + 8 * (g >> 1)) = make_uint4(a0, a1, b0, b1);
    }
}
// the (dt, dt + 1) = (2 pr, 2 pr + 1) pair of store_rows, for a wave that holds only those two column tiles.  The same body, kept apart:
// routed through one another the two forms change the register allocation of nearly every kernel that stores.
__device__ __forceinline__ void store_rows_pair(unsigned short* row, const f32x4& va, const f32x4& vb, float mul, bool on, int g, int pr) {
    unsigned a0 = pack2bf(va[0] * mul, va[1] * mul), a1 = pack2bf(va[2] * mul, va[3] * mul);
    unsigned b0 = pack2bf(vb[0] * mul, vb[1] * mul), b1 = pack2bf(vb[2] * mul, vb[3] * mul);
    permlane16_swap_u32(a0, b0);
    permlane16_swap_u32(a1, b1);
    if (on) *(uint4*)(row + 16 * (2 * pr + (g & 1)) + 8 * (g >> 1)) = make_uint4(a0, a1, b0, b1);
}

// Host: the dropout arguments of every attention entry.  The counter of a score is ((b * nheads + h) * S + q) * 256 + key in 32 bits.
inline int check_dropout_args(const char* op, int B, int S, int nheads, int drop_thr16) {
    if (drop_thr16 < 0 || drop_thr16 > 65535) return fail(op, "bad dropout threshold");
    if (drop_thr16 > 0 && (unsigned long long)B * nheads * S * 256ull >= (1ull << 32)) return fail(op, "dropout index overflow");
    return 0;
}

}  // namespace clibd
