// Multi-head attention forward / backward for 128- and 192-wide heads (the newer BarcodeBERT towers: hidden 768 with 6 or 4 heads) on gfx950.
// Beside attention.hip, which stays specialised for 64-wide heads: no key mask, no query prefix, no e4m3 output here.  The LDS image (256- and
// 384-byte rows, their swizzles and the bank-conflict argument), its staging, the fragment reads, the orientation and the row store are
// attn_image.h's, shared with attention.hip and rollout.hip.
//
// One workgroup per (sequence, head): 4 waves, one per SIMD, in the backward and the short forward; 8 waves in the forward at S > 64.  Two [S_pad][DH] bf16 images of that head live in LDS: K and V in the forward and in
// the backward's dQ phase, Q and dO in its dK / dV phase.  That is the rule behind the sequence limits: 2 x 256 x 256 B = 128 KiB at DH = 128,
// 2 x 192 x 384 B = 144 KiB at DH = 192 (plus the row statistics), and 2 x 224 x 384 B would pass the 160 KiB of a compute unit.
// The scores of one 16-query tile against ALL keys stay in registers (<= 16 key tiles x 4 fp32), so the softmax is an exact full-row softmax.
// Key columns >= S get probability exactly 0, output rows >= S are never written.
#include "attn_image.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_attn_wide.h"
#include <stdlib.h>

namespace clibd {
namespace wide {

constexpr int WAVES = 4;

// scale factors of the four keys 16 kt + 4 g .. + 3 of query row `qrow` (= (b * nheads + h) * S + q)
__device__ __forceinline__ void drop_quad(unsigned seed, unsigned qrow, int kt, int g, unsigned thr16, float scale, float (&f)[4]) {
    const unsigned base = (qrow << 8) + 16u * (unsigned)kt + 4u * (unsigned)g;
    drop_pair(seed, base, thr16, scale, f[0], f[1]);
    drop_pair(seed, base + 2, thr16, scale, f[2], f[3]);
}

// ============================================ forward ==========================================================
// NKT: number of 16-key tiles, even (S_pad = 16 NKT, a multiple of 32).  DROP: dropout on the probabilities, compile-time (its hash is ~7 VALU per score).
// NW: waves per workgroup (fwd_waves below); wave w takes query tiles w, w + NW, ...
template <int DH, int NKT, bool DROP, int NW>
__global__ __launch_bounds__(64 * NW) void attention_wide_fwd_kernel(const unsigned short* __restrict__ qkv, int S, int nheads,
                                                                        unsigned short* __restrict__ out, float scale, unsigned drop_seed,
                                                                        int drop_thr16, float drop_scale, float* __restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int S_pad = 16 * NKT, KS = DH / 32, DT = DH / 16;
    char* k_img = smem;
    char* v_img = smem + S_pad * 2 * DH;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x / nheads, h = blockIdx.x % nheads;
    const int H = nheads * DH;
    const size_t ld = (size_t)3 * H;
    const unsigned short* qbase = qkv + (size_t)b * S * ld + h * DH;
    const int g = lane >> 4, i = lane & 15;
    const int nqt = (S + 15) >> 4;
    const float c2 = scale * 1.4426950408889634f;   // p = exp2(c2 s - c2 max): one FMA + one v_exp per score
    const bool last_live = S > 16 * (NKT - 1);      // NKT is even: the last key tile can be all padding (S = 133 -> 9 live tiles of 10)
    img_stage<DH>(k_img, qbase + H, ld, S, S_pad, wave, lane, NW);
    img_stage<DH>(v_img, qbase + 2 * H, ld, S, S_pad, wave, lane, NW);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int qt = wave; qt < nqt; qt += NW) {
        const int q = qt * 16 + i;
        const int qc = min(q, S - 1);
        bf16x8 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const bf16x8*)(qbase + (size_t)qc * ld + 32 * ks + 8 * g);
        f32x4 sc[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            sc[kt] = (f32x4){0, 0, 0, 0};
            if (kt == NKT - 1 && !last_live) continue;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_row_frag<DH>(k_img, kt * 16 + i, ks, g), qf[ks], sc[kt], 0, 0, 0);
        }
        float mx = NEG_BIG;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt == NKT - 1 && !last_live) continue;
            if (kt >= NKT - 2 && kt * 16 + 15 >= S) {   // S > 16 (NKT - 2): only the last two tiles can hold padding keys
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt * 16 + 4 * g + r >= S) sc[kt][r] = NEG_BIG;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[kt][r]);
        }
        mx = rows4_max(mx);
        const float mc = mx * c2;
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt == NKT - 1 && !last_live) continue;   // sc stays exactly 0: the probabilities of an all-padding tile
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(fmaf(sc[kt][r], c2, -mc));   // padding scores underflow to exactly 0
                sc[kt][r] = e;
                sum += e;
            }
        }
        sum = rows4_sum(sum);
        const float inv = 1.0f / sum;
        if (lse != nullptr && g == 0 && q < S) lse[(size_t)blockIdx.x * S + q] = mc + __builtin_amdgcn_logf(sum);
        f32x4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NKT / 2; ++s) {
            if (DROP) {
                const unsigned qrow = (unsigned)blockIdx.x * (unsigned)S + (unsigned)q;
                float f[4];
                drop_quad(drop_seed, qrow, 2 * s, g, (unsigned)drop_thr16, drop_scale, f);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[2 * s][r] *= f[r];
                drop_quad(drop_seed, qrow, 2 * s + 1, g, (unsigned)drop_thr16, drop_scale, f);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[2 * s + 1][r] *= f[r];
            }
            const bf16x8 pf = pack_frag(sc[2 * s], sc[2 * s + 1]);   // un-normalised probabilities (<= 1/(1-p)); 1/sum is applied to O
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_tr_frag<DH>(v_img, s, dt, lane), pf, o[dt], 0, 0, 0);
        }
        store_rows<DT>(out + ((size_t)b * S + qc) * H + h * DH, o, inv, q < S, g);
    }
}

// ============================================ backward =========================================================
// Two phases over the forward's log-sum-exp (P = exp2(c2 s - lse) is the normalised probability with one FMA and one v_exp):
//   phase 1, K and V resident, per 16-query tile:  dP = (dO V^T) o F,  delta = sum_k P dP,  dS / scale = P (dP - delta) -> bf16,  dQ = scale (dS / scale) K
//   phase 2, Q and dO resident, per 16-key tile:   the same P, dP and dS / scale from the saved delta,  dV = (P o F)^T dO,  dK = scale (dS / scale)^T Q
// Every output element has one owner and one summation order: no atomics, two runs agree bit for bit.
template <int DH, int NKT, bool DROP>
__global__ __launch_bounds__(64 * WAVES) void attention_wide_bwd_kernel(const unsigned short* __restrict__ qkv,
                                                                        const unsigned short* __restrict__ dout,
                                                                        const float* __restrict__ lse, int S, int nheads,
                                                                        unsigned short* __restrict__ dqkv, float scale, unsigned drop_seed,
                                                                        int drop_thr16, float drop_scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int S_pad = 16 * NKT, KS = DH / 32, DT = DH / 16;
    char* t0 = smem;                       // phase 1: K   | phase 2: Q
    char* t1 = smem + S_pad * 2 * DH;      // phase 1: V   | phase 2: dO
    float* st_m = (float*)(smem + 2 * S_pad * 2 * DH);   // lse per query row; +BIG for rows >= S, i.e. P = 0 exactly
    float* st_d = st_m + S_pad;                          // delta = sum_k P dP
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x / nheads, h = blockIdx.x % nheads;
    const int H = nheads * DH;
    const size_t ld = (size_t)3 * H;
    const unsigned short* qbase = qkv + (size_t)b * S * ld + h * DH;
    const unsigned short* dobase = dout + (size_t)b * S * H + h * DH;
    unsigned short* dqbase = dqkv + (size_t)b * S * ld + h * DH;
    const int g = lane >> 4, i = lane & 15;
    const float c2 = scale * 1.4426950408889634f;
    const int nt = (S + 15) >> 4;                     // live 16-row tiles, queries and keys alike
    const bool last_live = S > 16 * (NKT - 1);

    img_stage<DH>(t0, qbase + H, ld, S, S_pad, wave, lane, WAVES);
    img_stage<DH>(t1, qbase + 2 * H, ld, S, S_pad, wave, lane, WAVES);
    for (int r = threadIdx.x; r < S_pad; r += 64 * WAVES) {
        st_m[r] = r < S ? lse[(size_t)blockIdx.x * S + r] : -NEG_BIG;
        st_d[r] = 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---------------- phase 1: per 16-query tile: dP, delta, dS, dQ ----------------
    for (int qt = wave; qt < nt; qt += WAVES) {
        const int q = qt * 16 + i;
        const int qc = min(q, S - 1);
        bf16x8 qf[KS], dof[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = *(const bf16x8*)(qbase + (size_t)qc * ld + 32 * ks + 8 * g);
            dof[ks] = *(const bf16x8*)(dobase + (size_t)qc * H + 32 * ks + 8 * g);
        }
        const float m = st_m[q];   // q < S_pad always
        f32x4 sc[NKT], dp[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            sc[kt] = (f32x4){0, 0, 0, 0};
            dp[kt] = (f32x4){0, 0, 0, 0};
            if (kt == NKT - 1 && !last_live) continue;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_row_frag<DH>(t0, kt * 16 + i, ks, g), qf[ks], sc[kt], 0, 0, 0);
                dp[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_row_frag<DH>(t1, kt * 16 + i, ks, g), dof[ks], dp[kt], 0, 0, 0);
            }
        }
        float dl = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt == NKT - 1 && !last_live) continue;   // sc, dp stay exactly 0
            float f[4] = {1.f, 1.f, 1.f, 1.f};
            if (DROP) drop_quad(drop_seed, (unsigned)blockIdx.x * (unsigned)S + (unsigned)q, kt, g, (unsigned)drop_thr16, drop_scale, f);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p = __builtin_amdgcn_exp2f(fmaf(sc[kt][r], c2, -m));   // normalised probability
                if (kt >= NKT - 2 && kt * 16 + 4 * g + r >= S) p = 0.f;      // padding keys
                const float d = dp[kt][r] * f[r];                            // O = (P o F) V  =>  dP = (dO V^T) o F
                sc[kt][r] = p;
                dp[kt][r] = d;
                dl += p * d;
            }
        }
        dl = rows4_sum(dl);
        if (g == 0) st_d[q] = dl;
        f32x4 dq[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[dt] = (f32x4){0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NKT / 2; ++s) {
            f32x4 d0, d1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                d0[r] = sc[2 * s][r] * (dp[2 * s][r] - dl);
                d1[r] = sc[2 * s + 1][r] * (dp[2 * s + 1][r] - dl);
            }
            const bf16x8 dsf = pack_frag(d0, d1);   // dS / scale; the scale goes on the fp32 accumulators
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_tr_frag<DH>(t0, s, dt, lane), dsf, dq[dt], 0, 0, 0);
        }
        store_rows<DT>(dqbase + (size_t)qc * ld, dq, scale, q < S, g);
    }
    __syncthreads();   // every wave is done reading the K / V images; delta is visible

    // ---------------- phase 2: per 16-key tile: dV, dK (query on the MFMA row, key on the lane) ----------------
    img_stage<DH>(t0, qbase, ld, S, S_pad, wave, lane, WAVES);
    img_stage<DH>(t1, dobase, (size_t)H, S, S_pad, wave, lane, WAVES);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int kt = wave; kt < nt; kt += WAVES) {
        const int key = kt * 16 + i;
        const int kc = min(key, S - 1);
        bf16x8 kf[KS], vf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[ks] = *(const bf16x8*)(qbase + H + (size_t)kc * ld + 32 * ks + 8 * g);
            vf[ks] = *(const bf16x8*)(qbase + 2 * H + (size_t)kc * ld + 32 * ks + 8 * g);
        }
        f32x4 dv[DT], dk[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) { dv[dt] = (f32x4){0, 0, 0, 0}; dk[dt] = (f32x4){0, 0, 0, 0}; }
#pragma unroll 1
        for (int s = 0; s < (nt + 1) / 2; ++s) {
            f32x4 pp[2], dd[2];
#pragma unroll
            for (int hq = 0; hq < 2; ++hq) {
                const int qt = 2 * s + hq;
                pp[hq] = (f32x4){0, 0, 0, 0};
                dd[hq] = (f32x4){0, 0, 0, 0};
                if (hq == 1 && qt >= nt) continue;   // past the last live query tile (wave-uniform)
                f32x4 sv = (f32x4){0, 0, 0, 0}, dpv = (f32x4){0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_row_frag<DH>(t0, qt * 16 + i, ks, g), kf[ks], sv, 0, 0, 0);
                    dpv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_row_frag<DH>(t1, qt * 16 + i, ks, g), vf[ks], dpv, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qq = qt * 16 + 4 * g + r;   // < S_pad
                    const float p = __builtin_amdgcn_exp2f(fmaf(sv[r], c2, -st_m[qq]));   // 0 for query rows >= S; padding keys' rows are never stored
                    float fm = 1.0f;
                    if (DROP)
                        fm = drop_one(drop_seed, (((unsigned)blockIdx.x * (unsigned)S + (unsigned)qq) << 8) + (unsigned)key, (unsigned)drop_thr16, drop_scale);
                    pp[hq][r] = p * fm;
                    dd[hq][r] = p * (dpv[r] * fm - st_d[qq]);
                }
            }
            const bf16x8 pf = pack_frag(pp[0], pp[1]);
            const bf16x8 dsf = pack_frag(dd[0], dd[1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_tr_frag<DH>(t1, s, dt, lane), pf, dv[dt], 0, 0, 0);
                dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_tr_frag<DH>(t0, s, dt, lane), dsf, dk[dt], 0, 0, 0);
            }
        }
        store_rows<DT>(dqbase + H + (size_t)kc * ld, dk, scale, key < S, g);
        store_rows<DT>(dqbase + 2 * H + (size_t)kc * ld, dv, 1.0f, key < S, g);
    }
}

// Waves per forward workgroup at more than four query tiles (S > 64): eight, two per SIMD (at most 178 registers).  Measured at B = 256, S = 133,
// H = 768 (tools/bench_attention_wide.py, two alternating runs each): 6 x 128 forward 62 -> 47 us with dropout, 52 -> 41 us without; 4 x 192
// 80 -> 59 us and 70 -> 52 us — the nine query tiles fall 2 + 1 x 7 instead of 3 + 2 + 2 + 2, and a second wave per SIMD covers the other's LDS and MFMA
// latencies.  Results are the same bits (a tile's arithmetic does not depend on which wave takes it).  CLIBD_ATTN_WIDE_FWD_WAVES=4 (A/B knob,
// read once per process) keeps four.  The backward stays at four waves: its dQ phase needs up to 426 registers.
static int fwd_waves() {
    static const int knob = [] { const char* e = getenv("CLIBD_ATTN_WIDE_FWD_WAVES"); return e ? atoi(e) : 0; }();
    return knob == 4 ? 4 : 8;
}

constexpr int max_seq(int head_dim) { return head_dim == 128 ? 256 : 192; }

static int wide_check(const char* op, const void* qkv, int B, int S, int nheads, int head_dim, int drop_thr16) {
    if (!qkv) return fail(op, "null pointer");
    if (B <= 0 || S <= 0 || nheads <= 0) return fail(op, "non-positive shape");
    if (head_dim != 128 && head_dim != 192) return fail(op, "head_dim must be 128 or 192 (64-wide heads take clibd_attention_fwd / _bwd)");
    if (S > max_seq(head_dim)) return fail(op, head_dim == 128 ? "S must be <= 256 at head_dim 128" : "S must be <= 192 at head_dim 192 (LDS budget)");
    if ((long long)B * nheads > 0x7fffffffLL) return fail(op, "grid too large");
    if (!aligned16(qkv)) return fail(op, "alignment (16 bytes)");
    return check_dropout_args(op, B, S, nheads, drop_thr16);
}

}  // namespace wide
}  // namespace clibd

using namespace clibd;
using namespace clibd::wide;

#define WIDE_DISPATCH(DHV, MACRO)                                 \
    switch (nkt) {                                                \
        case 2: MACRO(DHV, 2); break;                             \
        case 4: MACRO(DHV, 4); break;                             \
        case 6: MACRO(DHV, 6); break;                             \
        case 8: MACRO(DHV, 8); break;                             \
        case 10: MACRO(DHV, 10); break;                           \
        case 12: MACRO(DHV, 12); break;                           \
        case 14: MACRO(128, 14); break;   /* S > 192: head_dim 128 only (wide_check) */ \
        default: MACRO(128, 16); break;                           \
    }

extern "C" int clibd_attention_wide_fwd(const void* qkv, int B, int S, int nheads, int head_dim, void* out, float* lse, uint32_t drop_seed,
                                        int drop_thr16, float drop_scale, void* stream) {
    if (int e = wide_check("attention_wide_fwd", qkv, B, S, nheads, head_dim, drop_thr16)) return e;
    if (!out) return fail("attention_wide_fwd", "null out");
    if (!aligned16(out) || ((uintptr_t)lse & 3)) return fail("attention_wide_fwd", "out / lse alignment");
    const int nkt = 2 * ((S + 31) / 32);
    const size_t lds = (size_t)2 * nkt * 16 * 2 * head_dim;
    const float scale = head_dim == 128 ? 0.08838834764831845f : 0.07216878364870322f;   // 1 / sqrt(head_dim)
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH_W(DHV, N, DRP, NWV)                                                                                                             \
    do {                                                                                                                                       \
        hipFuncSetAttribute((const void*)attention_wide_fwd_kernel<DHV, N, DRP, NWV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);    \
        hipLaunchKernelGGL((attention_wide_fwd_kernel<DHV, N, DRP, NWV>), dim3(B * nheads), dim3(64 * NWV), lds, st, (const unsigned short*)qkv, S, \
                           nheads, (unsigned short*)out, scale, drop_seed, drop_thr16, drop_scale, lse);                                       \
    } while (0)
#define LAUNCH_D(DHV, N, DRP)                                               \
    do {                                                                    \
        if (N >= 6 && fwd_waves() == 8) LAUNCH_W(DHV, (N >= 6 ? N : 6), DRP, 8); \
        else LAUNCH_W(DHV, N, DRP, WAVES);                                  \
    } while (0)
#define LAUNCH(DHV, N)                            \
    do {                                          \
        if (drop_thr16 > 0) LAUNCH_D(DHV, N, true); \
        else LAUNCH_D(DHV, N, false);             \
    } while (0)
    if (head_dim == 128) { WIDE_DISPATCH(128, LAUNCH) } else { WIDE_DISPATCH(192, LAUNCH) }
#undef LAUNCH_W
#undef LAUNCH
#undef LAUNCH_D
    return check_launch("attention_wide_fwd");
}

extern "C" int clibd_attention_wide_bwd(const void* qkv, const void* dout, const float* lse, int B, int S, int nheads, int head_dim, void* dqkv,
                                        uint32_t drop_seed, int drop_thr16, float drop_scale, void* stream) {
    if (int e = wide_check("attention_wide_bwd", qkv, B, S, nheads, head_dim, drop_thr16)) return e;
    if (!dout || !dqkv) return fail("attention_wide_bwd", "null dout / dqkv");
    if (!lse) return fail("attention_wide_bwd", "null lse: the backward needs the forward's log-sum-exp");
    if (!aligned16(dout) || !aligned16(dqkv) || ((uintptr_t)lse & 3)) return fail("attention_wide_bwd", "dout / dqkv / lse alignment");
    const int nkt = 2 * ((S + 31) / 32);
    const size_t lds = (size_t)2 * nkt * 16 * 2 * head_dim + (size_t)2 * nkt * 16 * sizeof(float);
    const float scale = head_dim == 128 ? 0.08838834764831845f : 0.07216878364870322f;
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH_D(DHV, N, DRP)                                                                                                                  \
    do {                                                                                                                                       \
        hipFuncSetAttribute((const void*)attention_wide_bwd_kernel<DHV, N, DRP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);         \
        hipLaunchKernelGGL((attention_wide_bwd_kernel<DHV, N, DRP>), dim3(B * nheads), dim3(64 * WAVES), lds, st, (const unsigned short*)qkv,   \
                           (const unsigned short*)dout, lse, S, nheads, (unsigned short*)dqkv, scale, drop_seed, drop_thr16, drop_scale);      \
    } while (0)
#define LAUNCH(DHV, N)                            \
    do {                                          \
        if (drop_thr16 > 0) LAUNCH_D(DHV, N, true); \
        else LAUNCH_D(DHV, N, false);             \
    } while (0)
    if (head_dim == 128) { WIDE_DISPATCH(128, LAUNCH) } else { WIDE_DISPATCH(192, LAUNCH) }
#undef LAUNCH
#undef LAUNCH_D
    return check_launch("attention_wide_bwd");
}
