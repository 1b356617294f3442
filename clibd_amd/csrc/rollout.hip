// Attention rollout (reference: scripts/result/representation_visualization/{image,dna}_representation_visualization.py, `rollout`) for
// gfx950: the fused attention map of a layer recomputed from its packed qkv, the exact discard of its k smallest entries, and the chain.
//
// Fused maps.  The attention kernels (attention.hip) are flash-style and never hold the probabilities P in memory, so there is nothing to
// hook: P is recomputed here.  One workgroup (4 waves) owns 64 queries of one image — one 16-query tile per wave — and walks the heads.
// Per head the K rows [S_pad][64] bf16 are staged into LDS as the attention kernels' head image (attn_image.h: layout, LDS-DMA staging,
// row fragments, NEG_BIG), double buffered so that the next head's K arrives under this head's arithmetic.  S^T = K.Q^T runs on
// v_mfma_f32_16x16x32_bf16 in the attention kernels' orientation (key on the MFMA row, query on the lane): a lane holds ONE query (lane & 15)
// and the keys 16 kt + 4 (lane >> 4) + r, all of them in <= 64 accumulators, so the softmax is an exact full-row softmax in fp32.  The
// probabilities fold into a second register set of the same shape (running sum, max or min) and after the last head one 16-byte store
// per (lane, key tile) writes the fused row: S * ld floats per image reach memory, not heads * S * S.
//
// Discard.  One workgroup per map.  The entries are non-negative floats, so their bit patterns order as uint32: four passes of an 8-bit
// radix select with a 256-bin LDS histogram (integer LDS atomics; the counts do not depend on the order) find the k-th smallest value t
// exactly; the map (<= 256 KB) is re-read from L2.  Entries below t go to 0, entries equal to t in ascending flat index until k are taken
// (an ordered block scan, only when some but not all of them are taken), flat index 0 never.
//
// Chain.  Only row 0 of the reference's matrix product is read, so the chain is a vector-matrix walk from the last selected layer to
// the first: thread j accumulates sum_i v[i] a[i, j] as four interleaved fma chains over i, combined pairwise (loads coalesced across j).
// One workgroup per image.
#include "attn_image.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_rollout.h"

namespace clibd {

constexpr int RO_THREADS = 256;
constexpr int RO_WAVES = 4;
constexpr int RO_DH = 64;
constexpr int RO_MAX_S = 256;
constexpr int SEL_THREADS = 1024;

// NKT: 16-key tiles held per lane (S <= 16 NKT).  Grid: B * ngroups workgroups, workgroup (b, grp) owns query tiles 4 grp .. 4 grp + 3.
template <int NKT>
__global__ __launch_bounds__(RO_THREADS) void attn_fused_maps_kernel(const unsigned short* __restrict__ qkv, int S, int nheads, int fusion,
                                                                     float* __restrict__ out, int ld, int ngroups) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int S_pad = 16 * NKT;
    constexpr int IMG = S_pad * 128;   // bytes of one K image
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x / ngroups, grp = blockIdx.x % ngroups;
    const int H = nheads * RO_DH;
    const size_t ldq = (size_t)3 * H;
    const unsigned short* base = qkv + (size_t)b * S * ldq;
    const int g = lane >> 4, i = lane & 15;
    const int q = (grp * RO_WAVES + wave) * 16 + i;
    const int qc = min(q, S - 1);
    const bool active = (grp * RO_WAVES + wave) * 16 < S;   // wave-uniform: a wave without a live query still stages and waits
    const float c2 = 0.125f * 1.4426950408889634f;          // p = exp2(c2 * s - c2 * max): 1 / sqrt(64) folded with log2(e)

    f32x4 fz[NKT];
    const float init = fusion == CLIBD_FUSE_MIN ? __builtin_huge_valf() : 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) fz[kt] = (f32x4){init, init, init, init};

    bf16x8 qn[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qn[ks] = *(const bf16x8*)(base + (size_t)qc * ldq + 32 * ks + 8 * g);
    img_stage<RO_DH>(smem, base + H, ldq, S, S_pad, wave, lane, RO_WAVES);

    for (int h = 0; h < nheads; ++h) {
        // head h's K image and Q fragment have arrived; every wave is done with the other image (it read it for head h - 1)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        bf16x8 qf[2] = {qn[0], qn[1]};
        if (h + 1 < nheads) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) qn[ks] = *(const bf16x8*)(base + (size_t)qc * ldq + (h + 1) * RO_DH + 32 * ks + 8 * g);
            img_stage<RO_DH>(smem + ((h + 1) & 1) * IMG, base + H + (h + 1) * RO_DH, ldq, S, S_pad, wave, lane, RO_WAVES);
        }
        if (!active) continue;
        const char* kt_lds = smem + (h & 1) * IMG;
        int nlive = S - 4 * g;   // this lane's key 16 kt + 4 g + r is live iff 16 kt + r < nlive
        asm volatile("" : "+v"(nlive));   // re-derived per head: hoisted out of the head loop, the 64 compare masks cost the scalar registers
        f32x4 sc[NKT];
        float mx = NEG_BIG;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            sc[kt] = (f32x4){0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(img_row_frag<RO_DH>(kt_lds, kt * 16 + i, ks, g), qf[ks], sc[kt], 0, 0, 0);
            if (kt * 16 + 15 >= S) {   // a tile that holds padded keys
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt * 16 + r >= nlive) sc[kt][r] = NEG_BIG;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[kt][r]);
        }
        mx = rows4_max(mx);
        const float mc = mx * c2;
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(fmaf(sc[kt][r], c2, -mc));   // a masked score underflows to exactly 0
                sc[kt][r] = e;
                sum += e;
            }
        sum = rows4_sum(sum);
        const float inv = 1.0f / sum;
        if (fusion == CLIBD_FUSE_MEAN) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) fz[kt][r] += sc[kt][r] * inv;
        } else if (fusion == CLIBD_FUSE_MAX) {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) fz[kt][r] = fmaxf(fz[kt][r], sc[kt][r] * inv);
        } else {
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) fz[kt][r] = fminf(fz[kt][r], sc[kt][r] * inv);
        }
    }
    if (!active || q >= S) return;
    const float nh = (float)nheads;
    float* orow = out + ((size_t)b * S + q) * ld;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        const int key0 = kt * 16 + 4 * g;
        if (key0 >= ld) continue;   // ld % 4 == 0: key0 + 3 < ld
        f32x4 v = fz[kt];
        if (fusion == CLIBD_FUSE_MEAN) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = v[r] / nh;
        }
        *(float4*)(orow + key0) = make_float4(v[0], v[1], v[2], v[3]);   // keys >= S: exactly 0
    }
}

// One workgroup per map.  rec[4 b ..]: bits of t, entries below t, entries equal to t that are taken, k.
__global__ __launch_bounds__(SEL_THREADS) void rollout_discard_kernel(float* __restrict__ maps, int S, int ld, int k, unsigned* __restrict__ rec) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_rem;
    __shared__ unsigned s_wcnt[SEL_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* m = maps + (size_t)blockIdx.x * S * ld;
    unsigned* myrec = rec + 4 * (size_t)blockIdx.x;
    const int n = S * S;
    if (k <= 0) {
        if (tid < 4) myrec[tid] = 0u;
        return;
    }
    // the rem-th smallest (1-based) of the entries whose high bits equal `prefix`
    unsigned prefix = 0u, rem = (unsigned)k;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int idx = tid; idx < n; idx += SEL_THREADS) {
            const int i = idx / S, j = idx - i * S;
            const unsigned u = __float_as_uint(m[(size_t)i * ld + j]);
            if (pass == 0 || (u >> (shift + 8)) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0u, bin = 255u;
            for (unsigned bb = 0; bb < 256u; ++bb) {
                const unsigned c = hist[bb];
                if (cum + c >= rem) {
                    bin = bb;
                    break;
                }
                cum += c;
            }
            s_prefix = (prefix << 8) | bin;
            s_rem = rem - cum;
        }
        __syncthreads();
        prefix = s_prefix;
        rem = s_rem;
    }
    const unsigned t = prefix;
    const unsigned cnt_eq = hist[t & 255u];   // the last pass's histogram: entries equal to t
    if (tid == 0) {
        myrec[0] = t;
        myrec[1] = (unsigned)k - rem;
        myrec[2] = rem;
        myrec[3] = (unsigned)k;
    }
    if (rem >= cnt_eq) {   // every entry equal to t is taken: no order needed
        for (int idx = tid; idx < n; idx += SEL_THREADS) {
            const int i = idx / S, j = idx - i * S;
            float* p = m + (size_t)i * ld + j;
            if (idx != 0 && __float_as_uint(*p) <= t) *p = 0.f;
        }
        return;
    }
    // some of the entries equal to t stay: rank them by flat index with an ordered block scan (index 0 takes a rank, and keeps its value)
    unsigned running = 0u;
    for (int base = 0; base < n; base += SEL_THREADS) {
        const int idx = base + tid;
        const bool valid = idx < n;
        const int ic = valid ? idx : 0;
        const int i = ic / S, j = ic - i * S;
        float* p = m + (size_t)i * ld + j;
        const unsigned u = __float_as_uint(*p);
        const bool eq = valid && u == t;
        const bool less = valid && u < t;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(eq);
        const unsigned lrank = (unsigned)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wcnt[wave] = (unsigned)__builtin_popcountll(bal);
        __syncthreads();
        unsigned off = running, tot = 0u;
        for (int w = 0; w < SEL_THREADS / 64; ++w) {
            const unsigned c = s_wcnt[w];
            if (w < wave) off += c;
            tot += c;
        }
        if (idx != 0 && (less || (eq && off + lrank < rem))) *p = 0.f;
        running += tot;
        __syncthreads();
    }
}

// One workgroup per image, thread j owns column j.
__global__ __launch_bounds__(RO_THREADS) void rollout_chain_kernel(const float* __restrict__ maps, int L, int B, int S, int ld, float* __restrict__ out) {
    __shared__ float v[RO_MAX_S];
    __shared__ float r[RO_MAX_S];
    __shared__ float red[RO_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    v[tid] = tid == 0 ? 1.f : 0.f;
    for (int l = L - 1; l >= 0; --l) {
        const float* F = maps + ((size_t)l * B + b) * S * ld;
        for (int row = wave; row < S; row += RO_WAVES) {   // r[row]: the lanes' strided shares, then the wave's butterfly — one order
            float s = 0.f;
            for (int kk = lane; kk < S; kk += 64) s += F[(size_t)row * ld + kk];
            s = wave_sum(s);
            if (lane == 0) r[row] = (s + 1.0f) * 0.5f;
        }
        __syncthreads();
        float acc = 0.f;
        if (tid < S) {
            // four interleaved fma chains (i mod 4), combined pairwise: one fixed order, four loads in flight, and a quarter of the
            // chain length a single accumulator would round through
            float p[4] = {0.f, 0.f, 0.f, 0.f};
            auto term = [&](int i, float& s) {
                const float a = (F[(size_t)i * ld + tid] + (i == tid ? 1.0f : 0.f)) * 0.5f;
                s = __builtin_fmaf(v[i], a, s);
            };
            int i = 0;
            for (; i + 4 <= S; i += 4) {
                term(i, p[0]);
                term(i + 1, p[1]);
                term(i + 2, p[2]);
                term(i + 3, p[3]);
            }
            if (i < S) term(i, p[0]);
            if (i + 1 < S) term(i + 1, p[1]);
            if (i + 2 < S) term(i + 2, p[2]);
            acc = ((p[0] + p[1]) + (p[2] + p[3])) / r[tid];
        }
        __syncthreads();   // every thread has read v
        v[tid] = acc;
        __syncthreads();
    }
    float mx = (tid >= 1 && tid < S) ? v[tid] : -__builtin_huge_valf();
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (tid >= 1 && tid < S) out[(size_t)b * (S - 1) + tid - 1] = v[tid] / mx;
}

template <int NKT>
static int launch_fused(const unsigned short* qkv, int B, int S, int heads, int fusion, float* out, int ld, hipStream_t st) {
    const int lds = 2 * 16 * NKT * 128;
    if (hipFuncSetAttribute((const void*)attn_fused_maps_kernel<NKT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return set_error(CLIBD_ELAUNCH, "attn_fused_maps: cannot reserve the K images in LDS");
    const int ngroups = ((S + 15) / 16 + RO_WAVES - 1) / RO_WAVES;
    hipLaunchKernelGGL(attn_fused_maps_kernel<NKT>, dim3((unsigned)B * ngroups), dim3(RO_THREADS), lds, st, qkv, S, heads, fusion, out, ld, ngroups);
    return check_launch("attn_fused_maps");
}

}  // namespace clibd

using namespace clibd;

extern "C" int clibd_attn_fused_maps(const void* qkv, int B, int S, int heads, int fusion, float* out, int ld, void* stream) {
    if (!qkv || !out) return set_error(CLIBD_EINVAL, "attn_fused_maps: null pointer");
    if (B <= 0 || heads <= 0 || S <= 0) return set_error(CLIBD_EINVAL, "attn_fused_maps: non-positive shape");
    if (S > RO_MAX_S) return set_error(CLIBD_EINVAL, "attn_fused_maps: S must be at most 256");
    if (fusion != CLIBD_FUSE_MEAN && fusion != CLIBD_FUSE_MAX && fusion != CLIBD_FUSE_MIN)
        return set_error(CLIBD_EINVAL, "attn_fused_maps: fusion must be CLIBD_FUSE_MEAN, CLIBD_FUSE_MAX or CLIBD_FUSE_MIN");
    if (ld < S || ld % 4 != 0) return set_error(CLIBD_EINVAL, "attn_fused_maps: ld must be >= S and a multiple of 4");
    if (!aligned16(qkv) || !aligned16(out)) return set_error(CLIBD_EINVAL, "attn_fused_maps: qkv and out must be 16-byte aligned");
    if ((long long)B * (((S + 15) / 16 + RO_WAVES - 1) / RO_WAVES) > 0x7fffffffLL || heads > (1 << 16))
        return set_error(CLIBD_EINVAL, "attn_fused_maps: batch or head count too large");
    const unsigned short* x = (const unsigned short*)qkv;
    hipStream_t st = (hipStream_t)stream;
    const int nkt = (S + 15) / 16;
    if (nkt <= 2) return launch_fused<2>(x, B, S, heads, fusion, out, ld, st);
    if (nkt <= 4) return launch_fused<4>(x, B, S, heads, fusion, out, ld, st);
    if (nkt <= 6) return launch_fused<6>(x, B, S, heads, fusion, out, ld, st);
    if (nkt <= 9) return launch_fused<9>(x, B, S, heads, fusion, out, ld, st);
    if (nkt <= 13) return launch_fused<13>(x, B, S, heads, fusion, out, ld, st);
    return launch_fused<16>(x, B, S, heads, fusion, out, ld, st);
}

extern "C" size_t clibd_rollout_discard_workspace_bytes(int B) { return B > 0 ? (size_t)B * 16 : 0; }

extern "C" int clibd_rollout_discard(float* maps, int B, int S, int ld, int k, void* workspace, size_t workspace_bytes, void* stream) {
    if (!maps || !workspace) return set_error(CLIBD_EINVAL, "rollout_discard: null pointer");
    if (B <= 0 || S <= 0) return set_error(CLIBD_EINVAL, "rollout_discard: non-positive shape");
    if (S > RO_MAX_S) return set_error(CLIBD_EINVAL, "rollout_discard: S must be at most 256");
    if (ld < S) return set_error(CLIBD_EINVAL, "rollout_discard: ld must be >= S");
    if (k < 0 || k > S * S) return set_error(CLIBD_EINVAL, "rollout_discard: k must be in 0..S*S");
    if (!aligned16(workspace) || workspace_bytes < clibd_rollout_discard_workspace_bytes(B))
        return set_error(CLIBD_EINVAL, "rollout_discard: workspace too small or misaligned (clibd_rollout_discard_workspace_bytes)");
    hipLaunchKernelGGL(rollout_discard_kernel, dim3(B), dim3(SEL_THREADS), 0, (hipStream_t)stream, maps, S, ld, k, (unsigned*)workspace);
    return check_launch("rollout_discard");
}

extern "C" int clibd_rollout_chain(const float* maps, int L, int B, int S, int ld, float* out, void* stream) {
    if (!maps || !out) return set_error(CLIBD_EINVAL, "rollout_chain: null pointer");
    if (L <= 0 || B <= 0) return set_error(CLIBD_EINVAL, "rollout_chain: non-positive shape");
    if (S < 2 || S > RO_MAX_S) return set_error(CLIBD_EINVAL, "rollout_chain: S must be in 2..256");
    if (ld < S) return set_error(CLIBD_EINVAL, "rollout_chain: ld must be >= S");
    hipLaunchKernelGGL(rollout_chain_kernel, dim3(B), dim3(RO_THREADS), 0, (hipStream_t)stream, maps, L, B, S, ld, out);
    return check_launch("rollout_chain");
}
