// Eval-phase scoring (the reference's inference_and_print_result, bioscanclip/util/util.py:555-700, minus its Python loops).
//
// clibd_topk_label_hits: one thread per (query, level).  The thread reads the query's kmax key indices (as clibd_topk_ip /
// clibd_topk_ip_fast wrote them), gathers the kmax key labels of its level, and finds the first rank whose label equals the
// query's: `gt_label in pred_labels[:k]` for every k at once (labels are compared, not indices, so duplicate labels count).
// Counts are integer atomics, aggregated per wave first: lanes with the same (segment, level) or (segment, class) are grouped
// by a ballot loop and one leader lane adds the group's popcount.  Integer sums are exact and order-free, so the outputs are
// identical from run to run by construction (deterministic mode included).
//
// Bound: latency of the random key-label gathers (kmax dependent-free 4-byte loads per thread from a label table of Nk x L x 4
// bytes, 338 KB at 21 k keys: L2-resident), not bandwidth: Q x L x kmax x 4 bytes is 6.4 MB at 50 k queries x 4 levels x 8.
//
// clibd_eval_pair_features: the reference's averaged_feature (np.mean([img, dna], 0)) and concatenated_feature ([img | dna])
// in one streaming pass (HBM-bound: 8 N D bytes read, 12 N D bytes written).
#include "common.h"
#include "../../include/clibd_hip.h"
#include "host_util.h"

namespace clibd {

constexpr int EH_MAX_K = 8;      // kmax and n_k limit (the top-k kernels keep 8-entry lists)
constexpr int EH_MAX_L = 8;
constexpr int EH_MAX_SEG = 64;

struct EvalHitsParams {
    int k_list[EH_MAX_K];
    int class_offset[EH_MAX_L + 1];
};

// The per-wave grouping loops visit every distinct key among the counted lanes: the leader's key is broadcast with v_readlane
// (no LDS-crossbar instruction, see common.h) and a ballot selects the lanes that share it.
__global__ __launch_bounds__(256) void label_hits_kernel(const long long* __restrict__ idx, const int* __restrict__ key_labels,
                                                         const int* __restrict__ query_labels, const int* __restrict__ segment, int Q,
                                                         int kmax, int Nk, int L, int C, int n_k, int nseg, EvalHitsParams p,
                                                         int* __restrict__ first_hit, int* __restrict__ level_hits,
                                                         int* __restrict__ class_hits, int* __restrict__ class_count, int* __restrict__ error) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < (long long)Q * L;
    int q = 0, l = 0, seg = 0, cls = -1, first = kmax, err = 0;
    if (live) {
        q = (int)(t / L);
        l = (int)(t - (long long)q * L);
        const int ql = query_labels[(size_t)q * L + l];
        const int ncls = p.class_offset[l + 1] - p.class_offset[l];
        if (ql < 0 || ql >= ncls) err |= 2;
        else cls = p.class_offset[l] + ql;
        if (segment) {
            seg = segment[q];
            if (seg < 0 || seg >= nseg) { err |= 4; cls = -1; }
        }
        // all kmax index loads, then all kmax label gathers, in flight together (the gathers are the latency)
        long long id[EH_MAX_K];
#pragma unroll
        for (int r = 0; r < EH_MAX_K; ++r) id[r] = r < kmax ? idx[(size_t)q * kmax + r] : 0;
        int kl[EH_MAX_K];
#pragma unroll
        for (int r = 0; r < EH_MAX_K; ++r) {
            const bool in = id[r] >= 0 && id[r] < Nk;
            if (r < kmax && !in) err |= 1;
            kl[r] = (r < kmax && in) ? key_labels[(size_t)id[r] * L + l] : -1;
        }
#pragma unroll
        for (int r = EH_MAX_K - 1; r >= 0; --r)
            if (r < kmax && kl[r] == ql && ql >= 0) first = r;
        first_hit[(size_t)q * L + l] = first;
    }
    if (err) atomicOr(error, err);
    const bool counted = live && cls >= 0;
    // hit bits of every k of k_list (ascending: first < k)
    unsigned long long hit[EH_MAX_K];
#pragma unroll
    for (int j = 0; j < EH_MAX_K; ++j) hit[j] = j < n_k ? __ballot(counted && first < p.k_list[j]) : 0ull;
    // ---- level_hits[seg][j][l]: groups of equal (seg, level)
    unsigned long long active = __ballot(counted);
    const int lkey = seg * L + l;
    while (active) {
        const int leader = __ffsll((long long)active) - 1;
        const int key = __builtin_amdgcn_readlane(lkey, leader);
        const unsigned long long grp = __ballot(counted && lkey == key);
        if (lane == leader) {
            const int s = key / L, lv = key - s * L;
            for (int j = 0; j < n_k; ++j) {
                const int n = __popcll(grp & hit[j]);
                if (n) atomicAdd(level_hits + ((size_t)s * n_k + j) * L + lv, n);
            }
        }
        active &= ~grp;
    }
    // ---- class_count[seg][c] and class_hits[seg][j][c]: groups of equal (seg, class)
    active = __ballot(counted);
    const int ckey = seg * C + cls;
    while (active) {
        const int leader = __ffsll((long long)active) - 1;
        const int key = __builtin_amdgcn_readlane(ckey, leader);
        const unsigned long long grp = __ballot(counted && ckey == key);
        if (lane == leader) {
            const int s = key / C, c = key - s * C;
            atomicAdd(class_count + (size_t)s * C + c, __popcll(grp));
            for (int j = 0; j < n_k; ++j) {
                const int n = __popcll(grp & hit[j]);
                if (n) atomicAdd(class_hits + ((size_t)s * n_k + j) * C + c, n);
            }
        }
        active &= ~grp;
    }
}

// one thread per 4 columns of one row: avg = (img + dna) * 0.5 (the fp32 rounding of the reference's float64 mean of two fp32
// values), cat = [img | dna]
__global__ __launch_bounds__(256) void pair_features_kernel(const float* __restrict__ img, const float* __restrict__ dna, int N, int D,
                                                            float* __restrict__ avg, float* __restrict__ cat) {
    const int d4 = D / 4;
    const size_t n4 = (size_t)N * d4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const size_t n = i / d4, c = (i - n * d4) * 4;
        const float4 a = *(const float4*)(img + n * D + c);
        const float4 b = *(const float4*)(dna + n * D + c);
        *(float4*)(avg + n * D + c) = make_float4((a.x + b.x) * 0.5f, (a.y + b.y) * 0.5f, (a.z + b.z) * 0.5f, (a.w + b.w) * 0.5f);
        *(float4*)(cat + n * 2 * D + c) = a;
        *(float4*)(cat + n * 2 * D + D + c) = b;
    }
}

}  // namespace clibd

using namespace clibd;

extern "C" int clibd_topk_label_hits(const int64_t* idx, int Q, int kmax, const int32_t* key_labels, int Nk, const int32_t* query_labels, int L,
                                     const int32_t* class_offset, const int32_t* k_list, int n_k, const int32_t* segment, int nseg,
                                     int32_t* first_hit, int32_t* level_hits, int32_t* class_hits, int32_t* class_count, int32_t* error,
                                     void* stream) {
    if (!idx || !key_labels || !query_labels || !class_offset || !k_list || !first_hit || !level_hits || !class_hits || !class_count || !error)
        return set_error(CLIBD_EINVAL, "topk_label_hits: null pointer");
    if (Q <= 0 || Nk <= 0 || L < 1 || L > EH_MAX_L) return set_error(CLIBD_EINVAL, "topk_label_hits: need Q > 0, Nk > 0 and 1 <= L <= 8");
    if (kmax < 1 || kmax > EH_MAX_K) return set_error(CLIBD_EINVAL, "topk_label_hits: need 1 <= kmax <= 8");
    if (n_k < 1 || n_k > EH_MAX_K) return set_error(CLIBD_EINVAL, "topk_label_hits: need 1 <= n_k <= 8");
    if (nseg < 1 || nseg > EH_MAX_SEG || (!segment && nseg != 1)) return set_error(CLIBD_EINVAL, "topk_label_hits: need 1 <= nseg <= 64 (1 without segment)");
    EvalHitsParams p{};
    for (int j = 0; j < n_k; ++j) {
        if (k_list[j] < 1 || k_list[j] > kmax) return set_error(CLIBD_EINVAL, "topk_label_hits: need 1 <= k <= kmax for every k of k_list");
        if (j > 0 && k_list[j] <= k_list[j - 1]) return set_error(CLIBD_EINVAL, "topk_label_hits: k_list must be strictly ascending");
        p.k_list[j] = k_list[j];
    }
    if (class_offset[0] != 0) return set_error(CLIBD_EINVAL, "topk_label_hits: class_offset[0] must be 0");
    for (int l = 0; l <= L; ++l) {
        if (l > 0 && class_offset[l] < class_offset[l - 1]) return set_error(CLIBD_EINVAL, "topk_label_hits: class_offset must be non-decreasing");
        p.class_offset[l] = class_offset[l];
    }
    const long long C = class_offset[L];
    if (C < 1 || C * nseg >= (1ll << 31)) return set_error(CLIBD_EINVAL, "topk_label_hits: need 1 <= C and nseg * C < 2^31");
    if ((long long)Q * L >= (1ll << 40)) return set_error(CLIBD_EINVAL, "topk_label_hits: too many queries");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(level_hits, 0, sizeof(int32_t) * (size_t)nseg * n_k * L, st) != hipSuccess ||
        hipMemsetAsync(class_hits, 0, sizeof(int32_t) * (size_t)nseg * n_k * C, st) != hipSuccess ||
        hipMemsetAsync(class_count, 0, sizeof(int32_t) * (size_t)nseg * C, st) != hipSuccess ||
        hipMemsetAsync(error, 0, sizeof(int32_t), st) != hipSuccess)
        return set_error(CLIBD_ELAUNCH, "topk_label_hits: memset");
    const long long threads = (long long)Q * L;
    hipLaunchKernelGGL(label_hits_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (const long long*)idx, key_labels, query_labels,
                       segment, Q, kmax, Nk, L, (int)C, n_k, nseg, p, first_hit, level_hits, class_hits, class_count, error);
    return check_launch("topk_label_hits");
}

extern "C" int clibd_eval_pair_features(const float* img, const float* dna, int N, int D, float* avg, float* cat, void* stream) {
    if (!img || !dna || !avg || !cat) return set_error(CLIBD_EINVAL, "eval_pair_features: null pointer");
    if (N <= 0 || D <= 0 || D % 4 != 0) return set_error(CLIBD_EINVAL, "eval_pair_features: need N > 0 and D a positive multiple of 4");
    if (!aligned16(img) || !aligned16(dna) || !aligned16(avg) || !aligned16(cat)) return set_error(CLIBD_EINVAL, "eval_pair_features: alignment");
    hipLaunchKernelGGL(pair_features_kernel, dim3(grid_for((size_t)N * (D / 4), 256, 8192)), dim3(256), 0, (hipStream_t)stream, img, dna, N, D, avg, cat);
    return check_launch("eval_pair_features");
}
