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
//
// Seen/unseen classification by a confidence threshold (the reference's scripts/method_nn.py: decide_prediction_with_threshold inside
// search_threshold_with_harmonic_mean's loop over 1 000 thresholds).  clibd_threshold_sweep_hits runs two kernels:
//   1. sweep_masks_kernel, one thread per (query, level): gathers the m labels of source A's keys and the m of source B's (as
//      label_hits_kernel does) and writes two m-bit match masks hA | hB << 8 to the workspace.  Latency of the 2m gathers, like above.
//   2. threshold_sweep_kernel, one thread per threshold, grid = threshold tiles x query chunks.  The chunk's records (m confidences
//      widened to fp64, L mask words, the segment) are staged once in LDS and read by every lane at the same address (a broadcast,
//      no bank conflict).  Per query: m fp64 compares build the selection mask s, per level ((s & hA) | (~s & hB)) & ((1 << k) - 1)
//      is a hit.  The n_k x L counters of the current segment stay in registers and are flushed with integer atomicAdd when the
//      segment changes and at the chunk's end.  ALU-bound on paper (Q x T x (m + L (3 + 2 n_k)) lane operations: 7e8 at 16 k queries x
//      1 000 thresholds, tens of microseconds), in practice launch-bound.
// The compare is (double)conf > threshold itself: no rounded fp32 threshold, so there is nothing to prove about it.  Integer sums
// only: exact, order-free, identical from run to run.
// clibd_threshold_merge: one thread per query writes the merged index list at ONE threshold (A's index, or Nka + B's) for
// clibd_topk_label_hits against the concatenated label table.
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

constexpr int TS_TILE = 256;     // thresholds per block (one per thread)
constexpr int TS_CHUNK = 64;     // queries per block

struct SweepParams {
    unsigned kmask[EH_MAX_K];    // (1 << k) - 1 of every k of k_list, 0 beyond n_k
};

// one thread per (query, level): ws[q * L + l] = hA | hB << 8, bit r set when the label of A's (B's) rank-r key equals the query's
__global__ __launch_bounds__(256) void sweep_masks_kernel(const long long* __restrict__ idx_a, const long long* __restrict__ idx_b,
                                                          const int* __restrict__ labels_a, const int* __restrict__ labels_b,
                                                          const int* __restrict__ query_labels, const int* __restrict__ segment, int Q, int m,
                                                          int Nka, int Nkb, int L, int nseg, unsigned* __restrict__ ws, int* __restrict__ error) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)Q * L) return;
    const int q = (int)(t / L), l = (int)(t - (long long)q * L);
    const int ql = query_labels[(size_t)q * L + l];
    int err = ql < 0 ? 2 : 0;
    if (segment && l == 0) {
        const int sg = segment[q];
        if (sg < 0 || sg >= nseg) err |= 4;
    }
    long long ia[EH_MAX_K], ib[EH_MAX_K];
#pragma unroll
    for (int r = 0; r < EH_MAX_K; ++r) {
        ia[r] = r < m ? idx_a[(size_t)q * m + r] : 0;
        ib[r] = r < m ? idx_b[(size_t)q * m + r] : 0;
    }
    int la[EH_MAX_K], lb[EH_MAX_K];
#pragma unroll
    for (int r = 0; r < EH_MAX_K; ++r) {
        const bool in_a = ia[r] >= 0 && ia[r] < Nka, in_b = ib[r] >= 0 && ib[r] < Nkb;
        if (r < m && !(in_a && in_b)) err |= 1;
        la[r] = (r < m && in_a) ? labels_a[(size_t)ia[r] * L + l] : -1;
        lb[r] = (r < m && in_b) ? labels_b[(size_t)ib[r] * L + l] : -1;
    }
    unsigned w = 0;
#pragma unroll
    for (int r = 0; r < EH_MAX_K; ++r) {
        if (r < m && ql >= 0 && la[r] == ql) w |= 1u << r;
        if (r < m && ql >= 0 && lb[r] == ql) w |= 0x100u << r;
    }
    ws[t] = w;
    if (err) atomicOr(error, err);
}

// one thread per threshold; block (x, y) = threshold tile x, query chunk y
__global__ __launch_bounds__(TS_TILE) void threshold_sweep_kernel(const float* __restrict__ conf, const unsigned* __restrict__ ws,
                                                                  const int* __restrict__ segment, const double* __restrict__ thresholds, int Q,
                                                                  int m, int L, int nseg, int T, int n_k, SweepParams p,
                                                                  int* __restrict__ level_hits) {
    __shared__ double s_conf[TS_CHUNK][EH_MAX_K];
    __shared__ unsigned s_mask[TS_CHUNK][EH_MAX_L];
    __shared__ int s_seg[TS_CHUNK];
    const int q0 = blockIdx.y * TS_CHUNK;
    const int nq = min(TS_CHUNK, Q - q0);
    for (int i = threadIdx.x; i < nq * EH_MAX_K; i += TS_TILE) {
        const int qi = i / EH_MAX_K, j = i - qi * EH_MAX_K;
        s_conf[qi][j] = j < m ? (double)conf[(size_t)(q0 + qi) * m + j] : 0.0;
        s_mask[qi][j] = j < L ? ws[(size_t)(q0 + qi) * L + j] : 0u;
    }
    for (int qi = threadIdx.x; qi < nq; qi += TS_TILE) {
        const int sg = segment ? segment[q0 + qi] : 0;
        s_seg[qi] = (sg >= 0 && sg < nseg) ? sg : -1;       // a segment out of range: reported by the mask pass, never counted
    }
    __syncthreads();
    const int t = blockIdx.x * TS_TILE + threadIdx.x;
    if (t >= T) return;
    const double thr = thresholds[t];
    int cnt[EH_MAX_K][EH_MAX_L];
#pragma unroll
    for (int i = 0; i < EH_MAX_K; ++i)
#pragma unroll
        for (int l = 0; l < EH_MAX_L; ++l) cnt[i][l] = 0;
    int cur = -1;
    auto flush = [&]() {
        int* out = level_hits + ((size_t)t * nseg + cur) * n_k * L;
#pragma unroll
        for (int i = 0; i < EH_MAX_K; ++i)
#pragma unroll
            for (int l = 0; l < EH_MAX_L; ++l)
                if (i < n_k && l < L) {
                    if (cnt[i][l]) atomicAdd(out + i * L + l, cnt[i][l]);
                    cnt[i][l] = 0;
                }
    };
    for (int qi = 0; qi < nq; ++qi) {
        const int sg = s_seg[qi];                            // the same for every lane: a scalar branch
        if (sg < 0) continue;
        if (sg != cur) {
            if (cur >= 0) flush();
            cur = sg;
        }
        unsigned s = 0;
#pragma unroll
        for (int j = 0; j < EH_MAX_K; ++j)
            if (j < m && s_conf[qi][j] > thr) s |= 1u << j;  // strict and per position; a NaN confidence (or threshold) selects B
#pragma unroll
        for (int l = 0; l < EH_MAX_L; ++l)
            if (l < L) {
                const unsigned w = s_mask[qi][l];
                const unsigned sel = (s & w) | (~s & (w >> 8));
#pragma unroll
                for (int i = 0; i < EH_MAX_K; ++i)
                    if (i < n_k) cnt[i][l] += (sel & p.kmask[i]) != 0;
            }
    }
    if (cur >= 0) flush();
}

// one thread per query: merged_idx[q, j] = idx_a[q, j] if (double)conf[q, j] > threshold, else Nka + idx_b[q, j]; from_a[q]: the bits of A
__global__ __launch_bounds__(256) void threshold_merge_kernel(const float* __restrict__ conf, const long long* __restrict__ idx_a,
                                                              const long long* __restrict__ idx_b, int Q, int m, int Nka, int Nkb, double threshold,
                                                              long long* __restrict__ merged, int* __restrict__ from_a, int* __restrict__ error) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    int bits = 0;
    bool bad = false;
    for (int j = 0; j < m; ++j) {
        const size_t e = (size_t)q * m + j;
        const long long a = idx_a[e], b = idx_b[e];
        const bool in_a = a >= 0 && a < Nka, in_b = b >= 0 && b < Nkb;
        bad |= !(in_a && in_b);
        const bool sel = (double)conf[e] > threshold;
        if (sel) bits |= 1 << j;
        merged[e] = sel ? (in_a ? a : -1) : (in_b ? (long long)Nka + b : -1);   // an offending entry becomes -1 (clibd_topk_label_hits refuses it too)
    }
    from_a[q] = bits;
    if (bad) atomicOr(error, 1);
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

extern "C" size_t clibd_threshold_sweep_workspace_bytes(int Q, int L) {
    if (Q <= 0 || L < 1 || L > EH_MAX_L) return 0;
    return sizeof(uint32_t) * (size_t)Q * L;
}

extern "C" int clibd_threshold_sweep_hits(const float* conf, const int64_t* idx_a, const int64_t* idx_b, int Q, int m, const int32_t* key_labels_a,
                                          int Nka, const int32_t* key_labels_b, int Nkb, const int32_t* query_labels, int L, const int32_t* segment,
                                          int nseg, const double* thresholds, int T, const int32_t* k_list, int n_k, int32_t* level_hits,
                                          int32_t* error, void* workspace, size_t workspace_bytes, void* stream) {
    if (!conf || !idx_a || !idx_b || !key_labels_a || !key_labels_b || !query_labels || !thresholds || !k_list || !level_hits || !error || !workspace)
        return set_error(CLIBD_EINVAL, "threshold_sweep_hits: null pointer");
    if (Q <= 0 || Nka <= 0 || Nkb <= 0 || L < 1 || L > EH_MAX_L)
        return set_error(CLIBD_EINVAL, "threshold_sweep_hits: need Q > 0, Nka > 0, Nkb > 0 and 1 <= L <= 8");
    if (m < 1 || m > EH_MAX_K) return set_error(CLIBD_EINVAL, "threshold_sweep_hits: need 1 <= m <= 8");
    if (n_k < 1 || n_k > EH_MAX_K) return set_error(CLIBD_EINVAL, "threshold_sweep_hits: need 1 <= n_k <= 8");
    if (T < 1) return set_error(CLIBD_EINVAL, "threshold_sweep_hits: need T >= 1");
    if (nseg < 1 || nseg > EH_MAX_SEG || (!segment && nseg != 1))
        return set_error(CLIBD_EINVAL, "threshold_sweep_hits: need 1 <= nseg <= 64 (1 without segment)");
    SweepParams p{};
    for (int j = 0; j < n_k; ++j) {
        if (k_list[j] < 1 || k_list[j] > m) return set_error(CLIBD_EINVAL, "threshold_sweep_hits: need 1 <= k <= m for every k of k_list");
        if (j > 0 && k_list[j] <= k_list[j - 1]) return set_error(CLIBD_EINVAL, "threshold_sweep_hits: k_list must be strictly ascending");
        p.kmask[j] = (1u << k_list[j]) - 1u;
    }
    const long long entries = (long long)T * nseg * n_k * L;
    if (entries >= (1ll << 31)) return set_error(CLIBD_EINVAL, "threshold_sweep_hits: level_hits [T, nseg, n_k, L] must stay below 2^31 entries");
    if ((long long)Q * L >= (1ll << 40)) return set_error(CLIBD_EINVAL, "threshold_sweep_hits: too many queries");
    const long long chunks = ((long long)Q + TS_CHUNK - 1) / TS_CHUNK;
    if (chunks > 65535) return set_error(CLIBD_EINVAL, "threshold_sweep_hits: more than 65535 * 64 queries");
    if (workspace_bytes < clibd_threshold_sweep_workspace_bytes(Q, L) || !aligned16(workspace))
        return set_error(CLIBD_EINVAL, "threshold_sweep_hits: workspace too small or misaligned (clibd_threshold_sweep_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(level_hits, 0, sizeof(int32_t) * (size_t)entries, st) != hipSuccess || hipMemsetAsync(error, 0, sizeof(int32_t), st) != hipSuccess)
        return set_error(CLIBD_ELAUNCH, "threshold_sweep_hits: memset");
    const long long threads = (long long)Q * L;
    hipLaunchKernelGGL(sweep_masks_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (const long long*)idx_a, (const long long*)idx_b,
                       key_labels_a, key_labels_b, query_labels, segment, Q, m, Nka, Nkb, L, nseg, (unsigned*)workspace, error);
    hipLaunchKernelGGL(threshold_sweep_kernel, dim3((unsigned)((T + TS_TILE - 1) / TS_TILE), (unsigned)chunks), dim3(TS_TILE), 0, st, conf,
                       (const unsigned*)workspace, segment, thresholds, Q, m, L, nseg, T, n_k, p, level_hits);
    return check_launch("threshold_sweep_hits");
}

extern "C" int clibd_threshold_merge(const float* conf, const int64_t* idx_a, const int64_t* idx_b, int Q, int m, int Nka, int Nkb, double threshold,
                                     int64_t* merged_idx, int32_t* from_a, int32_t* error, void* stream) {
    if (!conf || !idx_a || !idx_b || !merged_idx || !from_a || !error) return set_error(CLIBD_EINVAL, "threshold_merge: null pointer");
    if (Q <= 0 || Nka <= 0 || Nkb <= 0) return set_error(CLIBD_EINVAL, "threshold_merge: need Q > 0, Nka > 0 and Nkb > 0");
    if (m < 1 || m > EH_MAX_K) return set_error(CLIBD_EINVAL, "threshold_merge: need 1 <= m <= 8");
    if ((long long)Q * m >= (1ll << 31)) return set_error(CLIBD_EINVAL, "threshold_merge: merged_idx [Q, m] must stay below 2^31 entries");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(error, 0, sizeof(int32_t), st) != hipSuccess) return set_error(CLIBD_ELAUNCH, "threshold_merge: memset");
    hipLaunchKernelGGL(threshold_merge_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, conf, (const long long*)idx_a, (const long long*)idx_b, Q,
                       m, Nka, Nkb, threshold, (long long*)merged_idx, from_a, error);
    return check_launch("threshold_merge");
}

extern "C" int clibd_eval_pair_features(const float* img, const float* dna, int N, int D, float* avg, float* cat, void* stream) {
    if (!img || !dna || !avg || !cat) return set_error(CLIBD_EINVAL, "eval_pair_features: null pointer");
    if (N <= 0 || D <= 0 || D % 4 != 0) return set_error(CLIBD_EINVAL, "eval_pair_features: need N > 0 and D a positive multiple of 4");
    if (!aligned16(img) || !aligned16(dna) || !aligned16(avg) || !aligned16(cat)) return set_error(CLIBD_EINVAL, "eval_pair_features: alignment");
    hipLaunchKernelGGL(pair_features_kernel, dim3(grid_for((size_t)N * (D / 4), 256, 8192)), dim3(256), 0, (hipStream_t)stream, img, dna, N, D, avg, cat);
    return check_launch("eval_pair_features");
}
