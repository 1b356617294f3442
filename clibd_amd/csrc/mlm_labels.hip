// Masked-LM pre-training with caller-made labels for gfx950: label compaction and BERT's Bernoulli sampler (clibd_hip_mlm_labels.h).
//
// Compaction.  labels [M] is cut into tiles of 256, one per workgroup, one label per thread.
//   (1) counts[t] = labelled positions of tile t: a ballot per wave, the four wave totals through LDS;
//   (2) ONE workgroup turns counts into exclusive offsets in place: thread j owns the run counts[j per .. (j + 1) per), per = ceil(tiles /
//       256), sums it, the 256 run totals are scanned in LDS (Hillis-Steele, integers), and the run is rewritten as running offsets.
//       The same workgroup writes n_labelled and ORs the overflow bit;
//   (3) a labelled position's slot = offsets[tile] + labelled positions before it in the tile (ballot prefix + the waves before it): the
//       order is ascending by construction and every slot has one writer.  Slots at or past r_cap are dropped (the flag of (2) says so).
//       Thread g of the grid then writes the padding slot g if n <= g < r_cap: the grid spans at least r_cap threads (r_cap <=
//       ceil(M / 64) * 64 <= tiles * 256), and slot g < min(n, r_cap) is written by the position that owns it: no slot has two writers.
// Integers only; the one atomic ORs a flag bit.
//
// Sampler.  One element per thread, grid-stride; three lowbias32 draws per element (the header has the rule).
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_mlm.h"
#include "../../include/clibd_hip_mlm_labels.h"
#include "host_util.h"

namespace clibd {

constexpr int LBL_THREADS = 256;
constexpr int LBL_WAVES = 4;
constexpr unsigned LBL_GOLDEN = 0x9E3779B9u;

struct SpecialIds {
    int64_t id[CLIBD_MLM_MAX_SPECIAL];
};

// the number of labelled positions of the workgroup's tile before this thread's, and (every thread) the tile's total
__device__ __forceinline__ int tile_rank(bool flag, int* wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(flag);
    if (lane == 0) wave_tot[wave] = __builtin_popcountll(bal);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < LBL_WAVES; ++w) {
        const int c = wave_tot[w];
        before += w < wave ? c : 0;
        total += c;
    }
    return before + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(LBL_THREADS) void labels_count_kernel(const int64_t* __restrict__ labels, int M, int V, int* __restrict__ counts,
                                                                   unsigned* __restrict__ err) {
    __shared__ int wave_tot[LBL_WAVES];
    const int i = blockIdx.x * LBL_THREADS + threadIdx.x;
    const int64_t l = i < M ? labels[i] : (int64_t)CLIBD_MLM_IGNORE;
    const bool flag = l != (int64_t)CLIBD_MLM_IGNORE;
    if (flag && (l < 0 || l >= (int64_t)V) && err != nullptr) atomicOr(err, 1u);   // a flag: no order in it
    int total;
    tile_rank(flag, wave_tot, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(LBL_THREADS) void labels_offsets_kernel(int* __restrict__ counts, int tiles, int r_cap, int* __restrict__ n_labelled,
                                                                     unsigned* __restrict__ overflow) {
    __shared__ int part[2][LBL_THREADS];
    const int t = threadIdx.x;
    const int per = (tiles + LBL_THREADS - 1) / LBL_THREADS;
    const int lo = min(t * per, tiles), hi = min(lo + per, tiles);
    int run = 0;
    for (int j = lo; j < hi; ++j) run += counts[j];
    int cur = 0;
    part[0][t] = run;
    __syncthreads();
    for (int d = 1; d < LBL_THREADS; d <<= 1) {   // inclusive scan of the run totals
        part[cur ^ 1][t] = part[cur][t] + (t >= d ? part[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int off = part[cur][t] - run;
    const int n = part[cur][LBL_THREADS - 1];
    for (int j = lo; j < hi; ++j) {
        const int c = counts[j];
        counts[j] = off;
        off += c;
    }
    if (t == 0) {
        n_labelled[0] = n;
        if (n > r_cap) atomicOr(overflow, 1u);   // sticky
    }
}

__global__ __launch_bounds__(LBL_THREADS) void labels_compact_kernel(const int64_t* __restrict__ labels, int M, const int* __restrict__ offsets,
                                                                     const int* __restrict__ n_labelled, int r_cap, int* __restrict__ rows,
                                                                     int64_t* __restrict__ targets) {
    __shared__ int wave_tot[LBL_WAVES];
    const int i = blockIdx.x * LBL_THREADS + threadIdx.x;
    const int64_t l = i < M ? labels[i] : (int64_t)CLIBD_MLM_IGNORE;
    const bool flag = l != (int64_t)CLIBD_MLM_IGNORE;
    int total;
    const int slot = offsets[blockIdx.x] + tile_rank(flag, wave_tot, total);
    if (flag && slot < r_cap) {
        rows[slot] = i;
        targets[slot] = l;
    }
    if (i >= n_labelled[0] && i < r_cap) {
        rows[i] = CLIBD_MLM_PAD_ROW;
        targets[i] = (int64_t)CLIBD_MLM_IGNORE;
    }
}

__global__ __launch_bounds__(LBL_THREADS) void mlm_mask_bert_kernel(const int64_t* __restrict__ ids, const int* __restrict__ attn_mask, int M, int S,
                                                                    unsigned seed, unsigned long long thr_choose, unsigned long long thr_mask,
                                                                    unsigned long long thr_rand_end, int64_t mask_id, SpecialIds special,
                                                                    int n_special, unsigned n_plain, int64_t* __restrict__ masked,
                                                                    int64_t* __restrict__ labels) {
    for (long long g = (long long)blockIdx.x * LBL_THREADS + threadIdx.x; g < M; g += (long long)gridDim.x * LBL_THREADS) {
        const int i = (int)g;
        const int64_t id = ids[i];
        bool eligible = (i % S) != 0 && (attn_mask == nullptr || attn_mask[i] != 0);
#pragma unroll
        for (int k = 0; k < CLIBD_MLM_MAX_SPECIAL; ++k) eligible = eligible && !(k < n_special && id == special.id[k]);
        const unsigned u0 = drop_hash(seed, (unsigned)i);
        int64_t out = id, lab = (int64_t)CLIBD_MLM_IGNORE;
        if (eligible && (unsigned long long)u0 < thr_choose) {
            lab = id;
            const unsigned long long u1 = drop_hash(0u, u0 + LBL_GOLDEN);
            if (u1 < thr_mask) {
                out = mask_id;
            } else if (u1 < thr_rand_end) {
                const unsigned u2 = drop_hash(0u, u0 + 2u * LBL_GOLDEN);
                out = (int64_t)n_special + (int64_t)(((unsigned long long)u2 * n_plain) >> 32);
            }
        }
        masked[i] = out;
        labels[i] = lab;
    }
}

static inline bool aligned_to(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
static inline int tiles_of(int M) { return (M + LBL_THREADS - 1) / LBL_THREADS; }
static inline unsigned long long threshold_of(double p) { return (unsigned long long)(p * 4294967296.0 + 0.5); }

}  // namespace clibd

using namespace clibd;

extern "C" size_t clibd_mlm_compact_workspace_bytes(int M) {
    if (M <= 0 || M > CLIBD_MLM_COMPACT_MAX_M) return 0;
    return align_up((size_t)tiles_of(M) * sizeof(int), 256);
}

extern "C" int clibd_mlm_compact_labels(const int64_t* labels, int M, int V, int r_cap, int32_t* rows, int64_t* targets, int32_t* n_labelled,
                                        uint32_t* overflow, uint32_t* err, void* workspace, size_t workspace_bytes, void* stream) {
    const char* op = "mlm_compact_labels";
    if (!labels || !rows || !targets || !n_labelled || !overflow || !workspace) return fail(op, "null pointer");
    if (M <= 0 || V <= 0) return fail(op, "non-positive shape");
    if (M > CLIBD_MLM_COMPACT_MAX_M) return fail(op, "M must be at most 2^24");
    if (r_cap < 64 || r_cap % 64 != 0) return fail(op, "r_cap must be a multiple of 64, at least 64");
    if (r_cap > pad64(M)) return fail(op, "r_cap must be at most M rounded up to 64");
    if (!aligned_to(labels, 8) || !aligned_to(targets, 8) || !aligned_to(rows, 4) || !aligned_to(n_labelled, 4) || !aligned_to(overflow, 4) ||
        !aligned_to(err, 4) || !aligned16(workspace))
        return fail(op, "misaligned pointer (int64 arrays 8 bytes, int32 arrays 4 bytes, workspace 16 bytes)");
    if (workspace_bytes < clibd_mlm_compact_workspace_bytes(M)) return fail(op, "workspace too small (clibd_mlm_compact_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const int tiles = tiles_of(M);
    int* counts = (int*)workspace;
    hipLaunchKernelGGL(labels_count_kernel, dim3((unsigned)tiles), dim3(LBL_THREADS), 0, st, labels, M, V, counts, (unsigned*)err);
    if (int e = check_launch("mlm_compact_labels (count)")) return e;
    hipLaunchKernelGGL(labels_offsets_kernel, dim3(1), dim3(LBL_THREADS), 0, st, counts, tiles, r_cap, (int*)n_labelled, (unsigned*)overflow);
    if (int e = check_launch("mlm_compact_labels (offsets)")) return e;
    hipLaunchKernelGGL(labels_compact_kernel, dim3((unsigned)tiles), dim3(LBL_THREADS), 0, st, labels, M, (const int*)counts, (const int*)n_labelled,
                       r_cap, (int*)rows, targets);
    return check_launch("mlm_compact_labels");
}

extern "C" int clibd_mlm_mask_bert(const int64_t* ids, const int32_t* attn_mask, int B, int S, int V, uint32_t seed, double p_choose, double p_mask,
                                   double p_random, int64_t mask_id, const int64_t* special, int n_special, int64_t* masked, int64_t* labels,
                                   void* stream) {
    const char* op = "mlm_mask_bert";
    if (!ids || !masked || !labels) return fail(op, "null pointer");
    if (B <= 0 || S <= 0) return fail(op, "non-positive shape");
    if ((long long)B * S >= (1LL << 31)) return fail(op, "B * S must be below 2^31");
    if (n_special < 0 || n_special > CLIBD_MLM_MAX_SPECIAL) return fail(op, "n_special must be in 0..8");
    if (n_special > 0 && !special) return fail(op, "null pointer (special)");
    if (V <= n_special) return fail(op, "V must exceed n_special");
    if (!(p_choose >= 0.0 && p_choose <= 1.0) || !(p_mask >= 0.0 && p_mask <= 1.0) || !(p_random >= 0.0 && p_random <= 1.0) ||
        !(p_mask + p_random <= 1.0 + 1e-9))
        return fail(op, "probabilities must lie in [0, 1] with p_mask + p_random <= 1");
    if (!aligned_to(ids, 8) || !aligned_to(masked, 8) || !aligned_to(labels, 8) || !aligned_to(attn_mask, 4))
        return fail(op, "misaligned pointer (int64 arrays 8 bytes, the mask 4 bytes)");
    SpecialIds sp;
    for (int k = 0; k < CLIBD_MLM_MAX_SPECIAL; ++k) sp.id[k] = k < n_special ? special[k] : 0;
    const int M = B * S;
    const unsigned long long tm = threshold_of(p_mask);
    hipLaunchKernelGGL(mlm_mask_bert_kernel, dim3(grid_for((size_t)M)), dim3(LBL_THREADS), 0, (hipStream_t)stream, ids, (const int*)attn_mask, M, S,
                       (unsigned)seed, threshold_of(p_choose), tm, tm + threshold_of(p_random), mask_id, sp, n_special, (unsigned)(V - n_special), masked,
                       labels);
    return check_launch("mlm_mask_bert");
}
