// Masked-k-mer pre-training of the BarcodeBERT tower (HF BertForMaskedLM(input_ids, labels)) for gfx950: what the towers' kernels lack.
//
// Sampler.  One wave per sequence (four sequences per workgroup).  Position s >= 1 gets the 64-bit key
//   (id == unk) << 40 | lowbias32((b S + s) ^ seed) << 8 | s
// — distinct within a sequence, ordered as the header's triple — and the wave's keys go to LDS.  A lane owns the positions lane + 64 j
// (S <= 256: at most four) and ranks each by counting the keys below it (every lane reads the same LDS word: a broadcast).  A position
// is chosen iff its rank is below n_mask; its slot among the chosen, ascending in s, is a ballot prefix count.  The number of rows,
// B n_mask, is a host quantity, so nothing is read back.  n_valid is counted by a second one-workgroup kernel (integers, tree sum).
//
// Gather / scatter.  16-byte chunks, grid-stride.  The scatter is two launches on the stream: zeros over all of out, then the listed rows.
//
// Cross-entropy.  One wave per row of bf16 logits (four rows per workgroup), three sweeps of 16-byte chunks, chunk c = lane + 64 k in
// ascending k: (1) max, arg max (strict >, so the lowest index wins inside a lane; across lanes the lowest index among the lanes that
// hold the max) and the target's logit picked out of the registers; (2) sum of exp(x - max); (3) the gradient over the logits in place.
// A lane writes only chunks it read itself, and nothing is re-read from memory after sweep 3 began.  fp32 statistics, expf / logf / a
// true division (the loss is compared with an fp32 evaluation of the same formula).  The wave reductions are the DPP / permlane ones of
// common.h.  `correct` is an integer atomic onto a word the entry zeroes; the loss is finished by one workgroup in one order.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_mlm.h"
#include "host_util.h"

namespace clibd {

constexpr int MLM_THREADS = 256;
constexpr int MLM_WAVES = 4;
constexpr int MLM_MAX_S = 256;
constexpr int MLM_MAX_V = 8192;

__global__ __launch_bounds__(MLM_THREADS) void mlm_mask_kernel(const int64_t* __restrict__ ids, int B, int S, unsigned seed, int n_mask,
                                                               int64_t mask_id, int64_t unk_id, int64_t* __restrict__ masked,
                                                               int* __restrict__ rows, int64_t* __restrict__ targets) {
    __shared__ unsigned long long keys[MLM_WAVES][MLM_MAX_S];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x * MLM_WAVES + wave;
    const bool live = b < B;   // wave-uniform; a wave past the batch still meets the barrier
    const size_t base = (size_t)(live ? b : 0) * S;
    int64_t id[4];
    unsigned long long key[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int s = lane + 64 * j;
        id[j] = 0;
        key[j] = ~0ull;   // position 0 and positions past the sequence rank after every real key
        if (live && s < S) {
            id[j] = ids[base + s];
            if (s >= 1)
                key[j] = ((unsigned long long)(id[j] == unk_id) << 40) | ((unsigned long long)drop_hash(seed, (unsigned)(base + s)) << 8) | (unsigned)s;
        }
        keys[wave][s] = key[j];
    }
    __syncthreads();
    int before = 0;   // chosen positions of the sequence below this lane's, over the groups of 64 done so far
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (64 * j >= S) break;   // wave-uniform: no position of this group exists
        const int s = lane + 64 * j;
        int rank = 0;
        for (int t = 1; t < S; ++t) rank += keys[wave][t] < key[j] ? 1 : 0;
        const bool chosen = live && s >= 1 && s < S && rank < n_mask;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(chosen);
        const int slot = before + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
        before += __builtin_popcountll(bal);
        if (live && s < S) masked[base + s] = chosen ? mask_id : id[j];
        if (chosen) {
            const size_t o = (size_t)b * n_mask + slot;
            rows[o] = (int)(base + s);
            targets[o] = id[j] == unk_id ? (int64_t)CLIBD_MLM_IGNORE : id[j];
        }
    }
}

// n_valid[0] = #{i < n : targets[i] != IGNORE}; one workgroup
__global__ __launch_bounds__(MLM_THREADS) void mlm_count_valid_kernel(const int64_t* __restrict__ targets, int n, int* __restrict__ n_valid) {
    __shared__ int part[MLM_THREADS];
    int c = 0;
    for (int i = threadIdx.x; i < n; i += MLM_THREADS) c += targets[i] != (int64_t)CLIBD_MLM_IGNORE ? 1 : 0;
    c = block_tree_sum(c, part);
    if (threadIdx.x == 0) n_valid[0] = c;
}

// chunk = 8 bf16 = 16 bytes; hc = H / 8
__global__ __launch_bounds__(MLM_THREADS) void rows_gather_kernel(const uint4* __restrict__ x, int M, int hc, const int* __restrict__ rows, int R,
                                                                  uint4* __restrict__ out) {
    const long long total = (long long)R * hc;
    for (long long i = (long long)blockIdx.x * MLM_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * MLM_THREADS) {
        const int r = (int)(i / hc), c = (int)(i - (long long)r * hc);
        const int m = rows[r];
        out[i] = (m >= 0 && m < M) ? x[(size_t)m * hc + c] : make_uint4(0u, 0u, 0u, 0u);
    }
}

__global__ __launch_bounds__(MLM_THREADS) void rows_zero_kernel(uint4* __restrict__ out, long long total) {
    for (long long i = (long long)blockIdx.x * MLM_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * MLM_THREADS)
        out[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(MLM_THREADS) void rows_scatter_kernel(const uint4* __restrict__ src, const int* __restrict__ rows, int R, int M, int hc,
                                                                   uint4* __restrict__ out) {
    const long long total = (long long)R * hc;
    for (long long i = (long long)blockIdx.x * MLM_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * MLM_THREADS) {
        const int r = (int)(i / hc), c = (int)(i - (long long)r * hc);
        const int m = rows[r];
        if (m >= 0 && m < M) out[(size_t)m * hc + c] = src[i];
    }
}

__device__ __forceinline__ void unpack8(uint4 v, float x[8]) {
    x[0] = bf2f((unsigned short)(v.x & 0xffffu)); x[1] = bf2f((unsigned short)(v.x >> 16));
    x[2] = bf2f((unsigned short)(v.y & 0xffffu)); x[3] = bf2f((unsigned short)(v.y >> 16));
    x[4] = bf2f((unsigned short)(v.z & 0xffffu)); x[5] = bf2f((unsigned short)(v.z >> 16));
    x[6] = bf2f((unsigned short)(v.w & 0xffffu)); x[7] = bf2f((unsigned short)(v.w >> 16));
}

// One wave per row.  nck = ceil(V / 8) chunks hold live columns, ld / 8 chunks are written.
__global__ __launch_bounds__(MLM_THREADS) void mlm_ce_kernel(uint4* logits, int ldc, const int64_t* __restrict__ targets, int R, int V,
                                                             const int* __restrict__ n_valid, float* __restrict__ row_loss,
                                                             int* __restrict__ correct, unsigned* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * MLM_WAVES + (threadIdx.x >> 6);
    if (row >= R) return;   // wave-uniform, and no barrier follows
    uint4* p = logits + (size_t)row * ldc;
    const int nck = (V + 7) >> 3;
    const int64_t t64 = targets[row];
    const bool in_range = t64 >= 0 && t64 < (int64_t)V;
    if (!in_range) {
        if (t64 != (int64_t)CLIBD_MLM_IGNORE && err != nullptr && lane == 0) atomicOr(err, 1u);   // a flag: no order in it
        for (int c = lane; c < ldc; c += 64) p[c] = make_uint4(0u, 0u, 0u, 0u);
        if (lane == 0) row_loss[row] = 0.f;
        return;
    }
    const int tgt = (int)t64;
    const float NEG = -__builtin_huge_valf();
    // sweep 1: max, arg max, the target's logit
    float best = NEG, xt = NEG;
    int arg = 0x7fffffff;
    for (int c = lane; c < nck; c += 64) {
        float x[8];
        unpack8(p[c], x);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = 8 * c + e;
            if (col < V) {
                if (x[e] > best) {
                    best = x[e];
                    arg = col;
                }
                if (col == tgt) xt = x[e];
            }
        }
    }
    const float mx = wave_max(best);
    const float amin = -wave_max((best == mx && arg != 0x7fffffff) ? -(float)arg : NEG);   // columns < 8192 are exact in fp32
    xt = wave_max(xt);
    // sweep 2: sum of exp(x - max), the lane's chunks in ascending order, then the wave's fixed butterfly
    float sum = 0.f;
    for (int c = lane; c < nck; c += 64) {
        float x[8];
        unpack8(p[c], x);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (8 * c + e < V) sum += expf(x[e] - mx);
    }
    sum = wave_sum(sum);
    const float n = (float)max(n_valid[0], 1);
    if (lane == 0) {
        row_loss[row] = (logf(sum) + mx) - xt;
        if ((int)amin == tgt) atomicAdd(correct, 1);   // an integer count: no order in it
    }
    // sweep 3: the gradient over the logits
    for (int c = lane; c < ldc; c += 64) {
        float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (c < nck) {
            float x[8];
            unpack8(p[c], x);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int col = 8 * c + e;
                if (col < V) g[e] = (expf(x[e] - mx) / sum - (col == tgt ? 1.f : 0.f)) / n;
            }
        }
        p[c] = make_uint4(pack2bf(g[0], g[1]), pack2bf(g[2], g[3]), pack2bf(g[4], g[5]), pack2bf(g[6], g[7]));
    }
}

// loss[0] = (sum_i row_loss[i]) / max(n_valid, 1): thread t adds i = t, t + 256, ... in rising order, then the tree; one workgroup
__global__ __launch_bounds__(MLM_THREADS) void mlm_loss_kernel(const float* __restrict__ row_loss, int R, const int* __restrict__ n_valid,
                                                               float* __restrict__ loss) {
    __shared__ float part[MLM_THREADS];
    float s = 0.f;
    for (int i = threadIdx.x; i < R; i += MLM_THREADS) s += row_loss[i];
    s = block_tree_sum(s, part);
    if (threadIdx.x == 0) loss[0] = s / (float)max(n_valid[0], 1);
}

static inline bool aligned_to(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace clibd

using namespace clibd;

extern "C" int clibd_mlm_mask(const int64_t* ids, int B, int S, uint32_t seed, int n_mask, int64_t mask_id, int64_t unk_id, int64_t* masked,
                              int32_t* rows, int64_t* targets, int32_t* n_valid, void* stream) {
    if (!ids || !masked || !rows || !targets || !n_valid) return set_error(CLIBD_EINVAL, "mlm_mask: null pointer");
    if (B <= 0) return set_error(CLIBD_EINVAL, "mlm_mask: non-positive batch");
    if (S < 2 || S > MLM_MAX_S) return set_error(CLIBD_EINVAL, "mlm_mask: S must be in 2..256");
    if (n_mask < 1 || n_mask > S - 1) return set_error(CLIBD_EINVAL, "mlm_mask: n_mask must be in 1..S-1");
    if ((long long)B * S >= (1LL << 31)) return set_error(CLIBD_EINVAL, "mlm_mask: B * S must be below 2^31");
    if (!aligned_to(ids, 8) || !aligned_to(masked, 8) || !aligned_to(targets, 8) || !aligned_to(rows, 4) || !aligned_to(n_valid, 4))
        return set_error(CLIBD_EINVAL, "mlm_mask: misaligned pointer (int64 arrays 8 bytes, int32 arrays 4 bytes)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mlm_mask_kernel, dim3((unsigned)((B + MLM_WAVES - 1) / MLM_WAVES)), dim3(MLM_THREADS), 0, st, ids, B, S, (unsigned)seed, n_mask,
                       mask_id, unk_id, masked, rows, targets);
    if (int e = check_launch("mlm_mask")) return e;
    hipLaunchKernelGGL(mlm_count_valid_kernel, dim3(1), dim3(MLM_THREADS), 0, st, (const int64_t*)targets, B * n_mask, n_valid);
    return check_launch("mlm_mask (count)");
}

static int rows_check(const char* op, const void* a, const void* b, const int32_t* rows, int R, int M, int H) {
    if (!a || !b || !rows) return fail(op, "null pointer");
    if (R <= 0 || M <= 0 || H <= 0) return fail(op, "non-positive shape");
    if (H % 8 != 0) return fail(op, "H must be a multiple of 8");
    if (!aligned16(a) || !aligned16(b) || !aligned_to(rows, 4)) return fail(op, "misaligned pointer (matrices 16 bytes, rows 4 bytes)");
    if ((long long)M * (H / 8) >= (1LL << 31) || (long long)R * (H / 8) >= (1LL << 31)) return fail(op, "matrix too large (rows * H / 8 must be below 2^31)");
    return 0;
}

extern "C" int clibd_rows_gather_bf16(const void* x, int M, int H, const int32_t* rows, int R, void* out, void* stream) {
    if (int e = rows_check("rows_gather_bf16", x, out, rows, R, M, H)) return e;
    const int hc = H / 8;
    hipLaunchKernelGGL(rows_gather_kernel, dim3(grid_for((size_t)R * hc)), dim3(MLM_THREADS), 0, (hipStream_t)stream, (const uint4*)x, M, hc, rows, R,
                       (uint4*)out);
    return check_launch("rows_gather_bf16");
}

extern "C" int clibd_rows_scatter_bf16(const void* src, const int32_t* rows, int R, int M, int H, void* out, void* stream) {
    if (int e = rows_check("rows_scatter_bf16", src, out, rows, R, M, H)) return e;
    const int hc = H / 8;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rows_zero_kernel, dim3(grid_for((size_t)M * hc)), dim3(MLM_THREADS), 0, st, (uint4*)out, (long long)M * hc);
    if (int e = check_launch("rows_scatter_bf16 (zeros)")) return e;
    hipLaunchKernelGGL(rows_scatter_kernel, dim3(grid_for((size_t)R * hc)), dim3(MLM_THREADS), 0, st, (const uint4*)src, rows, R, M, hc, (uint4*)out);
    return check_launch("rows_scatter_bf16");
}

extern "C" int clibd_mlm_ce_bf16(void* logits, int ld, const int64_t* targets, int R, int V, const int32_t* n_valid, float* row_loss, float* loss,
                                 int32_t* correct, uint32_t* err, void* stream) {
    if (!logits || !targets || !n_valid || !row_loss || !loss || !correct) return set_error(CLIBD_EINVAL, "mlm_ce_bf16: null pointer");
    if (R <= 0 || V <= 0) return set_error(CLIBD_EINVAL, "mlm_ce_bf16: non-positive shape");
    if (V > MLM_MAX_V) return set_error(CLIBD_EINVAL, "mlm_ce_bf16: V must be at most 8192");
    if (ld < V || ld % 8 != 0) return set_error(CLIBD_EINVAL, "mlm_ce_bf16: ld must be >= V and a multiple of 8");
    if (!aligned16(logits) || !aligned_to(targets, 8) || !aligned_to(n_valid, 4) || !aligned_to(row_loss, 4) || !aligned_to(loss, 4) ||
        !aligned_to(correct, 4) || !aligned_to(err, 4))
        return set_error(CLIBD_EINVAL, "mlm_ce_bf16: misaligned pointer (logits 16 bytes, targets 8 bytes, the rest 4 bytes)");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(correct, 0, sizeof(int32_t), st) != hipSuccess) return set_error(CLIBD_ELAUNCH, "mlm_ce_bf16: memset failed");
    hipLaunchKernelGGL(mlm_ce_kernel, dim3((unsigned)((R + MLM_WAVES - 1) / MLM_WAVES)), dim3(MLM_THREADS), 0, st, (uint4*)logits, ld / 8, targets, R, V,
                       (const int*)n_valid, row_loss, (int*)correct, (unsigned*)err);
    if (int e = check_launch("mlm_ce_bf16")) return e;
    hipLaunchKernelGGL(mlm_loss_kernel, dim3(1), dim3(MLM_THREADS), 0, st, (const float*)row_loss, R, (const int*)n_valid, loss);
    return check_launch("mlm_ce_bf16 (loss)");
}
