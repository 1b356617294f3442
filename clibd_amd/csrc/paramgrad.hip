// Parameter gradients of the full fine-tune mode (model_config.disable_lora): everything the LoRA step never
// needs because the base encoders are frozen there.  Weight gradients dW = dY^T X go through the NT GEMM on transposed
// operands (host side: clibd_amd/engine.py::linear_wgrad); this file holds the reductions that are not GEMM-shaped:
//   * LayerNorm gamma / beta gradients (replaces autograd of nn.LayerNorm in timm Block / HF BertLayer),
//   * sums over the batch of a [B, R] fp32 tensor (position-embedding / class-token gradients),
//   * the scatter of the embedding gradient into the word / token-type tables (autograd of nn.Embedding),
//   * a row-range slice + bf16 cast (patch rows of the ViT token gradient, feeding the patch-embedding weight gradient).
// All outputs ACCUMULATE (atomicAdd) into fp32 buffers the caller zeroes once per step (the flat gradient bucket).
// Deterministic mode (the entry points called with a workspace): the same kernels store one partial per block into a caller-owned workspace
// (pointer variant: ws != nullptr) and ordered_colsum_kernel (gemm.hip) adds the partials in block order; the word-table scatter
// becomes a stable radix sort of (id, row) and fixed-order segment sums (embed_* kernels below).  No float atomics on that path.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "host_util.h"

namespace clibd {

__device__ __forceinline__ float ld_as_f32(const float* p) { return *p; }
__device__ __forceinline__ float ld_as_f32(const unsigned short* p) { return bf2f(*p); }

constexpr int PG_ROWS = 64;

// one block: PG_ROWS rows x all H columns (H <= 1024: up to 4 columns per thread); coalesced along columns
template <typename DY>
__global__ __launch_bounds__(256) void ln_param_grads_kernel(const DY* __restrict__ dy, int ld_dy, const float* __restrict__ x,
                                                             const float* __restrict__ stats, int M, int H,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta, unsigned drop_seed,
                                                             int drop_thr16, float drop_scale, float* __restrict__ ws) {
    float sg[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
    // chunks blockIdx.x, blockIdx.x + gridDim.x, ... (the atomic form launches one block per chunk)
    for (int r0 = blockIdx.x * PG_ROWS; r0 < M; r0 += gridDim.x * PG_ROWS)
    for (int r = r0, r1 = min(r0 + PG_ROWS, M); r < r1; ++r) {
        const float mean = stats[2 * r], rstd = stats[2 * r + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = threadIdx.x + 256 * j;
            if (c < H) {
                float g = ld_as_f32(dy + (size_t)r * ld_dy + c);
                if (drop_thr16 > 0) g *= drop_one(drop_seed, (unsigned)r * (unsigned)H + (unsigned)c, (unsigned)drop_thr16, drop_scale);
                sg[j] += g * ((x[(size_t)r * H + c] - mean) * rstd);
                sb[j] += g;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = threadIdx.x + 256 * j;
        if (c < H) {
            if (ws != nullptr) {
                ws[(size_t)blockIdx.x * 2 * H + c] = sg[j];
                ws[(size_t)blockIdx.x * 2 * H + H + c] = sb[j];
            } else {
                atomicAdd(dgamma + c, sg[j]);
                atomicAdd(dbeta + c, sb[j]);
            }
        }
    }
}

// out[r] += sum over b in this block's batch chunk of x[b, r]
// ws != nullptr: ws[chunk * R + r] = the chunk's sum instead (summed in chunk order by ordered_colsum_kernel)
__global__ __launch_bounds__(256) void batch_sum_kernel(const float* __restrict__ x, int B, size_t R, float* __restrict__ out, int bchunk,
                                                        float* __restrict__ ws) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int b0 = blockIdx.y * bchunk, b1 = min(b0 + bchunk, B);
    float s = 0.f;
    for (int b = b0; b < b1; ++b) s += x[(size_t)b * R + r];
    if (ws != nullptr) ws[(size_t)blockIdx.y * R + r] = s;
    else atomicAdd(out + r, s);
}

// word table: dword[ids[m], :] += de[m, :] (scatter);  token-type table (vocabulary 2, HF BERT): block-level partial sums
__global__ __launch_bounds__(256) void bert_embed_bwd_kernel(const long long* __restrict__ ids, const long long* __restrict__ tt,
                                                             const float* __restrict__ de, int M, int H, int vocab, int type_vocab,
                                                             float* __restrict__ dword, float* __restrict__ dtype, float* __restrict__ tt_ws) {
    float t0[4] = {0.f, 0.f, 0.f, 0.f}, t1[4] = {0.f, 0.f, 0.f, 0.f};
    // chunks blockIdx.x, blockIdx.x + gridDim.x, ... (the atomic form launches one block per chunk)
    for (int r0 = blockIdx.x * PG_ROWS; r0 < M; r0 += gridDim.x * PG_ROWS)
    for (int r = r0, r1 = min(r0 + PG_ROWS, M); r < r1; ++r) {
        long long id = ids[r];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        long long ty = tt ? tt[r] : 0;
        ty = ty < 0 ? 0 : (ty >= type_vocab ? type_vocab - 1 : ty);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = threadIdx.x + 256 * j;
            if (c < H) {
                const float g = de[(size_t)r * H + c];
                if (dword) atomicAdd(dword + (size_t)id * H + c, g);
                if (dtype) {
                    if (ty == 0) t0[j] += g;
                    else if (ty == 1) t1[j] += g;
                    else atomicAdd(dtype + (size_t)ty * H + c, g);
                }
            }
        }
    }
    if (dtype) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = threadIdx.x + 256 * j;
            if (c < H) {
                if (tt_ws != nullptr) {   // deterministic mode (type_vocab <= 2): the block's [type_vocab, H] partial
                    tt_ws[(size_t)blockIdx.x * type_vocab * H + c] = t0[j];
                    if (type_vocab > 1) tt_ws[(size_t)blockIdx.x * type_vocab * H + H + c] = t1[j];
                } else {
                    atomicAdd(dtype + c, t0[j]);
                    if (type_vocab > 1) atomicAdd(dtype + (size_t)H + c, t1[j]);
                }
            }
        }
    }
}

// ---- word-table gradient without float atomics (deterministic mode) ----------------------------------------------------------------------
// dword[v, :] += sum over the rows m with ids[m] == v, in increasing m, of de[m, :]  (the store-and-sum form of a scatter):
//   1. keys[m] = clamp(ids[m]), vals[m] = m;
//   2. a stable LSD radix sort of (key, row) on 8-bit digits (one pass per digit the vocabulary needs): per tile of EMB_TILE rows an
//      integer histogram (embed_hist_kernel), one exclusive scan over (digit, tile) (embed_scan_kernel), and a placement whose rank inside the
//      tile comes from wave ballots (embed_scatter_kernel) — equal keys keep their row order, nothing depends on timing;
//   3. the sorted rows are cut into chunks of EMB_CHUNK positions (a long list — every DNA sequence starts with id 0, text has long pad runs —
//      spans many chunks).  embed_chunk_sum_kernel walks each chunk in order: a key's run that lies inside one chunk is added to its table row
//      directly (no other writer); the piece of a run that starts in an earlier chunk goes to head[chunk], the first piece of a run that
//      continues past its chunk to own[chunk].  embed_join_kernel then adds own[k] + head[k+1] + ... + head[last] in chunk order for every
//      run that crosses a chunk boundary.
constexpr int EMB_TILE = 1024;    // rows per tile of the sort: 256 threads x 4
constexpr int EMB_CHUNK = 128;    // sorted positions per chunk of the sums

__global__ __launch_bounds__(256) void embed_keys_kernel(const long long* __restrict__ ids, int M, int vocab, int* __restrict__ keys, int* __restrict__ vals) {
    for (int m = blockIdx.x * 256 + threadIdx.x; m < M; m += gridDim.x * 256) {
        long long id = ids[m];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        keys[m] = (int)id;
        vals[m] = m;
    }
}

// hist[d * ntiles + tile] = number of rows of the tile whose digit is d (integer counts: exact in any order)
__global__ __launch_bounds__(256) void embed_hist_kernel(const int* __restrict__ keys, int M, int shift, int ntiles, int* __restrict__ hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * EMB_TILE;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < M) atomicAdd(&h[(keys[i] >> shift) & 255], 1);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of n ints in place, one block of 1024 threads: each thread owns a contiguous segment
__global__ __launch_bounds__(1024) void embed_scan_kernel(int* __restrict__ a, int n) {
    __shared__ int tot[1024];
    const int t = threadIdx.x;
    const int seg = (n + 1023) / 1024;
    const int i0 = min(t * seg, n), i1 = min(i0 + seg, n);
    int s = 0;
    for (int i = i0; i < i1; ++i) s += a[i];
    tot[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // inclusive Hillis-Steele scan of the segment totals
        const int v = t >= off ? tot[t - off] : 0;
        __syncthreads();
        tot[t] += v;
        __syncthreads();
    }
    int run = tot[t] - s;
    for (int i = i0; i < i1; ++i) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
}

// stable placement: row i of tile b goes to off[d * ntiles + b] + (rows before i in the tile with the same digit d)
__global__ __launch_bounds__(256) void embed_scatter_kernel(const int* __restrict__ keys_in, const int* __restrict__ vals_in, int M, int shift, int ntiles,
                                                            const int* __restrict__ off, int* __restrict__ keys_out, int* __restrict__ vals_out) {
    __shared__ int wh[16][256];   // per 64-row group of the tile: count of each digit
    for (int i = threadIdx.x; i < 16 * 256; i += 256) (&wh[0][0])[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int key[4], val[4], d[4], rin[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * EMB_TILE + k * 256 + threadIdx.x;
        const bool ok = i < M;
        key[k] = ok ? keys_in[i] : 0;
        val[k] = ok ? vals_in[i] : 0;
        d[k] = ok ? ((key[k] >> shift) & 255) : 256;   // (256: no digit, matches only other out-of-range lanes)
        unsigned long long same = ~0ull;
#pragma unroll
        for (int bit = 0; bit < 9; ++bit) {
            const unsigned long long b = __ballot((d[k] >> bit) & 1);
            same &= ((d[k] >> bit) & 1) ? b : ~b;
        }
        rin[k] = __popcll(same & lt);
        const int grp = k * 4 + (threadIdx.x >> 6);   // 64-row group index inside the tile, in row order
        if (ok && rin[k] == 0) wh[grp][d[k]] = __popcll(same);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * EMB_TILE + k * 256 + threadIdx.x;
        if (i >= M) continue;
        const int grp = k * 4 + (threadIdx.x >> 6);
        int r = rin[k];
        for (int g = 0; g < grp; ++g) r += wh[g][d[k]];
        const int pos = off[(size_t)d[k] * ntiles + blockIdx.x] + r;
        keys_out[pos] = key[k];
        vals_out[pos] = val[k];
    }
}

// one block per chunk of EMB_CHUNK sorted positions; thread owns columns threadIdx.x + 256 j (H <= 1024)
__global__ __launch_bounds__(256) void embed_chunk_sum_kernel(const int* __restrict__ skeys, const int* __restrict__ svals, const float* __restrict__ de,
                                                              int M, int H, float* __restrict__ dword, float* __restrict__ head, float* __restrict__ own) {
    __shared__ int kk[EMB_CHUNK], vv[EMB_CHUNK];
    const int p0 = blockIdx.x * EMB_CHUNK, p1 = min(p0 + EMB_CHUNK, M), n = p1 - p0;
    for (int i = threadIdx.x; i < n; i += 256) { kk[i] = skeys[p0 + i]; vv[i] = svals[p0 + i]; }
    __syncthreads();
    const int prev = p0 > 0 ? skeys[p0 - 1] : -1, next = p1 < M ? skeys[p1] : -1;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int start = 0;
    for (int i0 = 0; i0 < n; i0 += 8) {
        float v[8][4];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = threadIdx.x + 256 * j;
                v[u][j] = (i0 + u < n && c < H) ? de[(size_t)vv[i0 + u] * H + c] : 0.f;
            }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u;
            if (i >= n) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += v[u][j];
            const int key = kk[i];
            if (i + 1 < n && kk[i + 1] == key) continue;
            // run [start, i] of key ends here (inside the chunk or at its end)
            float* dst;
            if (start == 0 && prev == key) dst = head + (size_t)blockIdx.x * H;            // continues a run from an earlier chunk
            else if (i == n - 1 && next == key) dst = own + (size_t)blockIdx.x * H;       // first piece of a run that crosses the chunk end
            else dst = nullptr;                                                            // the whole run: its table row has no other writer
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = threadIdx.x + 256 * j;
                if (c < H) {
                    if (dst != nullptr) dst[c] = acc[j];
                    else dword[(size_t)key * H + c] += acc[j];
                }
                acc[j] = 0.f;
            }
            start = i + 1;
        }
    }
}

// runs that cross chunk boundaries: the chunk where the run starts adds own[k] + head[k+1] + ... in chunk order
__global__ __launch_bounds__(256) void embed_join_kernel(const int* __restrict__ skeys, int M, int H, const float* __restrict__ head,
                                                         const float* __restrict__ own, float* __restrict__ dword) {
    const int k = blockIdx.x;
    const int p0 = k * EMB_CHUNK, p1 = min(p0 + EMB_CHUNK, M);
    if (p1 >= M) return;
    const int key = skeys[p1 - 1];
    if (skeys[p1] != key || (p0 > 0 && skeys[p0 - 1] == key)) return;   // not a crossing run, or not its first chunk
    int lo = p1, hi = M;   // first position after the run (keys are sorted)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (skeys[mid] == key) lo = mid + 1;
        else hi = mid;
    }
    const int klast = (lo - 1) / EMB_CHUNK;
    for (int j = 0; j < 4; ++j) {
        const int c = threadIdx.x + 256 * j;
        if (c >= H) break;
        float s = own[(size_t)k * H + c];
        int q = k + 1;
        for (; q + 8 <= klast + 1; q += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = head[(size_t)(q + u) * H + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; q <= klast; ++q) s += head[(size_t)q * H + c];
        dword[(size_t)key * H + c] += s;
    }
}

// out[b * (s1 - s0) + (s - s0), :] = bf16(x[b, s, :]) for s in [s0, s1)
__global__ __launch_bounds__(256) void slice_rows_cast_kernel(const float* __restrict__ x, int B, int S, int H, int s0, int s1,
                                                              unsigned short* __restrict__ out) {
    const int ns = s1 - s0;
    const size_t total = (size_t)B * ns * (H / 2);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int hp = (int)(i % (H / 2));
        const size_t row = i / (H / 2);
        const int b = (int)(row / ns), s = (int)(row % ns) + s0;
        const float2 v = *(const float2*)(x + ((size_t)b * S + s) * H + 2 * hp);
        *(unsigned*)(out + row * H + 2 * hp) = pack2bf(v.x, v.y);
    }
}

// y[i] = x[i] * dropout_factor(seed, i): the gradient through y = dropout(.) of an [M,H] activation (element index row*H+col)
__global__ __launch_bounds__(256) void dropout_apply_kernel(const float* __restrict__ x, size_t n, float* __restrict__ y, unsigned seed,
                                                            unsigned thr16, float scale) {
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; i < n; i += (size_t)gridDim.x * blockDim.x * 2) {
        float f0, f1;
        drop_pair(seed, (unsigned)i, thr16, scale, f0, f1);
        y[i] = x[i] * f0;
        if (i + 1 < n) y[i + 1] = x[i + 1] * f1;
    }
}

}  // namespace clibd

using namespace clibd;

// ---- the reductions: one entry point each.  NULL workspace: float atomics; with a workspace (deterministic mode, see the header of this
// file) the same kernel stores one partial per block / chunk and ordered_colsum_kernel adds them in a fixed order.
constexpr int PG_ORDERED_BLOCKS = 1024;   // cap of the partial count of the row-chunk kernels (grid-stride beyond it)
constexpr int TT_ORDERED_BLOCKS = 512;
// blocks of a row-chunk kernel: one per PG_ROWS rows in the atomic form, capped where every block owns a workspace row
static inline int row_chunk_blocks(int M, bool ws, int cap) {
    const int blocks = (M + PG_ROWS - 1) / PG_ROWS;
    return ws ? min(blocks, cap) : blocks;
}

extern "C" size_t clibd_layernorm_param_grads_workspace_bytes(int M, int H) {
    if (M <= 0 || H <= 0) return 0;
    return (size_t)row_chunk_blocks(M, true, PG_ORDERED_BLOCKS) * 2 * (size_t)H * sizeof(float);
}

extern "C" int clibd_layernorm_param_grads(const void* dy, int dy_is_f32, int ld_dy, const float* x, const float* stats, int M, int H,
                                           float* dgamma, float* dbeta, uint32_t drop_seed, int drop_thr16, float drop_scale,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !x || !stats || !dgamma || !dbeta) return set_error(CLIBD_EINVAL, "layernorm_param_grads: null pointer");
    if (M <= 0 || H <= 0 || H > 1024 || ld_dy < H) return set_error(CLIBD_EINVAL, "layernorm_param_grads: bad shape (H <= 1024)");
    if (int e = check_workspace("layernorm_param_grads", "workspace", workspace, workspace_bytes, clibd_layernorm_param_grads_workspace_bytes(M, H),
                                "clibd_layernorm_param_grads_workspace_bytes"))
        return e;
    float* ws = (float*)workspace;
    const int blocks = row_chunk_blocks(M, ws != nullptr, PG_ORDERED_BLOCKS);
    if (dy_is_f32)
        hipLaunchKernelGGL(ln_param_grads_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float*)dy, ld_dy, x, stats, M, H,
                           dgamma, dbeta, drop_seed, drop_thr16, drop_scale, ws);
    else
        hipLaunchKernelGGL(ln_param_grads_kernel<unsigned short>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)dy, ld_dy, x,
                           stats, M, H, dgamma, dbeta, drop_seed, drop_thr16, drop_scale, ws);
    if (int e = check_launch("layernorm_param_grads")) return e;
    return ws ? ordered_colsum_launch(ws, blocks, 2 * H, dgamma, H, dbeta, (hipStream_t)stream) : CLIBD_OK;
}

static inline int batch_chunks(int B) { return B >= 64 ? 8 : 1; }

extern "C" size_t clibd_batch_sum_workspace_bytes(int B, size_t R) {
    if (B <= 0 || R == 0) return 0;
    return (size_t)batch_chunks(B) * R * sizeof(float);
}

extern "C" int clibd_batch_sum_f32(const float* x, int B, size_t R, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !out || B <= 0 || R == 0) return set_error(CLIBD_EINVAL, "batch_sum: bad args");
    // the grid's x dimension in both forms; the fixed-order second kernel takes R as an int
    if ((workspace ? R : (R + 255) / 256) > 0x7fffffffull) return set_error(CLIBD_EINVAL, "batch_sum: R too large");
    if (int e = check_workspace("batch_sum", "workspace", workspace, workspace_bytes, clibd_batch_sum_workspace_bytes(B, R), "clibd_batch_sum_workspace_bytes"))
        return e;
    const int chunks = batch_chunks(B);
    const int bchunk = (B + chunks - 1) / chunks;
    const int nchunk = (B + bchunk - 1) / bchunk;
    hipLaunchKernelGGL(batch_sum_kernel, dim3((unsigned)((R + 255) / 256), (unsigned)nchunk), dim3(256), 0, (hipStream_t)stream, x, B, R, out, bchunk,
                       (float*)workspace);
    if (int e = check_launch("batch_sum")) return e;
    return workspace ? ordered_colsum_launch((const float*)workspace, nchunk, (int)R, out, (int)R, nullptr, (hipStream_t)stream) : CLIBD_OK;
}

struct EmbedWs { int *ka, *va, *kb, *vb, *hist; float *head, *own, *tt; size_t bytes; };
static EmbedWs embed_ws_layout(char* base, int M, int H, int type_vocab) {
    const int ntiles = (M + EMB_TILE - 1) / EMB_TILE, nchunks = (M + EMB_CHUNK - 1) / EMB_CHUNK;
    const int ttb = row_chunk_blocks(M, true, TT_ORDERED_BLOCKS);
    EmbedWs w{};
    Carver c(base);
    w.ka = c.take<int>(M); w.va = c.take<int>(M);
    w.kb = c.take<int>(M); w.vb = c.take<int>(M);
    w.hist = c.take<int>((size_t)256 * ntiles);
    w.head = c.take<float>((size_t)nchunks * H); w.own = c.take<float>((size_t)nchunks * H);
    w.tt = c.take<float>((size_t)ttb * type_vocab * H);
    w.bytes = c.total();
    return w;
}

extern "C" size_t clibd_bert_embed_bwd_workspace_bytes(int M, int H, int vocab, int type_vocab) {
    if (M <= 0 || H <= 0 || vocab <= 0 || type_vocab <= 0) return 0;
    return embed_ws_layout(nullptr, M, H, type_vocab).bytes;
}

extern "C" int clibd_bert_embed_bwd(const int64_t* ids, const int64_t* token_type, const float* de, int M, int H, int vocab, int type_vocab,
                                    float* dword, float* dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ids || !de || (!dword && !dtype)) return set_error(CLIBD_EINVAL, "bert_embed_bwd: null pointer");
    if (M <= 0 || H <= 0 || H > 1024 || vocab <= 0 || type_vocab <= 0) return set_error(CLIBD_EINVAL, "bert_embed_bwd: bad shape (H <= 1024)");
    if (workspace && (vocab > (1 << 24) || type_vocab > 2))
        return set_error(CLIBD_EINVAL, "bert_embed_bwd: with a workspace, vocabulary <= 2^24 and at most two token types");
    if (int e = check_workspace("bert_embed_bwd", "workspace", workspace, workspace_bytes, clibd_bert_embed_bwd_workspace_bytes(M, H, vocab, type_vocab),
                                "clibd_bert_embed_bwd_workspace_bytes"))
        return e;
    hipStream_t st = (hipStream_t)stream;
    if (!workspace) {   // both tables in one pass, float atomics
        hipLaunchKernelGGL(bert_embed_bwd_kernel, dim3(row_chunk_blocks(M, false, 0)), dim3(256), 0, st, (const long long*)ids,
                           (const long long*)token_type, de, M, H, vocab, type_vocab, dword, dtype, (float*)nullptr);
        return check_launch("bert_embed_bwd");
    }
    EmbedWs w = embed_ws_layout((char*)workspace, M, H, type_vocab);
    if (dtype) {
        const int ttb = row_chunk_blocks(M, true, TT_ORDERED_BLOCKS);
        hipLaunchKernelGGL(bert_embed_bwd_kernel, dim3(ttb), dim3(256), 0, st, (const long long*)ids, (const long long*)token_type, de, M, H, vocab,
                           type_vocab, (float*)nullptr, dtype, w.tt);
        if (int e = check_launch("bert_embed_bwd (token types)")) return e;
        if (int e = ordered_colsum_launch(w.tt, ttb, type_vocab * H, dtype, type_vocab * H, nullptr, st)) return e;
    }
    if (!dword) return CLIBD_OK;
    const int ntiles = (M + EMB_TILE - 1) / EMB_TILE, nchunks = (M + EMB_CHUNK - 1) / EMB_CHUNK;
    hipLaunchKernelGGL(embed_keys_kernel, dim3(grid_for((size_t)M)), dim3(256), 0, st, (const long long*)ids, M, vocab, w.ka, w.va);
    int *kin = w.ka, *vin = w.va, *kout = w.kb, *vout = w.vb;
    for (int shift = 0; (vocab - 1) >> shift > 0 || shift == 0; shift += 8) {
        hipLaunchKernelGGL(embed_hist_kernel, dim3(ntiles), dim3(256), 0, st, kin, M, shift, ntiles, w.hist);
        hipLaunchKernelGGL(embed_scan_kernel, dim3(1), dim3(1024), 0, st, w.hist, 256 * ntiles);
        hipLaunchKernelGGL(embed_scatter_kernel, dim3(ntiles), dim3(256), 0, st, kin, vin, M, shift, ntiles, w.hist, kout, vout);
        int* t = kin; kin = kout; kout = t;
        t = vin; vin = vout; vout = t;
    }
    if (int e = check_launch("bert_embed_bwd (sort)")) return e;
    hipLaunchKernelGGL(embed_chunk_sum_kernel, dim3(nchunks), dim3(256), 0, st, kin, vin, de, M, H, dword, w.head, w.own);
    hipLaunchKernelGGL(embed_join_kernel, dim3(nchunks), dim3(256), 0, st, kin, M, H, w.head, w.own, dword);
    return check_launch("bert_embed_bwd (sums)");
}

extern "C" int clibd_slice_rows_cast_bf16(const float* x, int B, int S, int H, int s0, int s1, void* out, void* stream) {
    if (!x || !out || B <= 0 || S <= 0 || H <= 0 || (H & 1) || s0 < 0 || s1 > S || s0 >= s1) return set_error(CLIBD_EINVAL, "slice_rows_cast: bad args");
    if (!aligned16(x) || !aligned16(out)) return set_error(CLIBD_EINVAL, "slice_rows_cast: alignment");
    hipLaunchKernelGGL(slice_rows_cast_kernel, dim3(grid_for((size_t)B * (s1 - s0) * (H / 2))), dim3(256), 0, (hipStream_t)stream, x, B, S, H,
                       s0, s1, (unsigned short*)out);
    return check_launch("slice_rows_cast");
}

extern "C" int clibd_dropout_apply_f32(const float* x, size_t n, float* y, uint32_t drop_seed, int drop_thr16, float drop_scale, void* stream) {
    if (!x || !y || n == 0 || n >= (1ull << 32)) return set_error(CLIBD_EINVAL, "dropout_apply: bad args (n < 2^32)");
    if (drop_thr16 < 0 || drop_thr16 > 65535) return set_error(CLIBD_EINVAL, "dropout_apply: bad dropout threshold");
    hipLaunchKernelGGL(dropout_apply_kernel, dim3(grid_for((n + 1) / 2)), dim3(256), 0, (hipStream_t)stream, x, n, y, drop_seed,
                       (unsigned)drop_thr16, drop_scale);
    return check_launch("dropout_apply");
}
