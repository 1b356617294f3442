// Embedding analysis (reference: scripts/result/distribution_of_similarities.py, scripts/result/create_confusion_matrix.py) for gfx950:
// sklearn's silhouette_samples for one labelling, the distance from each query to the nearest key of its own class, and the counts of a
// confusion matrix.
//
// Silhouette.  X [N, D] arrives with every cluster one contiguous run (seg[C + 1] the run offsets).  d(i, j) comes from the Gram form
// |x_i|^2 + |x_j|^2 - 2 x_i.x_j, which cancels, so the product runs on the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact f32 operands, an
// fp32 fma chain over k) and the norms are the SAME fma chain of a row with itself (row_norms_kernel walks k in the MFMA's order), so two
// identical rows are at distance exactly 0.  Neither the N x N distances nor N x C cluster sums exist in memory: a workgroup owns one
// (128-row tile, column chunk) pair, forms 128 x 128 distances at a time in LDS, and one thread per row walks the tile's columns in
// order with a running sum of the segment it is in.  A segment that lies strictly inside the chunk is folded at once into the row's
// min-of-means or its own-cluster sum; the chunk's first and last segment (which may continue in the neighbouring chunks) leave their
// partial sums in the workspace as "head" and "tail", and silhouette_finalize_kernel walks a row's chunks in order, stitches tail with
// head, and forms a, b and s.  Every sum has one order; no float atomics.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_analysis.h"
#include "host_util.h"

namespace clibd {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int SIL_TILE = 128;      // rows per workgroup and columns per distance tile
constexpr int SIL_BK = 32;         // the K-step: D must be a multiple of it
constexpr int SIL_LDT = 36;        // LDS row stride of a staged [128, 32] operand tile (floats): 16-byte aligned rows
constexpr int SIL_CHUNK_UNIT = 64; // col_chunk is a multiple of this
constexpr int SIL_DEFAULT_CHUNK = 1024;
constexpr int SIL_MAX_N = 1 << 24;

// cid[i] = the cluster of row i
__global__ __launch_bounds__(256) void seg_to_cid_kernel(const int* __restrict__ seg, int C, int N, int* __restrict__ cid) {
    for (int c = blockIdx.x; c < C; c += gridDim.x) {
        int b = seg[c], e = seg[c + 1];
        b = b < 0 ? 0 : b;
        e = e > N ? N : e;   // (validated on the host; the clamp keeps a wrong device copy inside the buffer)
        for (int i = b + threadIdx.x; i < e; i += 256) cid[i] = c;
    }
}

// nrm[i] = x_i . x_i as the fma chain the MFMA runs for the pair (i, i): within each K-step of 32 the order is k = 0, 16, 1, 17, ...
__global__ __launch_bounds__(256) void row_norms_kernel(const float* __restrict__ X, int N, int D, float* __restrict__ nrm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* x = X + (size_t)i * D;
    float acc = 0.f;
    for (int k0 = 0; k0 < D; k0 += SIL_BK) {
        float v[SIL_BK];
#pragma unroll
        for (int q = 0; q < SIL_BK / 4; ++q) {
            const float4 t = *(const float4*)(x + k0 + 4 * q);
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
#pragma unroll
        for (int s = 0; s < SIL_BK / 2; ++s) {
            acc = __builtin_fmaf(v[s], v[s], acc);
            acc = __builtin_fmaf(v[s + 16], v[s + 16], acc);
        }
    }
    nrm[i] = acc;
}

// One workgroup = rows [128 by, 128 by + 128) x columns [chunk bx).  part is [nchunk][4][N]: head, tail, min of the folded means, the
// folded own-cluster sum.
__global__ __launch_bounds__(256, 2) void silhouette_tile_kernel(const float* __restrict__ X, int N, int D, const int* __restrict__ seg,
                                                                  const int* __restrict__ cid, const float* __restrict__ nrm, int col_chunk,
                                                                  float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float smem[SIL_TILE * SIL_TILE];   // the staged operands, then the distance tile [col][row]
    __shared__ int s_ccid[SIL_TILE];
    __shared__ int s_csz[SIL_TILE];
    __shared__ float s_nq[SIL_TILE];
    __shared__ float s_nk[SIL_TILE];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wq = (w >> 1) * 64, wk = (w & 1) * 64;
    const int row0 = blockIdx.y * SIL_TILE;
    const int chunk = blockIdx.x;
    const int c0 = chunk * col_chunk;
    const int cend = min(c0 + col_chunk, N);
    float* sQ = smem;
    float* sK = smem + SIL_TILE * SIL_LDT;

    // the scanning thread's state (threads 0..127: one row each)
    const int my_row = row0 + tid;
    const bool scans = tid < SIL_TILE && my_row < N;
    const int my = scans ? cid[my_row] : -1;
    const int first = cid[c0];
    int cur = first, cursz = 1;
    float run = 0.f, head = 0.f, tail = 0.f, bmin = __builtin_huge_valf(), own = 0.f;
    if (tid < SIL_TILE) s_nq[tid] = my_row < N ? nrm[my_row] : 0.f;

    for (int kc0 = c0; kc0 < cend; kc0 += SIL_TILE) {
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        float4 gq[4], gk[4];
        auto gload = [&](int k0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = tid + 256 * u, r = idx >> 3, c4 = idx & 7;
                const int qr = row0 + r, kr = kc0 + r;
                gq[u] = qr < N ? *(const float4*)(X + (size_t)qr * D + k0 + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
                gk[u] = kr < cend ? *(const float4*)(X + (size_t)kr * D + k0 + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        gload(0);
        for (int k0 = 0; k0 < D; k0 += SIL_BK) {
            __syncthreads();   // the previous step's fragment reads (or the previous tile's scan) are done with smem
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = tid + 256 * u, r = idx >> 3, c4 = idx & 7;
                *(float4*)(sQ + r * SIL_LDT + 4 * c4) = gq[u];
                *(float4*)(sK + r * SIL_LDT + 4 * c4) = gk[u];
            }
            __syncthreads();
            if (k0 + SIL_BK < D) gload(k0 + SIL_BK);
            float fq[2][16], fk[2][16];
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 tq = *(const float4*)(sQ + (wq + 32 * b + l31) * SIL_LDT + 16 * h + 4 * q);
                    const float4 tk = *(const float4*)(sK + (wk + 32 * b + l31) * SIL_LDT + 16 * h + 4 * q);
                    fq[b][4 * q] = tq.x; fq[b][4 * q + 1] = tq.y; fq[b][4 * q + 2] = tq.z; fq[b][4 * q + 3] = tq.w;
                    fk[b][4 * q] = tk.x; fk[b][4 * q + 1] = tk.y; fk[b][4 * q + 2] = tk.z; fk[b][4 * q + 3] = tk.w;
                }
            // D[i = key][j = query]: lane half h supplies k = 16 h + s of this K-step (the same relabelling on both operands)
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fk[a][s], fq[b][s], acc[a][b], 0, 0, 0);
        }
        if (tid < SIL_TILE) {
            const int gc = kc0 + tid;
            int c = 0, sz = 1;
            float nk = 0.f;
            if (gc < cend) {
                c = cid[gc];
                sz = seg[c + 1] - seg[c];
                nk = nrm[gc];
            }
            s_ccid[tid] = c;
            s_csz[tid] = sz;
            s_nk[tid] = nk;
        }
        __syncthreads();   // every wave is done with the staged operands; the norms and column tables are visible
        // distances into smem[key][query]: the lane owns query column l31 of its blocks, the registers walk the keys
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int q = wq + 32 * b + l31;
                const float nq = s_nq[q];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = wk + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float d2 = (nq + s_nk[k]) - 2.0f * acc[a][b][r];
                    float d = __builtin_sqrtf(fmaxf(d2, 0.f));
                    if (row0 + q == kc0 + k) d = 0.f;   // sklearn forces the diagonal
                    smem[k * SIL_TILE + q] = d;
                }
            }
        __syncthreads();
        if (scans) {
            const int ncol = min(SIL_TILE, cend - kc0);
            float t = 0.f;   // this tile's share of the open segment: the sums are blocked by tile
            for (int c = 0; c < ncol; ++c) {
                const int sc = s_ccid[c];
                if (sc != cur) {
                    const float total = run + t;
                    if (cur == first) head = total;
                    else if (cur == my) own = total;
                    else bmin = fminf(bmin, total / (float)cursz);
                    cur = sc;
                    run = 0.f;
                    t = 0.f;
                }
                cursz = s_csz[c];
                t += smem[c * SIL_TILE + tid];
            }
            run += t;
        }
    }
    if (scans) {
        if (cur == first) head = run;
        else tail = run;
        float* p = part + (size_t)chunk * 4 * N + my_row;
        p[0] = head;
        p[(size_t)N] = tail;
        p[2 * (size_t)N] = bmin;
        p[3 * (size_t)N] = own;
    }
}

// one thread per row: the chunks in order
__global__ __launch_bounds__(256) void silhouette_finalize_kernel(const float* __restrict__ part, const int* __restrict__ seg,
                                                                  const int* __restrict__ cid, int N, int col_chunk, int nchunk,
                                                                  float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int my = cid[i];
    const int n_own = seg[my + 1] - seg[my];
    float bmin = __builtin_huge_valf(), own = 0.f, run = 0.f;
    int cur = -1;
    auto close = [&]() {
        if (cur < 0) return;
        if (cur == my) own = run;
        else bmin = fminf(bmin, run / (float)(seg[cur + 1] - seg[cur]));
    };
    for (int k = 0; k < nchunk; ++k) {
        const int c0 = k * col_chunk, cend = min(c0 + col_chunk, N);
        const int first = cid[c0], last = cid[cend - 1];
        const float* p = part + (size_t)k * 4 * N + i;
        if (first == cur) run += p[0];
        else {
            close();
            cur = first;
            run = p[0];
        }
        bmin = fminf(bmin, p[2 * (size_t)N]);
        if (first < my && my < last) own = p[3 * (size_t)N];
        if (last != first) {
            close();
            cur = last;
            run = p[(size_t)N];
        }
    }
    close();
    float s = 0.f;
    if (n_own > 1) {
        const float a = own / (float)(n_own - 1);
        const float m = fmaxf(a, bmin);
        s = m > 0.f ? (bmin - a) / m : 0.f;
    }
    out[i] = s;
}

// one wave per query: the keys of its class in ascending order, each distance one wave reduction of the lanes' strided shares
__global__ __launch_bounds__(256) void same_label_nearest_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk,
                                                                 int Nq, int Nk, int D, const int* __restrict__ seg, int C,
                                                                 const int* __restrict__ qclass, float* __restrict__ dist, int* __restrict__ arg) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Nq) return;
    float best = __builtin_huge_valf();
    int barg = -1;
    const int c = qclass[q];
    if (c >= 0 && c < C) {
        int b = seg[c], e = seg[c + 1];
        b = b < 0 ? 0 : b;
        e = e > Nk ? Nk : e;
        const float* qr = Q + (size_t)q * ldq;
        for (int j = b; j < e; ++j) {
            const float* kr = K + (size_t)j * ldk;
            float s = 0.f;
            for (int t = lane; t < D; t += 64) {
                const float df = qr[t] - kr[t];
                s = __builtin_fmaf(df, df, s);
            }
            s = wave_sum(s);
            if (s < best) {   // ties keep the lower key index
                best = s;
                barg = j;
            }
        }
    }
    if (lane == 0) {
        dist[q] = barg >= 0 ? __builtin_sqrtf(best) : __builtin_huge_valf();
        arg[q] = barg;
    }
}

__global__ __launch_bounds__(256) void zero_i32_kernel(int* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0;
}

__global__ __launch_bounds__(256) void confusion_counts_kernel(const int* __restrict__ t, const int* __restrict__ p, size_t n, int C,
                                                               int* __restrict__ counts) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int a = t[i], b = p[i];
        if (a >= 0 && a < C && b >= 0 && b < C) atomicAdd(counts + (size_t)a * C + b, 1);   // integer: the order does not matter
    }
}

struct SilWs {
    int* cid;
    float *nrm, *part;
    size_t total;
};

static int sil_chunk(int col_chunk) { return col_chunk == 0 ? SIL_DEFAULT_CHUNK : col_chunk; }
static int sil_nchunk(int N, int cc) { return (int)(((long long)N + cc - 1) / cc); }

static SilWs sil_carve(void* base, int N, int cc) {
    SilWs w;
    Carver c(base);
    w.cid = c.take<int>(N);
    w.nrm = c.take<float>(N);
    w.part = c.take<float>((size_t)sil_nchunk(N, cc) * 4 * (size_t)N);
    w.total = c.total();
    return w;
}

static bool chunk_ok(int col_chunk) { return col_chunk >= 0 && col_chunk % SIL_CHUNK_UNIT == 0; }

// seg_host[0] = 0 < seg_host[1] < ... < seg_host[C] = n
static bool seg_ok(const int32_t* s, int C, int n, bool strict) {
    if (s[0] != 0 || s[C] != n) return false;
    for (int c = 0; c < C; ++c)
        if (strict ? s[c + 1] <= s[c] : s[c + 1] < s[c]) return false;
    return true;
}

}  // namespace clibd

using namespace clibd;

extern "C" size_t clibd_silhouette_workspace_bytes(int N, int col_chunk) {
    if (N <= 0 || N > SIL_MAX_N || !chunk_ok(col_chunk)) return 0;
    return sil_carve(nullptr, N, sil_chunk(col_chunk)).total;
}

extern "C" int clibd_silhouette_samples(const float* X, int N, int D, const int32_t* seg, const int32_t* seg_host, int C, int col_chunk,
                                        float* s, void* workspace, size_t workspace_bytes, void* stream) {
    if (!X || !seg || !seg_host || !s || !workspace) return set_error(CLIBD_EINVAL, "silhouette_samples: null pointer");
    if (N < 3 || N > SIL_MAX_N) return set_error(CLIBD_EINVAL, "silhouette_samples: N must be in 3..2^24");
    if (C < 2 || C > N - 1)
        return set_error(CLIBD_EINVAL, "silhouette_samples: number of clusters must be in 2..N-1 (Valid values are 2 to n_samples - 1 (inclusive))");
    if (D <= 0 || D % SIL_BK != 0) return set_error(CLIBD_EINVAL, "silhouette_samples: D must be a positive multiple of 32 (zero pad it)");
    if (!chunk_ok(col_chunk)) return set_error(CLIBD_EINVAL, "silhouette_samples: col_chunk must be 0 or a positive multiple of 64");
    if (!aligned16(X)) return set_error(CLIBD_EINVAL, "silhouette_samples: X must be 16-byte aligned");
    if (!seg_ok(seg_host, C, N, true))
        return set_error(CLIBD_EINVAL, "silhouette_samples: seg must rise strictly from 0 to N (rows sorted by cluster, no empty cluster)");
    const int cc = sil_chunk(col_chunk);
    const SilWs ws = sil_carve(workspace, N, cc);
    if (!aligned16(workspace) || workspace_bytes < ws.total)
        return set_error(CLIBD_EINVAL, "silhouette_samples: workspace too small or misaligned (clibd_silhouette_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const int nchunk = sil_nchunk(N, cc);
    // every later index into seg comes from cid: keep it a valid cluster even if the device copy of seg disagrees with the host's
    if (hipMemsetAsync(ws.cid, 0, (size_t)N * 4, st) != hipSuccess) return set_error(CLIBD_ELAUNCH, "silhouette_samples: memset failed");
    hipLaunchKernelGGL(seg_to_cid_kernel, dim3(C < 4096 ? C : 4096), dim3(256), 0, st, seg, C, N, ws.cid);
    hipLaunchKernelGGL(row_norms_kernel, dim3((N + 255) / 256), dim3(256), 0, st, X, N, D, ws.nrm);
    if (int e = check_launch("silhouette_samples prepare")) return e;
    hipLaunchKernelGGL(silhouette_tile_kernel, dim3(nchunk, (N + SIL_TILE - 1) / SIL_TILE), dim3(256), 0, st, X, N, D, seg, ws.cid, ws.nrm, cc,
                       ws.part);
    if (int e = check_launch("silhouette_samples tiles")) return e;
    hipLaunchKernelGGL(silhouette_finalize_kernel, dim3((N + 255) / 256), dim3(256), 0, st, ws.part, seg, ws.cid, N, cc, nchunk, s);
    return check_launch("silhouette_samples finalize");
}

extern "C" int clibd_same_label_nearest(const float* Q, int ldq, const float* K, int ldk, int Nq, int Nk, int D, const int32_t* seg,
                                        const int32_t* seg_host, int C, const int32_t* qclass, float* dist, int32_t* arg, void* stream) {
    if (!Q || !K || !seg || !seg_host || !qclass || !dist || !arg) return set_error(CLIBD_EINVAL, "same_label_nearest: null pointer");
    if (Nq <= 0 || Nk <= 0 || D <= 0 || C <= 0) return set_error(CLIBD_EINVAL, "same_label_nearest: non-positive shape");
    if (ldq < D || ldk < D) return set_error(CLIBD_EINVAL, "same_label_nearest: ldq and ldk must be >= D");
    if (!seg_ok(seg_host, C, Nk, false)) return set_error(CLIBD_EINVAL, "same_label_nearest: seg must rise from 0 to Nk (keys grouped by class)");
    hipLaunchKernelGGL(same_label_nearest_kernel, dim3((Nq + 3) / 4), dim3(256), 0, (hipStream_t)stream, Q, ldq, K, ldk, Nq, Nk, D, seg, C,
                       qclass, dist, (int*)arg);
    return check_launch("same_label_nearest");
}

extern "C" int clibd_confusion_counts(const int32_t* true_code, const int32_t* pred_code, size_t N, int C, int32_t* counts, void* stream) {
    if (!true_code || !pred_code || !counts) return set_error(CLIBD_EINVAL, "confusion_counts: null pointer");
    if (N == 0 || C <= 0) return set_error(CLIBD_EINVAL, "confusion_counts: non-positive shape");
    if (C > 46340) return set_error(CLIBD_EINVAL, "confusion_counts: C too large (C * C must stay below 2^31)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(zero_i32_kernel, dim3(grid_for((size_t)C * C)), dim3(256), 0, st, (int*)counts, (size_t)C * C);
    hipLaunchKernelGGL(confusion_counts_kernel, dim3(grid_for(N)), dim3(256), 0, st, (const int*)true_code, (const int*)pred_code, N, C,
                       (int*)counts);
    return check_launch("confusion_counts");
}
