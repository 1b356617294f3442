// The INSECT / BZSL workflow's kernels for gfx950 (reference: scripts/BZSL/*.py, bioscanclip/epoch/fine_tuning_epoch.py): the per-class
// mean of embedding rows in numpy's summation order and the top-k of the logits themselves.
//
//   mean[c, :] = (((x[i1, :] + x[i2, :]) + x[i3, :]) + ... + x[in, :]) / n       i1 < i2 < ... < in the rows with labels[i] == c
//   val, idx   = the k largest logits of a row and their columns, equal values by ascending column
//
// The chain along a class's rows is sequential by definition — `==` against np.sum(rows, axis=0) / len(rows) needs that one order — so
// the parallelism is over the C * D independent chains.  The per-class row lists are built once: an integer histogram (count), an
// exclusive scan (offsets), a fill through integer atomics (which places a class's rows in any order) and a sort of each list back into
// ascending row order (the rows of a class are distinct, so every sort gives the same list).  No float atomics: two calls agree bit
// for bit, whatever the launch shape.
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_insect.h"
#include "host_util.h"

namespace clibd {

constexpr int kMaxProtoClasses = 65536;
constexpr int SORT_LDS = 4096;    // the longest row list that is sorted in LDS (16 KiB); a longer one is rebuilt by an ordered rescan

// count[l] += 1 per row; a label outside [0, C) only raises the flag (integer atomics: the totals do not depend on the order)
__global__ __launch_bounds__(256) void label_hist_kernel(const int* __restrict__ labels, int N, int C, int* __restrict__ count,
                                                         unsigned* __restrict__ err) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        const int l = labels[i];
        if ((unsigned)l < (unsigned)C) atomicAdd(&count[l], 1);
        else atomicOr(err, 1u);
    }
}

// offsets[c] = sum_{c' < c} count[c'], offsets[C] = the rows in range; cursor = offsets.  One workgroup of 1024: thread t owns the
// classes [t * per, (t + 1) * per), per <= 64.
__global__ __launch_bounds__(1024) void class_scan_kernel(const int* __restrict__ count, int C, int* __restrict__ offsets,
                                                          int* __restrict__ cursor) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (C + 1023) / 1024;
    const int c0 = t * per;
    const int c1 = min(c0 + per, C);
    int s = 0;
    for (int c = c0; c < c1; ++c) s += count[c];
    part[t] = s;
    __syncthreads();
    for (int w = 1; w < 1024; w <<= 1) {
        const int v = t >= w ? part[t - w] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int c = c0; c < c1; ++c) {
        offsets[c] = run;
        cursor[c] = run;
        run += count[c];
    }
    if (t == 1023) offsets[C] = part[1023];
}

// rows[cursor[l]++] = i: every class's list is complete after this kernel, in an order that the next kernel restores
__global__ __launch_bounds__(256) void class_fill_kernel(const int* __restrict__ labels, int N, int C, int* __restrict__ cursor,
                                                         int* __restrict__ rows) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        const int l = labels[i];
        if ((unsigned)l < (unsigned)C) rows[atomicAdd(&cursor[l], 1)] = (int)i;
    }
}

// One workgroup per class: its list in ascending row order.  Up to SORT_LDS rows: a bitonic sort in LDS, the tail padded with INT_MAX.
// Longer: the list is written again by walking the labels in order (ballot + popcount place the matches of each 256 rows), N reads per
// such class — there are fewer than N / SORT_LDS of them.
__global__ __launch_bounds__(256) void class_sort_kernel(const int* __restrict__ labels, int N, int C, const int* __restrict__ offsets,
                                                         int* __restrict__ rows) {
    __shared__ int buf[SORT_LDS];
    __shared__ int wtot[4];
    const int t = threadIdx.x;
    for (int c = blockIdx.x; c < C; c += gridDim.x) {
        const int o = offsets[c];
        const int n = offsets[c + 1] - o;
        if (n <= 1) continue;   // the same for every thread of the workgroup
        if (n <= SORT_LDS) {
            int P = 2;
            while (P < n) P <<= 1;
            for (int i = t; i < P; i += 256) buf[i] = i < n ? rows[o + i] : 0x7fffffff;
            __syncthreads();
            for (int k = 2; k <= P; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = t; i < P; i += 256) {
                        const int p = i ^ j;
                        if (p > i) {
                            const int a = buf[i], b = buf[p];
                            if (((i & k) == 0) ? (a > b) : (a < b)) {
                                buf[i] = b;
                                buf[p] = a;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            for (int i = t; i < n; i += 256) rows[o + i] = buf[i];
            __syncthreads();
        } else {
            const int lane = t & 63, w = t >> 6;
            int base = 0;
            for (long long i0 = 0; i0 < N; i0 += 256) {
                const long long i = i0 + t;
                const bool f = i < N && labels[i] == c;
                const unsigned long long m = __ballot(f);
                const int pre = __popcll(m & ((1ull << lane) - 1ull));
                if (lane == 0) wtot[w] = __popcll(m);
                __syncthreads();
                int before = 0, tot = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int v = wtot[q];
                    before += q < w ? v : 0;
                    tot += v;
                }
                if (f) rows[o + base + before + pre] = (int)i;   // base + before + pre < n: the histogram counted the same labels
                base += tot;
                __syncthreads();
            }
        }
    }
}

// One thread per (class, column) — per four columns with VEC (16-byte loads: D % 4 == 0, ld_x % 4 == 0, x 16-byte aligned).  Neighbouring
// threads read neighbouring columns of the same row; the row indices are the same address for the whole group.  The adds of a chain are
// in list order, the loads of four rows are issued ahead of them.
template <bool VEC>
__global__ __launch_bounds__(256) void class_mean_kernel(const float* __restrict__ x, size_t ld_x, const int* __restrict__ offsets,
                                                         const int* __restrict__ rows, int C, int D, float* __restrict__ mean,
                                                         size_t ld_mean, int transposed, int vec_store) {
    constexpr int W = VEC ? 4 : 1;
    const int DV = D / W;
    const size_t total = (size_t)C * DV;
    for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (size_t)gridDim.x * 256) {
        const int c = (int)(it / DV);
        const int d = (int)(it - (size_t)c * DV) * W;
        const int o = offsets[c];
        const int n = offsets[c + 1] - o;
        float a[4] = {0.f, 0.f, 0.f, 0.f};   // a[0 .. W - 1] are in use
        if (n > 0) {
            const float* xd = x + d;
            const int* rl = rows + o;
            if constexpr (VEC) {
                const float4 v = *(const float4*)(xd + (size_t)rl[0] * ld_x);
                a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
            } else {
                a[0] = xd[(size_t)rl[0] * ld_x];
            }
            int j = 1;
            if constexpr (VEC) {
                for (; j + 4 <= n; j += 4) {
                    const float4 v0 = *(const float4*)(xd + (size_t)rl[j] * ld_x);
                    const float4 v1 = *(const float4*)(xd + (size_t)rl[j + 1] * ld_x);
                    const float4 v2 = *(const float4*)(xd + (size_t)rl[j + 2] * ld_x);
                    const float4 v3 = *(const float4*)(xd + (size_t)rl[j + 3] * ld_x);
                    a[0] = ((((a[0] + v0.x) + v1.x) + v2.x) + v3.x);
                    a[1] = ((((a[1] + v0.y) + v1.y) + v2.y) + v3.y);
                    a[2] = ((((a[2] + v0.z) + v1.z) + v2.z) + v3.z);
                    a[3] = ((((a[3] + v0.w) + v1.w) + v2.w) + v3.w);
                }
                for (; j < n; ++j) {
                    const float4 v = *(const float4*)(xd + (size_t)rl[j] * ld_x);
                    a[0] = a[0] + v.x;
                    a[1] = a[1] + v.y;
                    a[2] = a[2] + v.z;
                    a[3] = a[3] + v.w;
                }
            } else {
                for (; j + 4 <= n; j += 4) {
                    const float v0 = xd[(size_t)rl[j] * ld_x], v1 = xd[(size_t)rl[j + 1] * ld_x];
                    const float v2 = xd[(size_t)rl[j + 2] * ld_x], v3 = xd[(size_t)rl[j + 3] * ld_x];
                    a[0] = ((((a[0] + v0) + v1) + v2) + v3);
                }
                for (; j < n; ++j) a[0] = a[0] + xd[(size_t)rl[j] * ld_x];
            }
            const float fn = (float)n;
#pragma unroll
            for (int q = 0; q < W; ++q) a[q] = a[q] / fn;   // the correctly rounded fp32 divide (hipcc's default)
        }
        if (transposed) {
#pragma unroll
            for (int q = 0; q < W; ++q) mean[(size_t)(d + q) * ld_mean + c] = a[q];
        } else if (VEC && vec_store) {
            *(float4*)(mean + (size_t)c * ld_mean + d) = make_float4(a[0], a[1], a[2], a[3]);
        } else {
#pragma unroll
            for (int q = 0; q < W; ++q) mean[(size_t)c * ld_mean + d + q] = a[q];
        }
    }
}

// softmax_topk_kernel's selection (classifier.hip) on the logits themselves: one wave per row, every lane keeps the 8 best
// (value, index) pairs of its stride-64 share in named registers (a fully unrolled compare-exchange chain: scratch 0), then k rounds in
// which the wave's best head wins — wave_max of the values, then the lowest index among the lanes that hold it (an index below 2^24 is
// exact in fp32) — and its lane pops it.  -inf is an ordinary value: an empty slot is (-inf, NOIDX), and a real index ranks before NOIDX.
__global__ __launch_bounds__(256) void logits_topk_kernel(const float* __restrict__ logits, int ld, int B, int C, int k,
                                                          float* __restrict__ val, int64_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* lr = logits + (size_t)row * ld;
    constexpr float NEG = -__builtin_huge_valf();
    constexpr int NOIDX = 0x7fffffff;
    float v0 = NEG, v1 = NEG, v2 = NEG, v3 = NEG, v4 = NEG, v5 = NEG, v6 = NEG, v7 = NEG;
    int i0 = NOIDX, i1 = NOIDX, i2 = NOIDX, i3 = NOIDX, i4 = NOIDX, i5 = NOIDX, i6 = NOIDX, i7 = NOIDX;
#define CLIBD_CEX(V, I)                       \
    if (ranks_before(cv, ci, V, I)) {         \
        const float tv = V; const int ti = I; \
        V = cv; I = ci; cv = tv; ci = ti;     \
    }
    for (int j = lane; j < C; j += 64) {
        float cv = lr[j];
        int ci = j;
        CLIBD_CEX(v0, i0) CLIBD_CEX(v1, i1) CLIBD_CEX(v2, i2) CLIBD_CEX(v3, i3)
        CLIBD_CEX(v4, i4) CLIBD_CEX(v5, i5) CLIBD_CEX(v6, i6) CLIBD_CEX(v7, i7)
    }
#undef CLIBD_CEX
    for (int r = 0; r < k; ++r) {
        const float best = wave_max(v0);
        const float cand = (v0 == best && i0 != NOIDX) ? (float)i0 : 3.0e38f;
        const int win = (int)(-wave_max(-cand));
        if (lane == 0) {
            val[(size_t)row * k + r] = best;
            idx[(size_t)row * k + r] = (int64_t)win;
        }
        if (i0 == win) {
            v0 = v1; i0 = i1; v1 = v2; i1 = i2; v2 = v3; i2 = i3; v3 = v4; i3 = i4;
            v4 = v5; i4 = i5; v5 = v6; i5 = i6; v6 = v7; i6 = i7; v7 = NEG; i7 = NOIDX;
        }
    }
}

struct ProtoWs {
    int *offsets, *cursor, *rows;   // [C + 1], [C], [N]
    size_t total;
};

static ProtoWs carve_proto(void* base, int N, int C) {
    ProtoWs w;
    Carver c(base);
    w.offsets = c.take<int>((size_t)C + 1);
    w.cursor = c.take<int>((size_t)C);
    w.rows = c.take<int>((size_t)N);
    w.total = c.total();
    return w;
}

}  // namespace clibd

using namespace clibd;

extern "C" size_t clibd_class_mean_workspace_bytes(int N, int C) {
    if (N <= 0 || C <= 0 || C > kMaxProtoClasses) return 0;
    return carve_proto(nullptr, N, C).total;
}

extern "C" int clibd_class_mean_f32(const float* x, int ld_x, const int32_t* labels, int N, int C, int D, float* mean, int ld_mean,
                                    int transposed, int32_t* count, int32_t* error, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    const char* op = "class_mean_f32";
    if (!x || !labels || !mean || !count || !error || !workspace) return fail(op, "null pointer");
    if (N <= 0 || C <= 0 || D <= 0) return fail(op, "non-positive shape");
    if (C > kMaxProtoClasses) return fail(op, "C must be at most 65536");
    if ((long long)N * (long long)D >= (1ll << 31)) return fail(op, "N * D must be below 2^31");
    if (transposed != 0 && transposed != 1) return fail(op, "transposed must be 0 or 1");
    if (ld_x < D) return fail(op, "ld_x must be >= D");
    if (ld_mean < (transposed ? C : D)) return fail(op, "ld_mean must be >= D (>= C when transposed)");
    if ((((uintptr_t)x) & 3u) != 0 || (((uintptr_t)mean) & 3u) != 0) return fail(op, "x and mean must be 4-byte aligned");
    if (!aligned16(workspace) || workspace_bytes < clibd_class_mean_workspace_bytes(N, C))
        return fail(op, "workspace too small or misaligned (clibd_class_mean_workspace_bytes)");
    const ProtoWs ws = carve_proto(workspace, N, C);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, (size_t)C * sizeof(int), st) != hipSuccess) return set_error(CLIBD_ELAUNCH, "class_mean_f32: memset failed");
    hipLaunchKernelGGL(label_hist_kernel, dim3(grid_for((size_t)N)), dim3(256), 0, st, labels, N, C, count, (unsigned*)error);
    if (int e = check_launch("class_mean_f32 histogram")) return e;
    hipLaunchKernelGGL(class_scan_kernel, dim3(1), dim3(1024), 0, st, count, C, ws.offsets, ws.cursor);
    if (int e = check_launch("class_mean_f32 scan")) return e;
    hipLaunchKernelGGL(class_fill_kernel, dim3(grid_for((size_t)N)), dim3(256), 0, st, labels, N, C, ws.cursor, ws.rows);
    if (int e = check_launch("class_mean_f32 fill")) return e;
    hipLaunchKernelGGL(class_sort_kernel, dim3(C < 4096 ? C : 4096), dim3(256), 0, st, labels, N, C, ws.offsets, ws.rows);
    if (int e = check_launch("class_mean_f32 sort")) return e;
    const bool vec = D % 4 == 0 && ld_x % 4 == 0 && aligned16(x);
    const int vec_store = !transposed && ld_mean % 4 == 0 && aligned16(mean);
    if (vec)
        hipLaunchKernelGGL(class_mean_kernel<true>, dim3(grid_for((size_t)C * (D / 4))), dim3(256), 0, st, x, (size_t)ld_x, ws.offsets, ws.rows,
                           C, D, mean, (size_t)ld_mean, transposed, vec_store);
    else
        hipLaunchKernelGGL(class_mean_kernel<false>, dim3(grid_for((size_t)C * D)), dim3(256), 0, st, x, (size_t)ld_x, ws.offsets, ws.rows, C,
                           D, mean, (size_t)ld_mean, transposed, 0);
    return check_launch("class_mean_f32");
}

extern "C" int clibd_logits_topk(const float* logits, int ld, int B, int C, int k, float* val, int64_t* idx, void* stream) {
    const char* op = "logits_topk";
    if (!logits || !val || !idx) return fail(op, "null pointer");
    if (B <= 0 || C <= 0) return fail(op, "non-positive shape");
    if (C > (1 << 24)) return fail(op, "C too large");
    if (ld < C) return fail(op, "ld must be >= C");
    if ((((uintptr_t)logits) & 3u) != 0) return fail(op, "logits must be 4-byte aligned");
    if (k < 1 || k > 8) return fail(op, "k must be in 1..8");
    if (k > C) return fail(op, "k larger than the number of classes (selected index k out of range)");
    hipLaunchKernelGGL(logits_topk_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, B, C, k, val, idx);
    return check_launch("logits_topk");
}
