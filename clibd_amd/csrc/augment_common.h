// The resampling core shared by the dataset transforms (augment.hip) and the SimCLR views (views.hip): torch's separable antialiased
// bilinear filter as per-axis weight tables, and the band resample (horizontal pass into LDS, vertical pass into registers, fp32 sums
// in a fixed order).  Each unit keeps its own record type, guard and epilogue.
#pragma once
#include "common.h"

namespace clibd {
namespace aug {

constexpr int OUT = 224;        // output side
constexpr int DOWN_MAX = 16;    // resize factor in / out per axis
constexpr int RB = 8;           // output rows per resample workgroup
constexpr int CAP = 16;         // horizontally filtered source rows staged in LDS at a time (16 x 224 x 3 fp32 = 42 KiB)
constexpr int IPT = RB * OUT / 256;   // (row, column) items per thread in the vertical pass

template <int KMAX_>
struct AxisTableT {             // per (image, axis); weights k-major so that neighbouring columns read neighbouring words
    static constexpr int KMAX = KMAX_;   // taps per output row / column the table holds
    int base[OUT];              // first source index of output index o
    int cnt[OUT];               // number of taps (0: the record is invalid, the output is 0)
    float w[KMAX_][OUT];
};

// torch's antialiased bilinear taps of output index o for in -> out (aten UpSampleKernel _compute_indices_min_size_weights_aa):
// scale = in/out, center = scale (o + 0.5), support = max(scale, 1), taps [max(int(center - support + 0.5), 0),
// min(int(center + support + 0.5), in)), weight max(0, 1 - |(t - center + 0.5) / max(scale, 1)|), normalised to sum 1.
struct Taps {
    int lo, hi;
    float center, inv, total;
    __device__ float raw(int t) const { return fmaxf(0.f, 1.f - fabsf(((float)t - center + 0.5f) * inv)); }
    __device__ float weight(int t) const { return raw(t) / total; }
};

__device__ inline Taps taps_of(int o, int in, int out) {
    Taps T;
    const float scale = (float)in / (float)out;
    const float support = scale >= 1.f ? scale : 1.f;
    T.center = (float)((double)scale * ((double)o + 0.5));
    T.inv = scale >= 1.f ? 1.f / scale : 1.f;
    T.lo = max((int)((double)T.center - (double)support + 0.5), 0);
    T.hi = min((int)((double)T.center + (double)support + 0.5), in);
    T.total = 0.f;
    for (int t = T.lo; t < T.hi; ++t) T.total += T.raw(t);
    if (T.total == 0.f) T.total = 1.f;
    return T;
}

// Composite weights of output index o on one axis: crop resample ext -> 224 (taps clamped to [0, ext), offset by off into the resized
// axis of size mid), then the resize in -> mid.  Sizes that do not change are exact copies (torch's filter at unit scale).  Taps beyond
// the table's KMAX are dropped, never written.
template <class Table>
__device__ void axis_weights(int o, int in, int mid, int off, int ext, bool ok, Table* __restrict__ T) {
    if (!ok) {
        T->base[o] = 0;
        T->cnt[o] = 0;
        return;
    }
    const bool crop_copy = ext == OUT, resize_copy = in == mid;
    Taps C;
    if (crop_copy) {
        C.lo = o; C.hi = o + 1; C.center = 0.f; C.inv = 1.f; C.total = 1.f;
    } else {
        C = taps_of(o, ext, OUT);
    }
    int lo, hi;
    if (resize_copy) {
        lo = off + C.lo;
        hi = off + C.hi;
    } else {
        lo = taps_of(off + C.lo, in, mid).lo;
        hi = taps_of(off + C.hi - 1, in, mid).hi;
    }
    const int n = min(max(hi - lo, 0), Table::KMAX);
    for (int k = 0; k < n; ++k) T->w[k][o] = 0.f;
    for (int c = C.lo; c < C.hi; ++c) {
        const float wc = crop_copy ? 1.f : C.weight(c);
        const int t = off + c;
        if (resize_copy) {
            if (t - lo < n) T->w[t - lo][o] += wc;
        } else {
            const Taps R = taps_of(t, in, mid);
            for (int s = R.lo; s < R.hi; ++s)
                if (s - lo >= 0 && s - lo < n) T->w[s - lo][o] += wc * R.weight(s);
        }
    }
    T->base[o] = lo;
    T->cnt[o] = n;
}

// One workgroup of 256 threads, output rows [r0, r0 + RB) of one image: acc[j] = the weighted sums of the source BYTES (not yet divided
// by 255) of item i = tid + 256 j, row r0 + i / 224, column i % 224.  `img`: the image's first pixel, W0 its row length in pixels;
// `rows`: CAP x (224 * 3) floats of LDS.  An invalid record's tables hold no taps: nothing is read and every sum is 0.
template <class Table>
__device__ inline void resample_band(const unsigned char* __restrict__ img, int W0, const Table* __restrict__ TV, const Table* __restrict__ TH,
                                     int r0, int tid, float (*rows)[OUT * 3], float (&acc)[IPT][3]) {
    int S0 = 0x7fffffff, S1 = 0;          // source rows the band needs (empty for an invalid record: every cnt is 0)
    for (int r = r0; r < r0 + RB; ++r) {
        const int n = TV->cnt[r];
        if (n > 0) {
            S0 = min(S0, TV->base[r]);
            S1 = max(S1, TV->base[r] + n);
        }
    }
#pragma unroll
    for (int j = 0; j < IPT; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.f;

    for (int c0 = S0; c0 < S1; c0 += CAP) {
        const int nrow = min(CAP, S1 - c0);
        __syncthreads();                  // the previous chunk's readers are done
        for (int i = tid; i < nrow * OUT; i += 256) {
            const int rr = i / OUT, o = i - rr * OUT;
            const int xb = TH->base[o], n = TH->cnt[o];
            const unsigned char* p = img + ((size_t)(c0 + rr) * W0 + xb) * 3;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            for (int k = 0; k < n; ++k) {
                const float w = TH->w[k][o];
                a0 += w * (float)p[3 * k];
                a1 += w * (float)p[3 * k + 1];
                a2 += w * (float)p[3 * k + 2];
            }
            rows[rr][o * 3] = a0;
            rows[rr][o * 3 + 1] = a1;
            rows[rr][o * 3 + 2] = a2;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const int i = tid + 256 * j;
            const int rr = i / OUT, o = i - rr * OUT, r = r0 + rr;
            const int vb = TV->base[r], vn = TV->cnt[r];
            const int k0 = max(c0, vb), k1 = min(c0 + nrow, vb + vn);
            for (int s = k0; s < k1; ++s) {
                const float w = TV->w[s - vb][r];
                acc[j][0] += w * rows[s - c0][o * 3];
                acc[j][1] += w * rows[s - c0][o * 3 + 1];
                acc[j][2] += w * rows[s - c0][o * 3 + 2];
            }
        }
    }
}

}  // namespace aug
}  // namespace clibd
