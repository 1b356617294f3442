// The two SimCLR views of every image on the device (reference util/dataset.py:314-325 get_simclr_pipeline_transform):
// RandomResizedCrop(224) -> RandomHorizontalFlip -> RandomApply([ColorJitter(0.8, 0.8, 0.8, 0.2)], 0.8) -> RandomGrayscale(0.2) ->
// GaussianBlur(21, (0.1, 2.0)) -> ToTensor, from the decoded RGB HWC uint8 pixels to fp32 [n,3,224,224], one clibd_view_xform per view.
// The arithmetic is torchvision's tensor path for a float image, fp32 throughout, nothing rounded between the stages
// (include/clibd_hip_views.h).  The host draws every random parameter (clibd_amd/simclr_views.py); three kernels do the work:
//   1. views_weights_kernel: per view and axis, the antialiased bilinear weights of the crop box -> 224 (augment_common.h);
//   2. views_resample_kernel: one workgroup per (view, band of RB output rows): the band resample shared with augment.hip, the flipped
//      pre-jitter image into the workspace, and — the contrast mean is a whole-image reduction in the middle of a pointwise chain — one
//      partial sum per workgroup of gray(the colour operations that precede contrast);
//   3. views_finish_kernel: one workgroup per (view, band of BR output rows): the partials summed in a fixed order, the whole pointwise
//      chain (jitter, grayscale) on the band's rows plus the blur's 10-row halo, blurred along the rows into LDS, along the columns
//      from there into out.
// No atomics, no allocation, no synchronisation; a view's output depends on its record and pixels only.  Every read of the pixel
// buffer goes through a record that passed record_ok(), so no record can make a kernel read outside [0, data_bytes).
#include "common.h"
#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_views.h"
#include "host_util.h"
#include "augment_common.h"

namespace clibd {
namespace {

using namespace aug;

constexpr int VKMAX = 40;               // taps per output row / column: a box side <= 224 * DOWN_MAX needs at most 2 * 16 + 2 = 34
constexpr int BOX_MAX = OUT * DOWN_MAX; // 3584
constexpr int NBAND = OUT / RB;         // resample workgroups (= contrast partials) per view
constexpr int TAPS = 21, HALO = TAPS / 2;
constexpr int BR = 16;                  // output rows per finish workgroup
constexpr int NR = BR + 2 * HALO;       // rows of the pointwise image a band's blur reads
constexpr int FT = 512, FW = FT / 64;   // finish workgroup: threads, waves (one row of the pointwise image per wave at a time)
constexpr int FIPT = BR * 3 * OUT / FT; // outputs per thread in the column pass
static_assert(OUT % BR == 0 && BR * 3 * OUT % FT == 0 && OUT <= 4 * 64, "finish kernel's tiling");

using ViewTable = AxisTableT<VKMAX>;
constexpr size_t kTableBytes = sizeof(ViewTable);
constexpr size_t kImageBytes = (size_t)OUT * OUT * 3 * sizeof(float);
static_assert(kTableBytes % 16 == 0 && kImageBytes % 16 == 0, "workspace sections stay 16-byte aligned");

__device__ inline bool order_ok(int order) {
    if (order & ~0xffff) return false;
    int seen = 0;
    for (int j = 0; j < 4; ++j) {
        const int op = (order >> (4 * j)) & 15;
        if (op > 3) return false;
        seen |= 1 << op;
    }
    return seen == 15;
}

__device__ inline bool record_ok(const clibd_view_xform& x, size_t data_bytes) {
    if (x.H0 < 1 || x.W0 < 1 || x.H0 > 65535 || x.W0 > 65535) return false;
    if (x.h < 1 || x.w < 1 || x.h > BOX_MAX || x.w > BOX_MAX || x.top < 0 || x.left < 0 || x.top > x.H0 - x.h || x.left > x.W0 - x.w) return false;
    if (!order_ok(x.order) || !(x.sigma >= 0.1f && x.sigma <= 2.0f)) return false;
    if (!isfinite(x.brightness) || !isfinite(x.contrast) || !isfinite(x.saturation) || !isfinite(x.hue) || x.offset < 0) return false;
    const size_t n = (size_t)x.H0 * (size_t)x.W0 * 3;
    return (size_t)x.offset <= data_bytes && n <= data_bytes - (size_t)x.offset;
}

// ---- the pointwise chain: torchvision _functional_tensor, float branch.  Contraction is off so that a product and a sum round where
// torch's separate kernels round them.
__device__ inline float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ inline float gray_of(float r, float g, float b) {
#pragma clang fp contract(off)
    return 0.2989f * r + 0.587f * g + 0.114f * b;
}

__device__ inline float blend(float a, float b, float f) {
#pragma clang fp contract(off)
    return clamp01(f * a + (1.f - f) * b);
}

// adjust_hue: _rgb2hsv, h <- (h + shift) mod 1, _hsv2rgb
__device__ inline void hue_shift(float& r, float& g, float& b, float shift) {
#pragma clang fp contract(off)
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = __fdiv_rn(cr, eqc ? 1.f : maxc);
    const float dv = eqc ? 1.f : cr;
    const float rc = __fdiv_rn(maxc - r, dv), gc = __fdiv_rn(maxc - g, dv), bc = __fdiv_rn(maxc - b, dv);
    float h = maxc == r ? bc - gc : (maxc == g ? 2.f + rc - bc : 4.f + gc - rc);
    h = __fdiv_rn(h, 6.f) + 1.f;
    h = h - floorf(h);                  // fmod(h / 6 + 1, 1): the argument is positive
    h = h + shift;
    h = h - floorf(h);                  // python's mod 1
    const float v = maxc;
    const float h6 = h * 6.f, fl = floorf(h6), f = h6 - fl;
    int i = (int)fl;
    i = i >= 6 ? i - 6 : i;             // h can round up to 1
    const float p = clamp01(v * (1.f - s));
    const float q = clamp01(v * (1.f - s * f));
    const float t = clamp01(v * (1.f - s * (1.f - f)));
    r = i == 0 || i == 5 ? v : (i == 1 ? q : (i == 4 ? t : p));     // (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q)
    g = i == 1 || i == 2 ? v : (i == 0 ? t : (i == 3 ? q : p));
    b = i == 3 || i == 4 ? v : (i == 2 ? t : (i == 5 ? q : p));
}

// The record's colour operations in its order.  UNTIL_CONTRAST: only those that precede contrast (what its mean is taken over).
template <bool UNTIL_CONTRAST>
__device__ inline void jitter(float& r, float& g, float& b, const clibd_view_xform& x, float mean) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int op = (x.order >> (4 * j)) & 15;
        if (op == CLIBD_VIEW_OP_BRIGHTNESS) {
            r = blend(r, 0.f, x.brightness);
            g = blend(g, 0.f, x.brightness);
            b = blend(b, 0.f, x.brightness);
        } else if (op == CLIBD_VIEW_OP_CONTRAST) {
            if (UNTIL_CONTRAST) return;
            r = blend(r, mean, x.contrast);
            g = blend(g, mean, x.contrast);
            b = blend(b, mean, x.contrast);
        } else if (op == CLIBD_VIEW_OP_SATURATION) {
            const float y = gray_of(r, g, b);
            r = blend(r, y, x.saturation);
            g = blend(g, y, x.saturation);
            b = blend(b, y, x.saturation);
        } else {
            hue_shift(r, g, b, x.hue);
        }
    }
}

__global__ __launch_bounds__(256) void views_weights_kernel(const clibd_view_xform* __restrict__ xf, size_t data_bytes,
                                                            ViewTable* __restrict__ tables) {
    const int b = blockIdx.x;
    const clibd_view_xform x = xf[b];
    const bool ok = record_ok(x, data_bytes);
    for (int i = threadIdx.x; i < 2 * OUT; i += blockDim.x) {
        const int axis = i / OUT, o = i - axis * OUT;
        if (axis == 0) axis_weights(o, x.H0, x.H0, x.top, x.h, ok, tables + 2 * (size_t)b);
        else axis_weights(o, x.W0, x.W0, x.left, x.w, ok, tables + 2 * (size_t)b + 1);
    }
}

__global__ __launch_bounds__(256) void views_resample_kernel(const unsigned char* __restrict__ data, const clibd_view_xform* __restrict__ xf,
                                                             size_t data_bytes, const ViewTable* __restrict__ tables, float* __restrict__ pre,
                                                             float* __restrict__ partials) {
    __shared__ float rows[CAP][OUT * 3];
    __shared__ float part[4];
    const int b = blockIdx.y, r0 = blockIdx.x * RB, tid = threadIdx.x;
    const clibd_view_xform x = xf[b];
    const ViewTable* TV = tables + 2 * (size_t)b;
    float acc[IPT][3];
    resample_band(data + x.offset, x.W0, TV, TV + 1, r0, tid, rows, acc);
    // pixel values are u8 / 255 (ToTensor, IEEE division); the weights act on the bytes, so an exact copy stays exact
    const bool hf = x.flags & CLIBD_VIEW_HFLIP;
    const bool mean_needed = (x.flags & CLIBD_VIEW_JITTER) && record_ok(x, data_bytes);
    float local = 0.f;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const int i = tid + 256 * j;
        const int rr = i / OUT, o = i - rr * OUT, r = r0 + rr;
        float v0 = __fdiv_rn(acc[j][0], 255.f), v1 = __fdiv_rn(acc[j][1], 255.f), v2 = __fdiv_rn(acc[j][2], 255.f);
        float* q = pre + ((size_t)b * 3 * OUT + r) * OUT + (hf ? OUT - 1 - o : o);
        q[0] = v0;
        q[(size_t)OUT * OUT] = v1;
        q[(size_t)2 * OUT * OUT] = v2;
        if (mean_needed) {
            jitter<true>(v0, v1, v2, x, 0.f);
            local += gray_of(v0, v1, v2);
        }
    }
    const float w = wave_sum(local);
    if ((tid & 63) == 0) part[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) partials[(size_t)b * NBAND + blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

__device__ inline int reflect(int i) { return i < 0 ? -i : (i >= OUT ? 2 * (OUT - 1) - i : i); }

__global__ __launch_bounds__(FT) void views_finish_kernel(const clibd_view_xform* __restrict__ xf, size_t data_bytes,
                                                          const float* __restrict__ pre, const float* __restrict__ partials,
                                                          float* __restrict__ out) {
    __shared__ float Hs[NR][3][OUT];     // the pointwise image of the band and its halo, blurred along the rows
    __shared__ float line[FW][3][OUT];   // one pointwise row per wave
    __shared__ float wts[TAPS];
    const int b = blockIdx.y, r0 = blockIdx.x * BR, tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    const clibd_view_xform x = xf[b];
    float* dst = out + (size_t)b * 3 * OUT * OUT;
    if (!record_ok(x, data_bytes)) {     // the same for the whole workgroup
#pragma unroll
        for (int j = 0; j < FIPT; ++j) {
            const int i = tid + FT * j;
            const int r = i / (3 * OUT), c = (i / OUT) % 3, o = i % OUT;
            dst[((size_t)c * OUT + r0 + r) * OUT + o] = 0.f;
        }
        return;
    }
    const bool jit = x.flags & CLIBD_VIEW_JITTER, gray = x.flags & CLIBD_VIEW_GRAY;
    float mean = 0.f;
    if (jit) {
        for (int i = 0; i < NBAND; ++i) mean += partials[(size_t)b * NBAND + i];
        mean = __fdiv_rn(mean, (float)(OUT * OUT));
    }
    if (tid < TAPS) {
        const float t = __fdiv_rn((float)(tid - HALO), x.sigma);
        wts[tid] = expf(-0.5f * (t * t));
    }
    __syncthreads();
    float total = 0.f;
    for (int k = 0; k < TAPS; ++k) total += wts[k];
    __syncthreads();
    if (tid < TAPS) wts[tid] = __fdiv_rn(wts[tid], total);

    const float* src = pre + (size_t)b * 3 * OUT * OUT;
    for (int j0 = 0; j0 < NR; j0 += FW) {
        const int j = j0 + wv;
        if (j < NR) {
            const int y = reflect(r0 - HALO + j);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = ln + 64 * q;
                if (o < OUT) {
                    const float* p = src + (size_t)y * OUT + o;
                    float v0 = p[0], v1 = p[(size_t)OUT * OUT], v2 = p[(size_t)2 * OUT * OUT];
                    if (jit) jitter<false>(v0, v1, v2, x, mean);
                    if (gray) v0 = v1 = v2 = gray_of(v0, v1, v2);
                    line[wv][0][o] = v0;
                    line[wv][1][o] = v1;
                    line[wv][2][o] = v2;
                }
            }
        }
        __syncthreads();                 // the rows are written (and wts, the first time round)
        if (j < NR) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = ln + 64 * q;
                if (o < OUT) {
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
                    for (int k = 0; k < TAPS; ++k) {
                        const int s = reflect(o + k - HALO);
                        const float w = wts[k];
                        a0 = fmaf(w, line[wv][0][s], a0);   // explicit: the three channels of a gray image must round alike
                        a1 = fmaf(w, line[wv][1][s], a1);
                        a2 = fmaf(w, line[wv][2][s], a2);
                    }
                    Hs[j][0][o] = a0;
                    Hs[j][1][o] = a1;
                    Hs[j][2][o] = a2;
                }
            }
        }
        __syncthreads();                 // the rows are read; Hs is complete after the last round
    }
#pragma unroll
    for (int j = 0; j < FIPT; ++j) {
        const int i = tid + FT * j;
        const int r = i / (3 * OUT), c = (i / OUT) % 3, o = i % OUT;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) a = fmaf(wts[k], Hs[r + k][c][o], a);
        dst[((size_t)c * OUT + r0 + r) * OUT + o] = a;
    }
}

}  // namespace
}  // namespace clibd

using namespace clibd;

static size_t partial_bytes(size_t n) { return (n * NBAND * sizeof(float) + 15) / 16 * 16; }

extern "C" size_t clibd_simclr_views_workspace_bytes(int n) {
    return n <= 0 ? 0 : (size_t)n * (2 * kTableBytes + kImageBytes) + partial_bytes((size_t)n);
}

extern "C" int clibd_simclr_views_u8(const void* data, size_t data_bytes, const clibd_view_xform* xf, int n, float* out, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (!data || !xf || !out || !workspace) return set_error(CLIBD_EINVAL, "simclr_views_u8: null pointer");
    if (n <= 0 || n > 65535) return set_error(CLIBD_EINVAL, "simclr_views_u8: n must be in [1, 65535]");
    if (((uintptr_t)xf & 7) || !aligned16(out) || !aligned16(workspace)) return set_error(CLIBD_EINVAL, "simclr_views_u8: alignment");
    if (workspace_bytes < clibd_simclr_views_workspace_bytes(n))
        return set_error(CLIBD_EINVAL, "simclr_views_u8: workspace too small (clibd_simclr_views_workspace_bytes)");
    ViewTable* tables = (ViewTable*)workspace;
    float* pre = (float*)((char*)workspace + (size_t)n * 2 * kTableBytes);
    float* partials = (float*)((char*)pre + (size_t)n * kImageBytes);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(views_weights_kernel, dim3(n), dim3(256), 0, s, xf, data_bytes, tables);
    hipLaunchKernelGGL(views_resample_kernel, dim3(NBAND, n), dim3(256), 0, s, (const unsigned char*)data, xf, data_bytes, tables, pre, partials);
    hipLaunchKernelGGL(views_finish_kernel, dim3(OUT / BR, n), dim3(FT), 0, s, xf, data_bytes, pre, partials, out);
    return check_launch("simclr_views_u8");
}
