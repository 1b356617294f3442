// Image transforms of the dataset on the device (reference util/dataset.py:185-195 training, :216-224 eval): Resize(256, antialias)
// -> RandomResizedCrop(224, antialias) / CenterCrop(224) -> RandomHorizontalFlip -> RandomVerticalFlip -> RandomRotation((-45, 45)),
// from the decoded RGB HWC uint8 pixels to fp32 [B,3,224,224].  The host draws every random parameter (clibd_amd/augment.py) and
// hands one clibd_image_xform per image; three kernels do the arithmetic:
//   1. axis_weights_kernel: per image and axis, the composite weights (Resize o crop-resample) of each of the 224 output rows / columns
//      over the source pixels, torch's separable antialiased bilinear filter for both factors (taps clamped to the image for the
//      resize, to the crop box for the crop resample; an axis whose size does not change is an exact copy);
//   2. resample_kernel: one workgroup per (image, band of RB output rows): the horizontal pass of the source rows the band needs into
//      LDS, the vertical pass from there into registers, fp32 sums in a fixed order; out directly (flips applied) or, for a record that
//      rotates, the pre-rotation image into the workspace;
//   3. rotate_kernel: torchvision's rotate (grid_sample nearest, zeros outside) of the flipped pre-rotation image into out.
// No atomics, no allocation, no synchronisation; an image's output depends on its record and pixels only.  Every read of the pixel
// buffer goes through a record that passed record_ok(), so no record can make a kernel read outside [0, data_bytes).
#include "common.h"
#include "../../include/clibd_hip.h"
#include "host_util.h"
#include "augment_common.h"

namespace clibd {
namespace {

using namespace aug;            // OUT, DOWN_MAX, RB, CAP, IPT, the weight tables and the band resample (augment_common.h)

constexpr int KMAX = 128;       // composite taps per output row / column (h, w <= 384 and a resize factor <= 16 need at most 98)
constexpr int CROP_MAX = 384;   // crop box side (RandomResizedCrop of a 256-short-side image: <= 342)
using AxisTable = AxisTableT<KMAX>;
constexpr size_t kTableBytes = sizeof(AxisTable);
constexpr size_t kPrerotBytes = (size_t)OUT * OUT * 3 * sizeof(float);
static_assert(kTableBytes % 16 == 0 && kPrerotBytes % 16 == 0, "workspace sections stay 16-byte aligned");

__device__ inline bool record_ok(const clibd_image_xform& x, size_t data_bytes) {
    if (x.H0 < 1 || x.W0 < 1 || x.H1 < 1 || x.W1 < 1 || x.H0 > 65535 || x.W0 > 65535 || x.H1 > 65535 || x.W1 > 65535) return false;
    if (x.h < 1 || x.w < 1 || x.h > CROP_MAX || x.w > CROP_MAX || x.top < 0 || x.left < 0 || x.top > x.H1 - x.h || x.left > x.W1 - x.w) return false;
    if (x.H0 > DOWN_MAX * x.H1 || x.W0 > DOWN_MAX * x.W1 || x.offset < 0) return false;
    const size_t n = (size_t)x.H0 * (size_t)x.W0 * 3;
    return (size_t)x.offset <= data_bytes && n <= data_bytes - (size_t)x.offset;
}

__global__ __launch_bounds__(256) void axis_weights_kernel(const clibd_image_xform* __restrict__ xf, size_t data_bytes,
                                                           AxisTable* __restrict__ tables) {
    const int b = blockIdx.x;
    const clibd_image_xform x = xf[b];
    const bool ok = record_ok(x, data_bytes);
    for (int i = threadIdx.x; i < 2 * OUT; i += blockDim.x) {
        const int axis = i / OUT, o = i - axis * OUT;
        if (axis == 0) axis_weights(o, x.H0, x.H1, x.top, x.h, ok, tables + 2 * (size_t)b);
        else axis_weights(o, x.W0, x.W1, x.left, x.w, ok, tables + 2 * (size_t)b + 1);
    }
}

__global__ __launch_bounds__(256) void resample_kernel(const unsigned char* __restrict__ data, const clibd_image_xform* __restrict__ xf,
                                                       const AxisTable* __restrict__ tables, float* __restrict__ prerot,
                                                       float* __restrict__ out) {
    __shared__ float rows[CAP][OUT * 3];
    const int b = blockIdx.y, r0 = blockIdx.x * RB, tid = threadIdx.x;
    const clibd_image_xform x = xf[b];
    const AxisTable* TV = tables + 2 * (size_t)b;
    const AxisTable* TH = TV + 1;
    float acc[IPT][3];
    resample_band(data + x.offset, x.W0, TV, TH, r0, tid, rows, acc);
    // pixel values are u8 / 255 (ToTensor, IEEE division); the weights act on the bytes, so an exact copy stays exact
    const bool rot = x.flags & CLIBD_XF_ROTATE, hf = x.flags & CLIBD_XF_HFLIP, vf = x.flags & CLIBD_XF_VFLIP;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const int i = tid + 256 * j;
        const int rr = i / OUT, o = i - rr * OUT, r = r0 + rr;
        const float v0 = __fdiv_rn(acc[j][0], 255.f), v1 = __fdiv_rn(acc[j][1], 255.f), v2 = __fdiv_rn(acc[j][2], 255.f);
        if (rot) {
            float* q = prerot + (((size_t)b * OUT + r) * OUT + o) * 3;
            q[0] = v0;
            q[1] = v1;
            q[2] = v2;
        } else {
            const int y = vf ? OUT - 1 - r : r, xo = hf ? OUT - 1 - o : o;
            float* q = out + ((size_t)b * 3 * OUT + y) * OUT + xo;
            q[0] = v0;
            q[(size_t)OUT * OUT] = v1;
            q[(size_t)2 * OUT * OUT] = v2;
        }
    }
}

// torchvision F.rotate(img, angle, NEAREST, expand=False, center=None, fill=0) on the flipped pre-rotation image: output pixel (y, x)
// samples grid = [x - 111.5, y - 111.5, 1] . (theta^T / 112), source = rint((g + 1) * 112 - 0.5) (grid_sample nearest,
// align_corners=False, ties to even), 0 outside.  One thread = 4 consecutive x (three 16-byte stores).
__global__ __launch_bounds__(256) void rotate_kernel(const clibd_image_xform* __restrict__ xf, const float* __restrict__ prerot,
                                                     float* __restrict__ out) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= OUT * OUT / 4) return;
    const clibd_image_xform x = xf[b];
    if (!(x.flags & CLIBD_XF_ROTATE)) return;
    const bool hf = x.flags & CLIBD_XF_HFLIP, vf = x.flags & CLIBD_XF_VFLIP;
    const float half = 0.5f * OUT;
    const float t00 = x.theta[0] / half, t10 = x.theta[1] / half, t20 = x.theta[2] / half;
    const float t01 = x.theta[3] / half, t11 = x.theta[4] / half, t21 = x.theta[5] / half;
    const int y = q / (OUT / 4), x0 = (q - y * (OUT / 4)) * 4;
    const float yb = (float)y - (half - 0.5f);
    const float* src = prerot + (size_t)b * OUT * OUT * 3;
    f32x4 c0, c1, c2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xb = (float)(x0 + e) - (half - 0.5f);
        const float gx = xb * t00 + yb * t10 + t20;
        const float gy = xb * t01 + yb * t11 + t21;
        const float fx = rintf((gx + 1.f) * half - 0.5f), fy = rintf((gy + 1.f) * half - 0.5f);
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (fx >= 0.f && fx <= (float)(OUT - 1) && fy >= 0.f && fy <= (float)(OUT - 1)) {
            int ix = (int)fx, iy = (int)fy;
            if (hf) ix = OUT - 1 - ix;
            if (vf) iy = OUT - 1 - iy;
            const float* p = src + ((size_t)iy * OUT + ix) * 3;
            v0 = p[0];
            v1 = p[1];
            v2 = p[2];
        }
        c0[e] = v0;
        c1[e] = v1;
        c2[e] = v2;
    }
    float* o = out + ((size_t)b * 3 * OUT + y) * OUT + x0;
    *(f32x4*)o = c0;
    *(f32x4*)(o + (size_t)OUT * OUT) = c1;
    *(f32x4*)(o + (size_t)2 * OUT * OUT) = c2;
}

}  // namespace
}  // namespace clibd

using namespace clibd;

extern "C" size_t clibd_image_transform_workspace_bytes(int B) {
    return B <= 0 ? 0 : (size_t)B * (2 * kTableBytes + kPrerotBytes);
}

extern "C" int clibd_image_transform_u8(const void* data, size_t data_bytes, const clibd_image_xform* xforms, int B, float* out_f32,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!data || !xforms || !out_f32 || B <= 0 || B > 65535) return set_error(CLIBD_EINVAL, "image_transform_u8: bad args");
    if (((uintptr_t)xforms & 7) || !aligned16(out_f32) || !aligned16(workspace)) return set_error(CLIBD_EINVAL, "image_transform_u8: alignment");
    if (!workspace || workspace_bytes < clibd_image_transform_workspace_bytes(B))
        return set_error(CLIBD_EINVAL, "image_transform_u8: workspace missing or short");
    AxisTable* tables = (AxisTable*)workspace;
    float* prerot = (float*)((char*)workspace + (size_t)B * 2 * kTableBytes);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(axis_weights_kernel, dim3(B), dim3(256), 0, s, xforms, data_bytes, tables);
    hipLaunchKernelGGL(resample_kernel, dim3(OUT / RB, B), dim3(256), 0, s, (const unsigned char*)data, xforms, tables, prerot, out_f32);
    hipLaunchKernelGGL(rotate_kernel, dim3((OUT * OUT / 4 + 255) / 256, B), dim3(256), 0, s, xforms, prerot, out_f32);
    return check_launch("image_transform_u8");
}
