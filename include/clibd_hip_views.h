/*
 * clibd_hip_views.h — the SimCLR view generator of libclibd_hip.so (gfx950): the two augmented views of every image from its decoded
 * pixels (reference: get_simclr_pipeline_transform, bioscanclip/util/dataset.py:314-325: RandomResizedCrop(224) ->
 * RandomHorizontalFlip -> RandomApply([ColorJitter(0.8, 0.8, 0.8, 0.2)], 0.8) -> RandomGrayscale(0.2) -> GaussianBlur(21, (0.1, 2.0))
 * -> ToTensor).
 *
 * A third header beside clibd_hip.h and clibd_hip_simclr.h: the same library, the same conventions (extern "C", caller-owned device
 * buffers, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message, arguments validated on the host before any
 * launch).  The addition is purely additive — no entry of the other two headers changes its signature or its arithmetic — so the ABI
 * version stays 7.  The Python binding keeps these symbols under this header's name in clibd_amd._lib.HEADERS.
 */
#ifndef CLIBD_HIP_VIEWS_H
#define CLIBD_HIP_VIEWS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * One record per VIEW (a batch of b images is n = 2b records; several records may name the same pixels).  The host draws every random
 * parameter; the device does torchvision's tensor-path arithmetic for a float image in fp32, with no rounding between the stages:
 *   1. the box (top, left, h, w) of the H0 x W0 image -> 224 x 224 with torch's separable antialiased bilinear filter (taps clamped to
 *      the box; a 224 x 224 box is an exact copy), value = fp32(u8) / 255 (IEEE division); CLIBD_VIEW_HFLIP mirrors the columns;
 *   2. with CLIBD_VIEW_JITTER the four colour operations in the order of `order` (nibble j = the id applied j-th; a permutation of
 *      0 brightness, 1 contrast, 2 saturation, 3 hue), gray(x) = 0.2989 r + 0.587 g + 0.114 b, blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1):
 *        brightness blend(x, 0, f); contrast blend(x, m, f), m = the mean of gray over the 224 x 224 image as it stands when contrast is
 *        reached; saturation blend(x, gray(x), f); hue: rgb -> hsv, h <- (h + f) mod 1, hsv -> rgb with torchvision's formulas;
 *   3. with CLIBD_VIEW_GRAY all three channels become gray(x);
 *   4. always: the separable 21-tap Gaussian blur, w_k ~ exp(-(k / sigma)^2 / 2), k = -10 .. 10, normalised in fp32, reflect padding of
 *      10 (the edge is not repeated), columns first, then rows.
 * Limits: H0, W0 <= 65535; 1 <= h, w <= 3584 (at most 34 taps per output row / column); the box inside the image; the pixels inside
 * [0, data_bytes); `order` a permutation; sigma in [0.1, 2.0]; finite factors.  A record outside them yields a zero image, and no record
 * makes a kernel read outside the buffers.  No atomics: the contrast mean is summed from per-workgroup partials in a fixed order, so an
 * image's output depends on its pixels and its record only and repeats bit for bit.
 * workspace: clibd_simclr_views_workspace_bytes(n) bytes, 16-byte aligned; xf 8-byte, out 16-byte aligned.
 */
enum { CLIBD_VIEW_HFLIP = 1, CLIBD_VIEW_JITTER = 2, CLIBD_VIEW_GRAY = 4 };
enum { CLIBD_VIEW_OP_BRIGHTNESS = 0, CLIBD_VIEW_OP_CONTRAST = 1, CLIBD_VIEW_OP_SATURATION = 2, CLIBD_VIEW_OP_HUE = 3 };
typedef struct clibd_view_xform {
    int64_t offset;             /* byte offset of the image's pixels (packed RGB, HWC, uint8) in data */
    int32_t H0, W0;             /* decoded size */
    int32_t top, left, h, w;    /* crop box, resampled to 224 x 224 */
    int32_t flags;              /* CLIBD_VIEW_* */
    int32_t order;              /* four nibbles of CLIBD_VIEW_OP_* */
    float brightness, contrast, saturation, hue;   /* the factors (hue: the shift, in turns) */
    float sigma;                /* of the blur */
    int32_t reserved;           /* 0 */
} clibd_view_xform;             /* 64 bytes */
size_t clibd_simclr_views_workspace_bytes(int n_views_total);
int clibd_simclr_views_u8(const void* data, size_t data_bytes, const clibd_view_xform* xf, int n, float* out /*[n,3,224,224]*/,
                          void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_VIEWS_H */
