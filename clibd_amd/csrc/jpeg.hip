// Baseline JPEG decode for gfx950: the bytes of a batch's eligible streams in, RGB HWC uint8 pixels in the packed buffer of the image
// transforms out, equal to libjpeg's (PIL's) byte for byte.  The marker walk and the scan decode are jpeg_core.h, shared with the host.
//
// Entropy decode.  One lane per image: a Huffman scan is a serial chain of dependent loads (stream bytes, code look-up, quantiser),
// divergent between lanes from the first symbol on, so the time of a wave is the sum of what its active lanes do, not their maximum, and
// the time of the kernel is that of its slowest chain once every wave is resident.  Two consequences.  The images are spread thinly:
// `lanes` images per one-wave workgroup, the smallest power of two (at most 8) that keeps the grid within 8192 waves, eight per SIMD
// — one image per wave up to B = 8192; the other lanes only help to stage.  And the chain is kept short: the wave first copies each of
// its images' records (the four Huffman tables and the quantisers, 4 KiB) into LDS and builds the zigzag-ordered quantiser / natural
// index table there, so a symbol costs LDS look-ups, and stream bytes arrive eight per load (jpeg_core.h).  LDS: 4352 bytes per image,
// at most 34 KiB per workgroup.  Restart markers are handled inside the lane (DC reset, RSTn order); an image with restart intervals
// is not split over lanes.  Registers, scratch and LDS: DESIGN §3.15.
//
// Reconstruction.  idct: one thread per 8 x 8 block, both passes of libjpeg's jidctint.c in registers (64 + 64 ints, fully unrolled),
// the result as eight 8-byte rows of a padded component plane in the workspace.  colour: one thread per aligned 16 bytes of the output;
// it computes the six pixels those bytes belong to (fancy upsampling of chroma as jdsample.c, jdcolor.c's fixed-point tables), packs
// their 18 bytes and stores the 16 it owns with one store; the at most two partial chunks at the ends of a slice go byte by byte.
// Every byte has one writer; nothing is accumulated.
//
// Range.  libjpeg's SIMD and C forms agree only while the dequantised coefficients and the first pass's results stay far inside int16
// and the second pass's inside the range-limit table.  Valid images do by a wide margin; idct flags whatever does not
// (CLIBD_JPEG_RANGE) and the caller decodes that image on the host.
#include <hip/hip_runtime.h>

#include "../../include/clibd_hip.h"
#include "../../include/clibd_hip_jpeg.h"
#include "host_util.h"
#include "jpeg_core.h"

static_assert(sizeof(clibd_jpeg_record) == CLIBD_JPEG_PLAN_BYTES, "struct clibd_jpeg_record is 4096 bytes");
static_assert(sizeof(clibd_jpeg_huff) == 912, "struct clibd_jpeg_huff is 912 bytes");

namespace clibd {

constexpr int JPEG_THREADS = 256;
constexpr int JPEG_IDCT_GROUPS = 16;     // workgroups per image along x (grid-stride over its blocks)
constexpr int JPEG_COLOUR_GROUPS = 32;   // ... over its 16-byte chunks
constexpr int JPEG_MAX_LANES = 8;        // images per workgroup of the entropy kernel
constexpr int JPEG_MAX_WAVES = 8192;     // its grid while lanes < JPEG_MAX_LANES: eight waves for each of the chip's 1024 SIMDs
constexpr int JPEG_LDS_PER_IMAGE = CLIBD_JPEG_PLAN_BYTES + 2 * 64 * 2;
constexpr int JPEG_SAFE = 16383;         // |dequantised coefficient| and |first-pass result| up to which every libjpeg IDCT agrees

struct JpegGeom {
    int H, W, hs, vs, mx, my;
    long long mcus, coef_begin, out_off;
};

// The record against itself and against the sizes of the call; every kernel runs it before it forms an address from the record.
__device__ inline int jpeg_geom(const clibd_jpeg_record* p, long long stream_bytes, long long total_blocks, const int64_t* offsets, int i,
                                long long out_bytes, JpegGeom* g) {
    if (p->sampling < 0 || p->sampling > 2 || p->H < 1 || p->W < 1 || p->H > 65535 || p->W > 65535) return CLIBD_JPEG_BAD_PLAN;
    g->H = p->H;
    g->W = p->W;
    g->hs = p->sampling == CLIBD_JPEG_444 ? 1 : 2;
    g->vs = p->sampling == CLIBD_JPEG_420 ? 2 : 1;
    g->mx = (g->W + 8 * g->hs - 1) / (8 * g->hs);
    g->my = (g->H + 8 * g->vs - 1) / (8 * g->vs);
    g->mcus = (long long)g->mx * g->my;
    if (p->mcus_x != g->mx || p->mcus_y != g->my || (long long)p->blocks != g->mcus * (g->hs * g->vs + 2)) return CLIBD_JPEG_BAD_PLAN;
    g->coef_begin = p->coef_begin;
    if (g->coef_begin < 0 || g->coef_begin > total_blocks || (long long)p->blocks > total_blocks - g->coef_begin) return CLIBD_JPEG_BAD_PLAN;
    if (p->stream_begin < 0 || p->stream_len < 0 || p->stream_begin > stream_bytes || (long long)p->stream_len > stream_bytes - p->stream_begin)
        return CLIBD_JPEG_BAD_PLAN;
    g->out_off = offsets[i];
    const long long n = 3ll * g->H * g->W;
    if (g->out_off < 0 || g->out_off > out_bytes || n > out_bytes - g->out_off) return CLIBD_JPEG_BAD_PLAN;
    return 0;
}

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ streams, long long stream_bytes,
                                                          const clibd_jpeg_record* __restrict__ plans, int B, int lanes,
                                                          int16_t* __restrict__ coef, long long total_blocks,
                                                          const int64_t* __restrict__ offsets, long long out_bytes, int* __restrict__ status) {
    extern __shared__ uint4 staged[];   // per image of the workgroup: its record, then uint16 [2][64] of jpeg_zq_entry
    const int first = blockIdx.x * lanes;
    for (int slot = 0; slot < lanes && first + slot < B; ++slot) {
        const uint4* src = (const uint4*)(plans + first + slot);
        uint4* dst = staged + slot * (JPEG_LDS_PER_IMAGE / 16);
        for (int t = threadIdx.x; t < CLIBD_JPEG_PLAN_BYTES / 16; t += 64) dst[t] = src[t];
    }
    __syncthreads();
    for (int slot = 0; slot < lanes && first + slot < B; ++slot) {
        const clibd_jpeg_record* rec = (const clibd_jpeg_record*)(staged + slot * (JPEG_LDS_PER_IMAGE / 16));
        uint16_t* zq = (uint16_t*)((char*)rec + CLIBD_JPEG_PLAN_BYTES);
        zq[threadIdx.x] = jpeg::jpeg_zq_entry(rec, 0, threadIdx.x);
        zq[64 + threadIdx.x] = jpeg::jpeg_zq_entry(rec, 1, threadIdx.x);
    }
    __syncthreads();
    const int i = first + threadIdx.x;
    if ((int)threadIdx.x >= lanes || i >= B) return;
    const clibd_jpeg_record* p = (const clibd_jpeg_record*)(staged + threadIdx.x * (JPEG_LDS_PER_IMAGE / 16));
    int st = p->reason;
    if (st == 0) {
        JpegGeom g;
        st = jpeg_geom(p, stream_bytes, total_blocks, offsets, i, out_bytes, &g);
        if (st == 0)
            st = jpeg::jpeg_decode_scan(streams + p->stream_begin, p->stream_len, p, (const uint16_t*)((const char*)p + CLIBD_JPEG_PLAN_BYTES),
                                        coef + g.coef_begin * 64, p->blocks);
    }
    status[i] = st;
}

// ---- libjpeg's jpeg_idct_islow (jidctint.c), CONST_BITS 13, PASS1_BITS 2 -------------------------------------------------------------
// The sums run in unsigned arithmetic (the same bits, no signed overflow for the out-of-range inputs that are flagged afterwards).
__device__ __forceinline__ void islow_1d(const int in[8], int out[8], int shift) {
    typedef unsigned U;
    U z2 = (U)in[2], z3 = (U)in[6];
    U z1 = (z2 + z3) * 4433u;
    U tmp2 = z1 + z3 * (U)(-15137);
    U tmp3 = z1 + z2 * 6270u;
    z2 = (U)in[0];
    z3 = (U)in[4];
    U tmp0 = (z2 + z3) * 8192u;
    U tmp1 = (z2 - z3) * 8192u;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)in[7];
    tmp1 = (U)in[5];
    tmp2 = (U)in[3];
    tmp3 = (U)in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u;
    tmp1 *= 16819u;
    tmp2 *= 25172u;
    tmp3 *= 12299u;
    z1 *= (U)(-7373);
    z2 *= (U)(-20995);
    z3 *= (U)(-16069);
    z4 *= (U)(-3196);
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const U r = 1u << (shift - 1);
    out[0] = (int)(tmp10 + tmp3 + r) >> shift;
    out[7] = (int)(tmp10 - tmp3 + r) >> shift;
    out[1] = (int)(tmp11 + tmp2 + r) >> shift;
    out[6] = (int)(tmp11 - tmp2 + r) >> shift;
    out[2] = (int)(tmp12 + tmp1 + r) >> shift;
    out[5] = (int)(tmp12 - tmp1 + r) >> shift;
    out[3] = (int)(tmp13 + tmp0 + r) >> shift;
    out[4] = (int)(tmp13 - tmp0 + r) >> shift;
}

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const clibd_jpeg_record* __restrict__ plans, long long stream_bytes,
                                                                 const int16_t* __restrict__ coef, uint8_t* __restrict__ samples,
                                                                 long long total_blocks, const int64_t* __restrict__ offsets,
                                                                 long long out_bytes, int* __restrict__ status) {
    const int i = blockIdx.y;
    const clibd_jpeg_record* p = plans + i;
    // status[i] is read here while other workgroups of the same image may be storing CLIBD_JPEG_RANGE to it (below): an unsynchronised
    // read and write of one word, on purpose.  Whichever value is seen, the outcome is the same: a workgroup that sees the flag only
    // skips planes nobody will read, because the colour kernel, launched after this one, zeroes the slice of a flagged image.
    if (p->reason != 0 || status[i] != 0) return;
    JpegGeom g;
    if (jpeg_geom(p, stream_bytes, total_blocks, offsets, i, out_bytes, &g) != 0) return;
    const long long nY = g.mcus * g.hs * g.vs;
    const int nblocks = p->blocks;
    for (int blk = blockIdx.x * JPEG_THREADS + threadIdx.x; blk < nblocks; blk += gridDim.x * JPEG_THREADS) {
        const uint4* src = (const uint4*)(coef + (g.coef_begin + blk) * 64);
        int c[64], w[64];
        int worst = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint4 v = src[r];
            const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c[8 * r + 2 * k] = (int)(short)(u[k] & 0xFFFFu);
                c[8 * r + 2 * k + 1] = (int)(short)(u[k] >> 16);
            }
        }
#pragma unroll
        for (int k = 0; k < 64; ++k) worst = max(worst, iabs(c[k]));
#pragma unroll
        for (int col = 0; col < 8; ++col) {   // pass 1: columns
            int in[8], o[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) in[r] = c[8 * r + col];
            islow_1d(in, o, 11);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                w[8 * r + col] = o[r];
                worst = max(worst, iabs(o[r]));
            }
        }
        // where the block's samples go
        long long plane;
        int pitch_blocks, by, bx;
        if (blk < nY) {
            plane = 0;
            pitch_blocks = g.mx * g.hs;
            by = blk / pitch_blocks;
            bx = blk - by * pitch_blocks;
        } else {
            long long cblk = blk - nY;
            plane = nY;
            if (cblk >= g.mcus) {
                cblk -= g.mcus;
                plane += g.mcus;
            }
            pitch_blocks = g.mx;
            by = (int)(cblk / g.mx);
            bx = (int)(cblk - (long long)by * g.mx);
        }
        const size_t pitch = (size_t)pitch_blocks * 8;
        uint8_t* dst = samples + (size_t)(g.coef_begin + plane) * 64 + (size_t)by * 8 * pitch + (size_t)bx * 8;
        bool wide = false;
#pragma unroll
        for (int r = 0; r < 8; ++r) {         // pass 2: rows
            int in[8], o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) in[k] = w[8 * r + k];
            islow_1d(in, o, 18);
            unsigned lo = 0, hi = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                wide |= o[k] < -512 || o[k] > 511;
                const unsigned s = (unsigned)min(max(min(max(o[k], -512), 511) + 128, 0), 255);
                if (k < 4) lo |= s << (8 * k);
                else hi |= s << (8 * (k - 4));
            }
            *(uint2*)(dst + r * pitch) = make_uint2(lo, hi);
        }
        if (worst > JPEG_SAFE || wide) status[i] = CLIBD_JPEG_RANGE;   // every writer stores the same value
    }
}

// ---- upsampling (jdsample.c) and colour (jdcolor.c) ------------------------------------------------------------------------------------
struct ChromaPlanes {
    const uint8_t *y, *cb, *cr;
    size_t pitch_y, pitch_c;
    int dw, dh;      // the chroma planes' real width and height (libjpeg's downsampled_width / _height)
    int sampling;
    bool fancy;      // jinit_upsampler: triangle filter only when downsampled_width > 2, else replication
};

__device__ __forceinline__ int chroma_at(const ChromaPlanes& P, const uint8_t* c, int y, int x) {
    if (P.sampling == CLIBD_JPEG_444) return c[(size_t)y * P.pitch_c + x];
    const int j = x >> 1;
    if (P.sampling == CLIBD_JPEG_422) {
        const uint8_t* row = c + (size_t)y * P.pitch_c;
        if (!P.fancy) return row[j];
        if (x & 1) return j == P.dw - 1 ? row[j] : (3 * row[j] + row[j + 1] + 2) >> 2;
        return j == 0 ? row[0] : (3 * row[j] + row[j - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    if (!P.fancy) return c[(size_t)r * P.pitch_c + j];
    const int r1 = (y & 1) ? min(r + 1, P.dh - 1) : max(r - 1, 0);   // the context row; duplicated at the top and bottom edges
    const uint8_t* near = c + (size_t)r * P.pitch_c;
    const uint8_t* far = c + (size_t)r1 * P.pitch_c;
    const int j1 = (x & 1) ? min(j + 1, P.dw - 1) : max(j - 1, 0);
    const int here = 3 * near[j] + far[j], side = 3 * near[j1] + far[j1];
    return (3 * here + side + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

// R | G << 8 | B << 16 of pixel (y, x)
__device__ __forceinline__ unsigned pixel_rgb(const ChromaPlanes& P, int y, int x) {
    const int Y = P.y[(size_t)y * P.pitch_y + x];
    const int cb = chroma_at(P, P.cb, y, x) - 128, cr = chroma_at(P, P.cr, y, x) - 128;
    const int r = Y + ((91881 * cr + 32768) >> 16);
    const int g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    const int b = Y + ((116130 * cb + 32768) >> 16);
    return clamp255(r) | clamp255(g) << 8 | clamp255(b) << 16;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_colour_kernel(const clibd_jpeg_record* __restrict__ plans, long long stream_bytes,
                                                                   const uint8_t* __restrict__ samples, long long total_blocks,
                                                                   uint8_t* __restrict__ out, long long out_bytes,
                                                                   const int64_t* __restrict__ offsets, const int* __restrict__ status) {
    const int i = blockIdx.y;
    const clibd_jpeg_record* p = plans + i;
    if (p->reason != 0) return;                 // the host's slice
    JpegGeom g;
    if (jpeg_geom(p, stream_bytes, total_blocks, offsets, i, out_bytes, &g) != 0) return;
    const bool zero = status[i] != 0;
    const long long nY = g.mcus * g.hs * g.vs;
    ChromaPlanes P;
    P.y = samples + (size_t)g.coef_begin * 64;
    P.cb = P.y + (size_t)nY * 64;
    P.cr = P.cb + (size_t)g.mcus * 64;
    P.pitch_y = (size_t)g.mx * g.hs * 8;
    P.pitch_c = (size_t)g.mx * 8;
    P.dw = (g.W + g.hs - 1) / g.hs;
    P.dh = (g.H + g.vs - 1) / g.vs;
    P.sampling = p->sampling;
    P.fancy = P.dw > 2;
    const long long n = 3ll * g.H * g.W;
    const unsigned npix = (unsigned)g.H * (unsigned)g.W;   // < 2^32
    uint8_t* slice = out + g.out_off;
    const unsigned head = (unsigned)((uintptr_t)slice & 15u);        // bytes of the first chunk that precede the slice
    const long long chunks = (n + head + 15) / 16;
    for (long long ch = (long long)blockIdx.x * JPEG_THREADS + threadIdx.x; ch < chunks; ch += (long long)gridDim.x * JPEG_THREADS) {
        const long long first = ch * 16 - head;                      // the chunk's first byte, relative to the slice; >= -15
        unsigned long long w0 = 0, w1 = 0, w2 = 0;
        const long long shifted = first + 18;                        // a multiple of 3 keeps the phase
        const long long p0 = shifted / 3 - 6;                        // first pixel the chunk touches (may be -5 .. -1 at the head)
        const int phase = (int)(shifted - (shifted / 3) * 3);
        if (!zero) {
            long long pi = p0;
            int y = 0, x = 0;
            if (pi >= 0) {
                y = (int)((unsigned)pi / (unsigned)g.W);
                x = (int)((unsigned)pi - (unsigned)y * (unsigned)g.W);
            }
#pragma unroll
            for (int j = 0; j < 6; ++j, ++pi) {
                unsigned rgb = 0;
                if (pi >= 0 && pi < (long long)npix) {
                    if (pi == 0) y = x = 0;
                    rgb = pixel_rgb(P, y, x);
                    if (++x == g.W) {
                        x = 0;
                        ++y;
                    }
                }
                const int bit = 24 * j;                               // compile-time: where the pixel's three bytes sit in w0:w1:w2
                if (bit < 64) w0 |= (unsigned long long)rgb << bit;
                if (bit < 64 && bit + 24 > 64) w1 |= (unsigned long long)rgb >> (64 - bit);
                if (bit >= 64 && bit < 128) w1 |= (unsigned long long)rgb << (bit - 64);
                if (bit >= 64 && bit < 128 && bit + 24 > 128) w2 |= (unsigned long long)rgb >> (128 - bit);
                if (bit >= 128) w2 |= (unsigned long long)rgb << (bit - 128);
            }
        }
        unsigned long long lo = w0, hi = w1;
        if (phase != 0) {
            lo = (w0 >> (8 * phase)) | (w1 << (64 - 8 * phase));
            hi = (w1 >> (8 * phase)) | (w2 << (64 - 8 * phase));
        }
        if (first >= 0 && first + 16 <= n) {
            *(uint4*)(slice + first) = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long long at = first + k;
                if (at >= 0 && at < n) slice[at] = (uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFFu);
            }
        }
    }
}

}  // namespace clibd

using namespace clibd;

static inline bool aligned_to(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

extern "C" int clibd_jpeg_plan(const uint8_t* data, size_t len, struct clibd_jpeg_record* plan) {
    if (!plan) return set_error(CLIBD_EINVAL, "jpeg_plan: null pointer");
    if (!data && len != 0) return set_error(CLIBD_EINVAL, "jpeg_plan: null pointer");
    return jpeg::jpeg_plan_stream(data, len, plan);
}

extern "C" size_t clibd_jpeg_workspace_bytes(int64_t total_blocks) {
    if (total_blocks <= 0) return 0;
    Carver c(nullptr);
    c.take<int16_t>((size_t)total_blocks * 64);
    c.take<uint8_t>((size_t)total_blocks * 64);
    return c.total();
}

extern "C" int clibd_jpeg_decode_u8(const uint8_t* streams, int64_t stream_bytes, const struct clibd_jpeg_record* plans, int B, uint8_t* out,
                                    int64_t out_bytes, const int64_t* offsets, int32_t* status, void* workspace, size_t workspace_bytes,
                                    int64_t total_blocks, int phases, void* stream) {
    if (!streams || !plans || !out || !offsets || !status || !workspace) return set_error(CLIBD_EINVAL, "jpeg_decode_u8: null pointer");
    if (B <= 0) return set_error(CLIBD_EINVAL, "jpeg_decode_u8: non-positive batch");
    if (B > 65535) return set_error(CLIBD_EINVAL, "jpeg_decode_u8: batch above 65535");
    if (stream_bytes <= 0 || out_bytes <= 0 || total_blocks <= 0) return set_error(CLIBD_EINVAL, "jpeg_decode_u8: non-positive size");
    if (total_blocks > (1ll << 40)) return set_error(CLIBD_EINVAL, "jpeg_decode_u8: total_blocks too large");
    if (phases < 1 || phases > 3) return set_error(CLIBD_EINVAL, "jpeg_decode_u8: phases must be 1, 2 or 3");
    if (!aligned16(plans) || !aligned_to(offsets, 8) || !aligned_to(status, 4))
        return set_error(CLIBD_EINVAL, "jpeg_decode_u8: misaligned pointer (plans 16 bytes, offsets 8 bytes, status 4 bytes)");
    if (!aligned16(workspace) || workspace_bytes < clibd_jpeg_workspace_bytes(total_blocks))
        return set_error(CLIBD_EINVAL, "jpeg_decode_u8: workspace too small or misaligned (clibd_jpeg_workspace_bytes)");
    Carver c(workspace);
    int16_t* coef = c.take<int16_t>((size_t)total_blocks * 64);
    uint8_t* samples = c.take<uint8_t>((size_t)total_blocks * 64);
    hipStream_t st = (hipStream_t)stream;
    if (phases & 1) {
        if (hipMemsetAsync(coef, 0, (size_t)total_blocks * 128, st) != hipSuccess) return set_error(CLIBD_ELAUNCH, "jpeg_decode_u8: memset failed");
        int lanes = 1;
        while (lanes < JPEG_MAX_LANES && (B + lanes - 1) / lanes > JPEG_MAX_WAVES) lanes *= 2;
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((B + lanes - 1) / lanes)), dim3(64), (size_t)lanes * JPEG_LDS_PER_IMAGE, st, streams, (long long)stream_bytes, plans, B,
                           lanes, coef, (long long)total_blocks, offsets, (long long)out_bytes, (int*)status);
        if (int e = check_launch("jpeg_decode_u8 (entropy)")) return e;
    }
    if (phases & 2) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3(JPEG_IDCT_GROUPS, (unsigned)B), dim3(JPEG_THREADS), 0, st, plans, (long long)stream_bytes,
                           (const int16_t*)coef, samples, (long long)total_blocks, offsets, (long long)out_bytes, (int*)status);
        if (int e = check_launch("jpeg_decode_u8 (idct)")) return e;
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3(JPEG_COLOUR_GROUPS, (unsigned)B), dim3(JPEG_THREADS), 0, st, plans, (long long)stream_bytes,
                           (const uint8_t*)samples, (long long)total_blocks, out, (long long)out_bytes, offsets, (const int*)status);
        if (int e = check_launch("jpeg_decode_u8 (colour)")) return e;
    }
    return 0;
}
