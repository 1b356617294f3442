/*
 * clibd_hip_jpeg.h — baseline JPEG decode on the device in libclibd_hip.so (gfx950): the host plans a stream (markers, tables, sizes), the
 * device decodes its entropy-coded scan and reconstructs RGB HWC uint8 pixels into the packed buffer that clibd_image_transform_u8 and
 * clibd_simclr_views_u8 read.  The pixels are libjpeg's defaults (integer "islow" IDCT, "fancy" chroma upsampling, 16-bit fixed-point
 * YCbCr -> RGB), so they equal PIL's byte for byte for every stream the plan calls eligible and the device finishes with status 0.
 *
 * An eleventh header beside clibd_hip.h and the nine additive ones: the same library, the same conventions (extern "C", caller-owned
 * buffers, `void* stream`, 0 / negative CLIBD_E* status, clibd_last_error for the message prefixed by the entry's name, nothing allocates
 * or synchronises, arguments validated on the host before any launch).  The addition is purely additive — no entry of the other headers
 * changes its signature or its arithmetic — so the ABI version stays 7.  The Python binding keeps these symbols under this
 * header's name in clibd_amd._lib.HEADERS.
 *
 * No atomics: every output byte has one writer, so two runs agree bit for bit.
 */
#ifndef CLIBD_HIP_JPEG_H
#define CLIBD_HIP_JPEG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIBD_JPEG_PLAN_BYTES 4096 /* sizeof(struct clibd_jpeg_record) */

/* plan->reason: why the host path must decode the stream (0: the device takes it) */
#define CLIBD_JPEG_OK 0
#define CLIBD_JPEG_NOT_JPEG 1    /* no SOI: a PNG, an empty buffer */
#define CLIBD_JPEG_TRUNCATED 2   /* a header segment runs past the buffer, or no SOS before its end */
#define CLIBD_JPEG_SOF_KIND 3    /* any frame but SOF0: progressive, extended, lossless, arithmetic */
#define CLIBD_JPEG_PRECISION 4   /* samples of other than 8 bits */
#define CLIBD_JPEG_COMPONENTS 5  /* not three components: grayscale, CMYK */
#define CLIBD_JPEG_SAMPLING 6    /* luma not (1,1), (2,1) or (2,2), or a chroma component not (1,1) */
#define CLIBD_JPEG_COLORSPACE 7  /* libjpeg would not read the components as YCbCr */
#define CLIBD_JPEG_DQT 8         /* a 16-bit, missing or malformed quantisation table */
#define CLIBD_JPEG_DHT 9         /* a missing, over-subscribed or malformed Huffman table, an id above 1, a symbol outside baseline's range */
#define CLIBD_JPEG_SCAN 10       /* not one interleaved scan of all three components over coefficients 0..63 */
#define CLIBD_JPEG_SIZE 11       /* a zero side */
#define CLIBD_JPEG_MARKER 12     /* a marker or a segment length the planner does not understand */

/* status[i] of clibd_jpeg_decode_u8: 0, the plan's reason, or what stopped the device decode of the image (its slice is zero then) */
#define CLIBD_JPEG_EXHAUSTED 32  /* the data ended, or a marker came, before the last MCU was complete */
#define CLIBD_JPEG_BAD_CODE 33   /* bits that are no code of the Huffman table */
#define CLIBD_JPEG_COEF_INDEX 34 /* a run that carries the coefficient index past 63 */
#define CLIBD_JPEG_BAD_MARKER 35 /* not the expected RSTn between intervals or EOI after the last MCU */
#define CLIBD_JPEG_TRAILING 36   /* whole bytes of entropy-coded data left over where a marker is due: more MCUs than the frame holds */
#define CLIBD_JPEG_RANGE 37      /* values outside the range in which every libjpeg build computes the same pixels */
#define CLIBD_JPEG_BAD_PLAN 38   /* a record that contradicts itself or the buffer sizes of the call */

#define CLIBD_JPEG_444 0 /* plan->sampling */
#define CLIBD_JPEG_422 1
#define CLIBD_JPEG_420 2

/* A Huffman table in look-up form: look[next 8 bits] = length << 8 | symbol for codes of up to 8 bits, 0 for longer ones, which go
 * through maxcode / valoffset (length l: code <= maxcode[l] -> huffval[(code + valoffset[l]) & 255]). */
struct clibd_jpeg_huff {
    uint16_t look[256];
    int32_t maxcode[18];   /* [1..16]: the largest code of that length, -1 if none; [17]: a sentinel above every code */
    int32_t valoffset[18];
    uint8_t huffval[256];
};

/* One stream's record.  clibd_jpeg_plan fills everything but the three placement fields, which the caller sets when it packs a batch. */
struct clibd_jpeg_record {
    int32_t reason;            /* CLIBD_JPEG_OK or why not */
    int32_t H, W;              /* from SOF0, 1..65535 (set as soon as a frame header was read, eligible or not) */
    int32_t sampling;          /* CLIBD_JPEG_444 / 422 / 420 */
    int32_t mcus_x, mcus_y;    /* ceil(W / (8 hs)), ceil(H / (8 vs)) */
    int32_t blocks;            /* mcus_x * mcus_y * (hs * vs + 2): 8 x 8 blocks of all three components, padding included */
    int32_t restart_interval;  /* MCUs between RSTn, 0: none */
    int32_t scan_begin;        /* first byte of entropy-coded data, relative to the stream's start */
    int32_t stream_len;        /* bytes of the stream; the scan ends at its EOI, which the device finds */
    int64_t stream_begin;      /* placement: where the stream starts in `streams` */
    int64_t coef_begin;        /* placement: the image's first block in the workspace, in blocks */
    int32_t reserved0[2];
    uint8_t dc_sel[4], ac_sel[4], q_sel[4]; /* per component: which of huff[0..1] (DC), huff[2..3] (AC, as 0..1) and quant[0..1] it uses */
    uint8_t reserved1[4];
    uint16_t quant[2][64];     /* natural (row-major) order */
    struct clibd_jpeg_huff huff[4]; /* DC id 0, DC id 1, AC id 0, AC id 1 */
    uint8_t reserved2[112];
};

/* ------------------------------------------------------------------------------------------------
 * Host only, no GPU needed: walks the markers of data[0 .. len) up to the scan and fills *plan.  Every segment length is checked against
 * len.  Returns plan->reason (>= 0), or CLIBD_EINVAL for a null plan.  data may be NULL when len is 0 (CLIBD_JPEG_NOT_JPEG).
 * Eligible: SOF0, 8-bit, three components in one interleaved scan, 8-bit DQT, luma (1,1) / (2,1) / (2,2) over (1,1) chroma, a colour
 * space libjpeg reads as YCbCr (a JFIF APP0, or no Adobe APP14 and component ids 1, 2, 3), Huffman ids 0..1, with or without DRI.
 */
int clibd_jpeg_plan(const uint8_t* data, size_t len, struct clibd_jpeg_record* plan);

/* bytes of workspace for a batch whose eligible plans hold total_blocks blocks: int16 coefficients and uint8 component planes */
size_t clibd_jpeg_workspace_bytes(int64_t total_blocks);

/* ------------------------------------------------------------------------------------------------
 * Decodes the B images of a batch into out.
 *   streams       uint8 [stream_bytes] on the device: the eligible streams, each at its plan's stream_begin.
 *   plans         struct clibd_jpeg_record [B] on the device, 16-byte aligned.  A record with reason != 0 is skipped: status = reason, and
 *                 its slice of out is not touched (the caller puts the host-decoded pixels there).
 *   out, offsets  image i is written as RGB HWC uint8 at out[offsets[i] .. + 3 H W); offsets int64 [B] on the device.  Nothing outside
 *                 the slices is written.  A slice that does not lie inside [0, out_bytes) is not written (CLIBD_JPEG_BAD_PLAN).
 *   status        int32 [B] on the device, written for every image.  status != 0: the slice is all zeros (reason == 0) or untouched.
 *   workspace     16-byte aligned, at least clibd_jpeg_workspace_bytes(total_blocks); total_blocks >= every coef_begin + blocks.
 *   phases        1: entropy decode only, 2: reconstruction only (of what an earlier call decoded), 3: both.
 * Stream reads are bounded by [stream_begin, stream_begin + stream_len) and by stream_bytes, coefficient writes by the plan's block count
 * and by total_blocks: no value read out of a scan enters an address.  B <= 65535.
 */
int clibd_jpeg_decode_u8(const uint8_t* streams, int64_t stream_bytes, const struct clibd_jpeg_record* plans, int B, uint8_t* out,
                         int64_t out_bytes, const int64_t* offsets, int32_t* status, void* workspace, size_t workspace_bytes,
                         int64_t total_blocks, int phases, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIBD_HIP_JPEG_H */
