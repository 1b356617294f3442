// Baseline JPEG: the marker walk that fills a clibd_jpeg_record and the entropy decode of one scan, written once for host and device.
// Plain C++ with no HIP header, so the same text compiles into the library's kernels and into a host program under a sanitizer.
//
// Bounds.  Every byte of a stream is read through jpeg_fetch, which compares the position with the end it is given and answers 0 past
// it; it loads eight bytes at a time where eight remain, never a byte at or past the end.  Every coefficient is written through jpeg_store, which compares the block index with the block count it is given.  Both limits
// come from the caller (the buffer length, the plan's block count), never from the scan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/clibd_hip_jpeg.h"

#if defined(__HIPCC__)
#define CLIBD_JPEG_HD __host__ __device__ inline
#else
#define CLIBD_JPEG_HD inline
#endif

namespace clibd {
namespace jpeg {

// zigzag position -> natural (row-major) index
CLIBD_JPEG_HD int jpeg_natural(int k) {
    static constexpr uint8_t order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return order[k & 63];
}

// A stream and the eight bytes of it that were loaded last (a scan is a chain of dependent loads: one per eight bytes, not per byte).
// Positions are 32-bit: a stream is shorter than 2^31 bytes (the plan refuses longer ones).
struct Stream {
    const uint8_t* data;
    int end;            // bytes in data
    int word_pos;       // word holds data[word_pos .. word_pos + 8), the lowest byte first; bytes at or past `end` are zero in it
    uint64_t word;
};

CLIBD_JPEG_HD Stream jpeg_stream(const uint8_t* data, int64_t end) {
    return Stream{data, end < 0 ? 0 : end > 0x7FFFFFF0 ? 0x7FFFFFF0 : (int)end, -8, 0u};
}

// The one read of stream bytes: the `count` (1 or 4) bytes data[pos .. pos + count) as a little-endian number when all of them lie in
// [0, end), else 0 with *past set.
CLIBD_JPEG_HD unsigned jpeg_fetch(Stream& s, int pos, int count, int* past) {
    if (pos < 0 || count < 1 || count > 4 || pos > s.end - count) {
        *past = 1;
        return 0u;
    }
    if (pos < s.word_pos || pos + count > s.word_pos + 8) {
        uint64_t w = 0;
        if (pos <= s.end - 8) {
            __builtin_memcpy(&w, s.data + pos, 8);   // little endian on both sides
        } else {
            for (int i = 0; i < 8 && pos + i < s.end; ++i) w |= (uint64_t)s.data[pos + i] << (8 * i);
        }
        s.word = w;
        s.word_pos = pos;
    }
    const uint64_t v = s.word >> (8 * (pos - s.word_pos));
    return count == 4 ? (unsigned)v : (unsigned)v & 0xFFu;
}

// quant[slot] in zigzag order with the natural index beside it: value << 6 | natural index, what the scan needs per coefficient
CLIBD_JPEG_HD uint16_t jpeg_zq_entry(const clibd_jpeg_record* plan, int slot, int k) {
    const int nat = jpeg_natural(k);
    return (uint16_t)((plan->quant[slot & 1][nat] & 0xFFu) << 6 | nat);
}

// ---- the plan (host) ----------------------------------------------------------------------------------------------------------------
// libjpeg's jpeg_make_d_derived_tbl with its checks, plus baseline's symbol ranges; false: the table cannot be used
inline bool jpeg_build_huff(const uint8_t* bits /* [1..16] */, const uint8_t* vals, int total, bool is_dc, clibd_jpeg_huff* t) {
    uint8_t size[257];
    uint32_t code_of[256];
    if (total < 1 || total > 256) return false;
    int p = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < bits[l]; ++i) size[p++] = (uint8_t)l;
    size[p] = 0;
    uint32_t code = 0;
    int si = size[0];
    p = 0;
    while (size[p]) {
        while (size[p] == si) code_of[p++] = code++;
        if (code >= (1u << si)) return false;   // over-subscribed (libjpeg refuses a complete tree too)
        code <<= 1;
        ++si;
    }
    for (int i = 0; i < 256; ++i) {
        t->look[i] = 0;
        t->huffval[i] = 0;
    }
    for (int i = 0; i < total; ++i) {
        const int v = vals[i];
        if (is_dc ? v > 11 : ((v & 15) > 10 || ((v & 15) == 0 && v != 0x00 && v != 0xF0))) return false;
        t->huffval[i] = (uint8_t)v;
    }
    p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (bits[l]) {
            t->valoffset[l] = p - (int32_t)code_of[p];
            p += bits[l];
            t->maxcode[l] = (int32_t)code_of[p - 1];
        } else {
            t->valoffset[l] = 0;
            t->maxcode[l] = -1;
        }
    }
    t->maxcode[0] = -1;
    t->valoffset[0] = 0;
    t->maxcode[17] = 0xFFFFF;
    t->valoffset[17] = 0;
    p = 0;
    for (int l = 1; l <= 8; ++l)
        for (int i = 0; i < bits[l]; ++i, ++p) {
            const uint32_t first = code_of[p] << (8 - l);
            for (uint32_t c = 0; c < (1u << (8 - l)); ++c) t->look[(first + c) & 255] = (uint16_t)(l << 8 | vals[p]);
        }
    return true;
}

inline int jpeg_plan_stream(const uint8_t* data, size_t len_, clibd_jpeg_record* plan) {
    uint8_t* raw = (uint8_t*)plan;
    for (size_t i = 0; i < sizeof(clibd_jpeg_record); ++i) raw[i] = 0;
    const int64_t len = len_ > 0x7FFFFFF0u ? 0x7FFFFFF0 : (int64_t)len_;
    plan->stream_len = (int32_t)len;
    int past = 0;
    Stream in = jpeg_stream(data, len);
    auto byte = [&](int64_t pos) { return jpeg_fetch(in, pos > 0x7FFFFFF0 ? -1 : (int)pos, 1, &past); };
    auto done = [&](int reason) {
        plan->reason = reason;
        return reason;
    };
    if (len_ > 0x7FFFFFF0u) return done(CLIBD_JPEG_MARKER);
    if (len < 2 || byte(0) != 0xFF || byte(1) != 0xD8) return done(CLIBD_JPEG_NOT_JPEG);

    uint16_t qt[4][64];
    bool have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false};
    bool jfif = false, adobe = false, have_sof = false;
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {0, 0, 0}, comp_v[3] = {0, 0, 0}, comp_q[3] = {0, 0, 0};
    int64_t pos = 2;
    for (;;) {
        // a marker: FF, any number of fill FFs, the code
        if (byte(pos) != 0xFF) return done(past ? CLIBD_JPEG_TRUNCATED : CLIBD_JPEG_MARKER);
        while (byte(pos) == 0xFF) ++pos;
        if (past) return done(CLIBD_JPEG_TRUNCATED);
        const unsigned m = byte(pos++);
        if (m == 0xD9) return done(CLIBD_JPEG_TRUNCATED);   // EOI before any scan
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) return done(CLIBD_JPEG_MARKER);
        const int64_t seg = pos;                              // the two length bytes
        const int64_t L = (int64_t)(byte(pos) << 8 | byte(pos + 1));
        if (past || L < 2 || seg + L > len) return done(CLIBD_JPEG_TRUNCATED);
        const int64_t body = seg + 2, end = seg + L;
        pos = end;
        if (m == 0xE0) {                                      // APP0: JFIF
            if (L >= 16 && byte(body) == 'J' && byte(body + 1) == 'F' && byte(body + 2) == 'I' && byte(body + 3) == 'F' && byte(body + 4) == 0)
                jfif = true;
        } else if (m == 0xEE) {                               // APP14: Adobe
            if (L >= 14 && byte(body) == 'A' && byte(body + 1) == 'd' && byte(body + 2) == 'o' && byte(body + 3) == 'b' && byte(body + 4) == 'e')
                adobe = true;
        } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {   // other APPn, COM
        } else if (m == 0xDB) {                               // DQT
            int64_t q = body;
            while (q < end) {
                const unsigned pt = byte(q++);
                if ((pt >> 4) != 0) return done(CLIBD_JPEG_DQT);       // 16-bit entries
                if ((pt & 15) > 3 || q + 64 > end) return done(CLIBD_JPEG_DQT);
                for (int k = 0; k < 64; ++k) qt[pt & 15][jpeg_natural(k)] = (uint16_t)byte(q + k);
                for (int k = 0; k < 64; ++k)
                    if (qt[pt & 15][k] == 0) return done(CLIBD_JPEG_DQT);
                have_q[pt & 15] = true;
                q += 64;
            }
        } else if (m == 0xC4) {                               // DHT
            int64_t q = body;
            while (q < end) {
                const unsigned tc = byte(q++);
                if ((tc >> 4) > 1 || (tc & 15) > 1 || q + 16 > end) return done(CLIBD_JPEG_DHT);
                uint8_t bits[17], vals[256];
                int total = 0;
                bits[0] = 0;
                for (int l = 1; l <= 16; ++l) total += (bits[l] = (uint8_t)byte(q + l - 1));
                q += 16;
                if (total > 256 || q + total > end) return done(CLIBD_JPEG_DHT);
                for (int i = 0; i < total; ++i) vals[i] = (uint8_t)byte(q + i);
                q += total;
                const int slot = (int)(tc >> 4) * 2 + (int)(tc & 15);
                if (!jpeg_build_huff(bits, vals, total, (tc >> 4) == 0, &plan->huff[slot])) return done(CLIBD_JPEG_DHT);
                have_h[slot] = true;
            }
        } else if (m == 0xDD) {                               // DRI
            if (L != 4) return done(CLIBD_JPEG_MARKER);
            plan->restart_interval = (int32_t)(byte(body) << 8 | byte(body + 1));
        } else if (m == 0xC0) {                               // SOF0
            if (have_sof || L < 8) return done(CLIBD_JPEG_MARKER);
            have_sof = true;
            const unsigned prec = byte(body), nf = byte(body + 5);
            plan->H = (int32_t)(byte(body + 1) << 8 | byte(body + 2));
            plan->W = (int32_t)(byte(body + 3) << 8 | byte(body + 4));
            if (prec != 8) return done(CLIBD_JPEG_PRECISION);
            if (nf != 3) return done(CLIBD_JPEG_COMPONENTS);
            if (L != 8 + 3 * 3) return done(CLIBD_JPEG_MARKER);
            if (plan->H < 1 || plan->W < 1) return done(CLIBD_JPEG_SIZE);
            for (int c = 0; c < 3; ++c) {
                comp_id[c] = (int)byte(body + 6 + 3 * c);
                comp_h[c] = (int)(byte(body + 7 + 3 * c) >> 4);
                comp_v[c] = (int)(byte(body + 7 + 3 * c) & 15);
                comp_q[c] = (int)byte(body + 8 + 3 * c);
                if (comp_q[c] > 3) return done(CLIBD_JPEG_DQT);
            }
            if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) return done(CLIBD_JPEG_SAMPLING);
            if (comp_h[0] == 1 && comp_v[0] == 1) plan->sampling = CLIBD_JPEG_444;
            else if (comp_h[0] == 2 && comp_v[0] == 1) plan->sampling = CLIBD_JPEG_422;
            else if (comp_h[0] == 2 && comp_v[0] == 2) plan->sampling = CLIBD_JPEG_420;
            else return done(CLIBD_JPEG_SAMPLING);
        } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return done(CLIBD_JPEG_SOF_KIND);                 // SOF1..15: extended, progressive, lossless, arithmetic
        } else if (m == 0xDA) {                               // SOS
            if (!have_sof) return done(CLIBD_JPEG_MARKER);
            if (byte(body) != 3 || L != 6 + 2 * 3) return done(CLIBD_JPEG_SCAN);
            for (int c = 0; c < 3; ++c) {
                if ((int)byte(body + 1 + 2 * c) != comp_id[c]) return done(CLIBD_JPEG_SCAN);
                const unsigned t = byte(body + 2 + 2 * c);
                if ((t >> 4) > 1 || (t & 15) > 1) return done(CLIBD_JPEG_DHT);
                plan->dc_sel[c] = (uint8_t)(t >> 4);
                plan->ac_sel[c] = (uint8_t)(t & 15);
                if (!have_h[plan->dc_sel[c]] || !have_h[2 + plan->ac_sel[c]]) return done(CLIBD_JPEG_DHT);
            }
            if (byte(body + 7) != 0 || byte(body + 8) != 63 || byte(body + 9) != 0) return done(CLIBD_JPEG_SCAN);
            // libjpeg's colour-space rule for three components
            if (!jfif && (adobe || comp_id[0] != 1 || comp_id[1] != 2 || comp_id[2] != 3)) return done(CLIBD_JPEG_COLORSPACE);
            // at most two distinct quantisation tables
            int slot_id[2] = {comp_q[0], -1};
            for (int c = 0; c < 3; ++c) {
                if (!have_q[comp_q[c]]) return done(CLIBD_JPEG_DQT);
                if (comp_q[c] == slot_id[0]) plan->q_sel[c] = 0;
                else if (slot_id[1] < 0 || comp_q[c] == slot_id[1]) {
                    slot_id[1] = comp_q[c];
                    plan->q_sel[c] = 1;
                } else return done(CLIBD_JPEG_DQT);
            }
            for (int s = 0; s < 2; ++s)
                for (int k = 0; k < 64; ++k) plan->quant[s][k] = qt[slot_id[s] < 0 ? slot_id[0] : slot_id[s]][k];
            const int hs = comp_h[0], vs = comp_v[0];
            plan->mcus_x = (plan->W + 8 * hs - 1) / (8 * hs);
            plan->mcus_y = (plan->H + 8 * vs - 1) / (8 * vs);
            plan->blocks = plan->mcus_x * plan->mcus_y * (hs * vs + 2);   // <= 8192 * 8192 * 3 at (1,1): below 2^31
            plan->scan_begin = (int32_t)end;
            return done(CLIBD_JPEG_OK);
        } else {
            return done(CLIBD_JPEG_MARKER);                   // DAC, DNL, DHP, EXP, JPGn, reserved
        }
    }
}

// ---- the scan (host and device) -----------------------------------------------------------------------------------------------------
struct BitReader {
    Stream in;
    int pos;
    uint64_t buf;   // the next `n` bits of the scan sit in its low bits, the oldest highest
    int n;          // bits in buf
    int pad;        // how many of them, the youngest, are zeros that stand in for data that is not there
    int marker;     // the marker that ended the data (0: none yet); -1: the buffer ended
};

// Leaves more than 32 bits in the buffer: enough for one Huffman code (<= 16) and its value bits (<= 11) without another call.
CLIBD_JPEG_HD void br_fill(BitReader& r) {
    if (r.n > 32) return;
    if (r.marker == 0) {   // four bytes at once while none of them is an FF
        int past = 0;
        const unsigned w = jpeg_fetch(r.in, r.pos, 4, &past);
        if (!past && ((((w & 0x7F7F7F7Fu) + 0x01010101u) & w & 0x80808080u) == 0u)) {
            r.buf = (r.buf << 32) | (uint64_t)__builtin_bswap32(w);
            r.n += 32;
            r.pos += 4;
            return;
        }
    }
    while (r.n <= 56) {
        unsigned b = 0;
        if (r.marker == 0) {
            int past = 0;
            b = jpeg_fetch(r.in, r.pos, 1, &past);
            if (past) {
                r.marker = -1;
            } else {
                ++r.pos;
                if (b == 0xFF) {   // FF 00: a data FF; FF FF .. xx: fill bytes, then whatever xx is
                    unsigned c;
                    do {
                        c = jpeg_fetch(r.in, r.pos, 1, &past);
                        if (!past) ++r.pos;
                    } while (c == 0xFF && !past);
                    if (past) r.marker = -1;
                    else if (c != 0) r.marker = (int)c;
                }
            }
        }
        if (r.marker != 0) {
            b = 0;
            r.pad += 8;
        }
        r.buf = (r.buf << 8) | b;
        r.n += 8;
    }
}

// the next k bits (k <= 16) without consuming them; br_fill has run
CLIBD_JPEG_HD unsigned br_peek(const BitReader& r, int k) { return (unsigned)(r.buf >> (r.n - k)) & ((1u << k) - 1u); }

// false: the bits consumed were not all data
CLIBD_JPEG_HD bool br_drop(BitReader& r, int k) {
    r.n -= k;
    return r.n >= r.pad;
}

// one Huffman symbol (at least 16 bits are in the buffer); -1 bad code, -2 data exhausted
CLIBD_JPEG_HD int jpeg_symbol(BitReader& r, const clibd_jpeg_huff* t) {
    const unsigned look = t->look[br_peek(r, 8)];
    if (look) return br_drop(r, (int)(look >> 8)) ? (int)(look & 255u) : -2;
    int l = 9;
    int32_t code = (int32_t)br_peek(r, 9);
    while (l <= 16 && code > t->maxcode[l]) {
        ++l;
        code = (int32_t)br_peek(r, l > 16 ? 16 : l);
    }
    if (l > 16) return -1;
    if (!br_drop(r, l)) return -2;
    return (int)t->huffval[(code + t->valoffset[l]) & 255];
}

// s more bits as libjpeg's HUFF_EXTEND reads them (1 <= s <= 11, in the buffer); *ok cleared when the data ran out
CLIBD_JPEG_HD int jpeg_receive_extend(BitReader& r, int s, bool* ok) {
    const int x = (int)br_peek(r, s);
    if (!br_drop(r, s)) *ok = false;
    return x < (1 << (s - 1)) ? x - (1 << s) + 1 : x;
}

// the one write of coefficients: block `b` of an image that owns `blocks` blocks at coef
CLIBD_JPEG_HD void jpeg_store(int16_t* coef, int64_t b, int64_t blocks, int k, int v) {
    if (b >= 0 && b < blocks) coef[b * 64 + (k & 63)] = (int16_t)v;
}

// After an interval's last MCU: the left-over bits of the last byte go, then the marker `want` must follow.  0, or the status.
CLIBD_JPEG_HD int jpeg_expect_marker(BitReader& r, int want) {
    br_fill(r);
    if (r.n - r.pad >= 8) return CLIBD_JPEG_TRAILING;
    if (r.marker == -1) return CLIBD_JPEG_EXHAUSTED;
    return r.marker == want ? 0 : CLIBD_JPEG_BAD_MARKER;
}

// Decodes the scan of `plan` out of stream[0 .. stream_len) into coef (zeroed by the caller; `blocks` blocks of 64, natural order,
// dequantised).  zq: uint16 [2][64], jpeg_zq_entry of the plan's two quantisation tables.  Layout: the luma blocks as a plane of (mcus_y vs) x (mcus_x hs) blocks, then the Cb plane, then the Cr plane, each
// mcus_y x mcus_x.  Returns 0 or the status that stopped it.
CLIBD_JPEG_HD int jpeg_decode_scan(const uint8_t* stream, int64_t stream_len, const clibd_jpeg_record* plan, const uint16_t* zq, int16_t* coef,
                                   int64_t blocks) {
    const int hs = plan->sampling == CLIBD_JPEG_444 ? 1 : 2, vs = plan->sampling == CLIBD_JPEG_420 ? 2 : 1;
    const int mx = plan->mcus_x, my = plan->mcus_y;
    if (plan->sampling < 0 || plan->sampling > 2 || mx < 1 || my < 1 || mx > 8192 || my > 8192) return CLIBD_JPEG_BAD_PLAN;
    const int64_t mcus = (int64_t)mx * my;
    if (mcus * (hs * vs + 2) != (int64_t)plan->blocks || blocks < plan->blocks) return CLIBD_JPEG_BAD_PLAN;
    if (plan->scan_begin < 0 || plan->scan_begin > stream_len || plan->restart_interval < 0) return CLIBD_JPEG_BAD_PLAN;
    for (int c = 0; c < 3; ++c)
        if (plan->dc_sel[c] > 1 || plan->ac_sel[c] > 1 || plan->q_sel[c] > 1) return CLIBD_JPEG_BAD_PLAN;
    const int64_t cb_base = mcus * hs * vs, cr_base = cb_base + mcus;
    const int ri = plan->restart_interval;

    BitReader r = {jpeg_stream(stream, stream_len), plan->scan_begin, 0u, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    int todo = ri, rst = 0;   // MCUs left in the interval; the next RSTn's n
    int mx_ = 0, my_ = 0;     // the MCU's column and row
    for (int64_t m = 0; m < mcus; ++m) {
        if (ri && todo == 0) {
            if (int e = jpeg_expect_marker(r, 0xD0 + rst)) return e;
            r.buf = 0u;
            r.n = r.pad = r.marker = 0;
            pred[0] = pred[1] = pred[2] = 0;
            rst = (rst + 1) & 7;
            todo = ri;
        }
        --todo;
        if (m != 0 && ++mx_ == mx) {
            mx_ = 0;
            ++my_;
        }
        const int nb = hs * vs + 2;
        for (int i = 0; i < nb; ++i) {
            const int c = i < hs * vs ? 0 : i - hs * vs + 1;
            int64_t b;
            if (c == 0) b = ((int64_t)my_ * vs + i / hs) * ((int64_t)mx * hs) + (int64_t)mx_ * hs + i % hs;
            else b = (c == 1 ? cb_base : cr_base) + m;
            const clibd_jpeg_huff* dc = &plan->huff[plan->dc_sel[c]];
            const clibd_jpeg_huff* ac = &plan->huff[2 + plan->ac_sel[c]];
            const uint16_t* q = zq + 64 * plan->q_sel[c];
            bool ok = true;
            br_fill(r);
            int s = jpeg_symbol(r, dc);
            if (s < 0) return s == -1 ? CLIBD_JPEG_BAD_CODE : CLIBD_JPEG_EXHAUSTED;
            if (s > 11) return CLIBD_JPEG_BAD_CODE;
            if (s) pred[c] += jpeg_receive_extend(r, s, &ok);
            if (!ok) return CLIBD_JPEG_EXHAUSTED;
            int v = (int)(int16_t)pred[c] * (int)(q[0] >> 6);
            if (pred[c] < -32768 || pred[c] > 32767 || v < -32768 || v > 32767) return CLIBD_JPEG_RANGE;
            jpeg_store(coef, b, blocks, 0, v);
            for (int k = 1; k < 64;) {
                br_fill(r);
                const int rs = jpeg_symbol(r, ac);
                if (rs < 0) return rs == -1 ? CLIBD_JPEG_BAD_CODE : CLIBD_JPEG_EXHAUSTED;
                const int run = rs >> 4;
                s = rs & 15;
                if (s == 0) {
                    if (run != 15) break;   // EOB
                    k += 16;                // ZRL
                    if (k > 64) return CLIBD_JPEG_COEF_INDEX;
                    continue;
                }
                k += run;
                if (k > 63 || s > 10) return k > 63 ? CLIBD_JPEG_COEF_INDEX : CLIBD_JPEG_BAD_CODE;
                const int a = jpeg_receive_extend(r, s, &ok);
                if (!ok) return CLIBD_JPEG_EXHAUSTED;
                const int nat = q[k] & 63;
                v = a * (int)(q[k] >> 6);
                if (v < -32768 || v > 32767) return CLIBD_JPEG_RANGE;
                jpeg_store(coef, b, blocks, nat, v);
                ++k;
            }
        }
    }
    return jpeg_expect_marker(r, 0xD9);
}

}  // namespace jpeg
}  // namespace clibd
