// jpeg_decode.hpp — the decoder for the streams jpeg.hpp writes, as __host__ __device__ functions: header check, marker walk, per-MCU
// entropy decoding, inverse DCT, chroma upsampling and colour conversion.  The same text runs in jpeg_decode.hip's kernels and,
// compiled for the host, behind srlhip_jpeg_probe / srlhip_jpeg_decode_host / jpeg_decode_hostcheck.cpp.  The arithmetic contract is
// written down in include/srlhip.h (srlhip_jpeg_decode).  Every function here reads a stream only inside the byte range it is handed.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "jpeg.hpp"

namespace srljpegdec {

using srljpeg::kHeaderBytes;
using srljpeg::kMaxSide;
using srljpeg::kMinSide;

constexpr int ST_OK = 0, ST_HEADER = 1, ST_EMPTY = 2, ST_DATA = 3;
// where the header's variable parts lie: the two tables' 64 values each (zigzag order), the frame's sides (big endian)
constexpr int kDqtAt[2] = {25, 94}, kSidesAt = 163;
// no stream of the accepted layout is this long (4096 MCUs of 384 coefficients of at most 27 bits, stuffed: < 2^26 bytes)
constexpr int64_t kMaxStreamBytes = (int64_t)1 << 30;

// ---- Huffman decode tables of the four Annex K.3 codes, built at compile time ---------------------------------------------------
// table 0 / 1: DC luminance / chrominance, 2 / 3: AC luminance / chrominance.  look[t][next 9 bits] = (length << 8) | symbol for a
// code of at most 9 bits, 0 where the code is longer; the longer ones (10 .. 16 bits) are found by Annex F.2.2.3's walk: the first
// length whose maxcode is not below the leading bits, symbol vals[leading bits + valoff[length]].
constexpr int kLookBits = 9;
struct DecTables {
    uint16_t look[4][1 << kLookBits];
    int32_t maxcode[4][17];
    int32_t valoff[4][17];
    uint8_t vals[4][162];
    uint8_t zigzag[64];
};

constexpr DecTables make_dec_tables() {
    DecTables t{};
    for (int k = 0; k < 4; k++) {
        const uint8_t *bits = k < 2 ? srljpeg::kDcBits[k] : srljpeg::kAcBits[k - 2];
        const uint8_t *vals = k < 2 ? srljpeg::kDcVals : srljpeg::kAcVals[k - 2];
        const int n = k < 2 ? 12 : 162;
        for (int i = 0; i < n; i++) t.vals[k][i] = vals[i];
        int32_t code = 0;
        int at = 0;
        for (int len = 1; len <= 16; len++) {
            t.valoff[k][len] = at - code;
            for (int i = 0; i < bits[len - 1]; i++, code++, at++)
                if (len <= kLookBits)
                    for (int f = 0; f < (1 << (kLookBits - len)); f++)
                        t.look[k][(code << (kLookBits - len)) + f] = (uint16_t)((len << 8) | vals[at]);
            t.maxcode[k][len] = bits[len - 1] ? code - 1 : -1;
            code <<= 1;
        }
    }
    for (int i = 0; i < 64; i++) t.zigzag[i] = srljpeg::kZigzag[i];
    return t;
}

// ---- header ---------------------------------------------------------------------------------------------------------------------
// the header jpeg.hpp writes for these sides; the table values in it are not compared
inline void expected_header(int img_h, int img_w, uint8_t *out) { srljpeg::write_header(out, img_h, img_w, 50); }

JPEG_HD bool header_byte_is_compared(int i) { return !((i >= kDqtAt[0] && i < kDqtAt[0] + 64) || (i >= kDqtAt[1] && i < kDqtAt[1] + 64)); }

JPEG_HD bool sides_ok(int h, int w) { return h >= kMinSide && h <= kMaxSide && w >= kMinSide && w <= kMaxSide; }

// Host: 0 and the sides when `s[0 .. len)` starts with the accepted layout, else ST_HEADER (ST_EMPTY for len 0)
inline int probe_header(const uint8_t *s, size_t len, int *img_h, int *img_w) {
    if (len == 0) return ST_EMPTY;
    if (len < (size_t)kHeaderBytes) return ST_HEADER;
    const int h = (s[kSidesAt] << 8) | s[kSidesAt + 1], w = (s[kSidesAt + 2] << 8) | s[kSidesAt + 3];
    if (!sides_ok(h, w)) return ST_HEADER;
    uint8_t want[kHeaderBytes + 8];
    expected_header(h, w, want);
    for (int i = 0; i < kHeaderBytes; i++)
        if (header_byte_is_compared(i) && s[i] != want[i]) return ST_HEADER;
    *img_h = h;
    *img_w = w;
    return ST_OK;
}

// ---- markers --------------------------------------------------------------------------------------------------------------------
// Byte i of the data is a marker's first byte when it is 0xFF and the next byte of the stream is not the stuffed 0x00 (an 0xFF that
// ends the stream counts: there is nothing that could be its 0x00).  The accepted data holds exactly n_mcus of them: behind MCU k
// RST(k mod 8), behind the last one EOI as the stream's final two bytes.
JPEG_HD bool marker_at(const uint8_t *s, int64_t i, int64_t len) { return s[i] == 0xFF && (i + 1 >= len || s[i + 1] != 0x00); }

JPEG_HD bool marker_ok(const uint8_t *s, int64_t i, int64_t len, int64_t k, int n_mcus) {
    if (k >= n_mcus || i + 1 >= len) return false;
    if (k == n_mcus - 1 && i != len - 2) return false;
    return s[i + 1] == srljpeg::mcu_trailer((int)k, n_mcus);
}

// Host: the walk the scan kernel does in parallel.  ends[k] = offset of the marker behind MCU k; ST_OK or ST_DATA.
inline int find_mcus_host(const uint8_t *s, int64_t len, int n_mcus, int32_t *ends) {
    if (len >= kMaxStreamBytes) return ST_DATA;
    int64_t k = 0;
    for (int64_t i = kHeaderBytes; i < len; i++)
        if (marker_at(s, i, len)) {
            if (!marker_ok(s, i, len, k, n_mcus)) return ST_DATA;
            ends[k++] = (int32_t)i;
        }
    return k == n_mcus ? ST_OK : ST_DATA;
}

// ---- entropy decoding -----------------------------------------------------------------------------------------------------------
// The bits of s[pos .. end), most significant first, the 0x00 behind every 0xFF removed.  Past `end` the source hands out zeros and
// counts them; a caller that consumed one of those has run past the MCU's end (overrun()).
struct BitSource {
    const uint8_t *s;
    uint32_t pos, end, acc;
    int nbits, fake;
    bool bad;
    JPEG_HD void refill() {                       // -> at least 25 bits
        while (nbits <= 24) {
            uint32_t b = 0;
            if (pos < end) {
                b = s[pos++];
                if (b == 0xFFu) {
                    if (pos < end && s[pos] == 0x00) pos++;
                    else bad = true;
                }
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    JPEG_HD uint32_t peek16() const { return (acc >> (nbits - 16)) & 0xFFFFu; }
    JPEG_HD void skip(int n) { nbits -= n; }
    JPEG_HD uint32_t take(int n) {                // n <= 16
        nbits -= n;
        return (acc >> nbits) & ((1u << n) - 1u);
    }
    JPEG_HD bool overrun() const { return bad || nbits < fake; }
};

// one symbol of table k; -1 for sixteen bits that are no code.  Bits: BitSource, or another source with its refill / peek16 / skip / take
template <class Bits>
JPEG_HD int decode_symbol(Bits &b, const DecTables &t, int k) {
    b.refill();
    const uint32_t v = b.peek16();
    const uint32_t e = t.look[k][v >> (16 - kLookBits)];
    if (e) {
        b.skip((int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int len = kLookBits + 1; len <= 16; len++) {
        const int32_t code = (int32_t)(v >> (16 - len));
        if (code <= t.maxcode[k][len]) {
            b.skip(len);
            return t.vals[k][code + t.valoff[k][len]];
        }
    }
    return -1;
}

// the n bits behind a category code (the encoder's rule inverted: a value below 2^(n - 1) stands for v - 2^n + 1)
template <class Bits>
JPEG_HD int extend_bits(Bits &b, int n) {
    b.refill();
    const int v = (int)b.take(n);
    return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
}

// a coefficient times its table entry, kept in 16 bits (two's complement wrap: exact for everything the encoder writes)
JPEG_HD int16_t dequant(int v, int q) { return (int16_t)(uint16_t)((uint32_t)v * (uint32_t)q); }

// One MCU from s[start .. end): Y0 Y1 Y2 Y3 Cb Cr -> coef[6][64], dequantised, natural order.  coef must come in ZEROED: only
// non-zero coefficients are stored.  dqt: the stream's two tables.  Returns false on malformed data.  At most 6 x 64 symbols are
// read whatever the data holds.
JPEG_HD bool decode_mcu(const uint8_t *s, uint32_t start, uint32_t end, const uint8_t *dqt0, const uint8_t *dqt1, const DecTables &t, int16_t *coef) {
    BitSource b{s, start, end, 0u, 0, 0, false};
    int pred[3] = {0, 0, 0};
    for (int blk = 0; blk < 6; blk++) {
        const int comp = blk < 4 ? 0 : blk - 3, tab = comp ? 1 : 0;
        const uint8_t *q = tab ? dqt1 : dqt0;
        int16_t *c = coef + 64 * blk;
        const int n = decode_symbol(b, t, tab);
        if (n < 0 || n > 11) return false;
        if (n) pred[comp] += extend_bits(b, n);
        if (pred[comp]) c[0] = dequant(pred[comp], q[0]);
        for (int k = 1; k < 64;) {
            const int rs = decode_symbol(b, t, 2 + tab);
            if (rs < 0) return false;
            const int run = rs >> 4, size = rs & 15;
            if (!size) {
                if (run != 15) break;                 // EOB
                k += 16;                              // ZRL: a coefficient has to follow
                if (k > 63) return false;
                continue;
            }
            k += run;
            if (k > 63) return false;
            c[t.zigzag[k]] = dequant(extend_bits(b, size), q[k]);
            k++;
        }
        if (b.overrun()) return false;
    }
    return true;
}

// ---- inverse DCT ----------------------------------------------------------------------------------------------------------------
// libjpeg's "slow integer" 8-point inverse DCT: 13-bit constants round(c 2^13), output descaled by SHIFT bits with round-to-nearest
// ((x + 2^(SHIFT-1)) >> SHIFT, arithmetic).  Sums are 32-bit two's complement and wrap (exact for everything the encoder writes).
template <int SHIFT>
JPEG_HD void idct8(const int32_t *in, int stride, int32_t *out, int ostride) {
    constexpr uint32_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
                       F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172, R = 1u << (SHIFT - 1);
    const uint32_t i0 = (uint32_t)in[0], i1 = (uint32_t)in[stride], i2 = (uint32_t)in[2 * stride], i3 = (uint32_t)in[3 * stride];
    const uint32_t i4 = (uint32_t)in[4 * stride], i5 = (uint32_t)in[5 * stride], i6 = (uint32_t)in[6 * stride], i7 = (uint32_t)in[7 * stride];
    // even part
    const uint32_t e = (i2 + i6) * F0541, t2 = e - i6 * F1847, t3 = e + i2 * F0765;
    const uint32_t t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    // odd part
    const uint32_t z5 = (i7 + i3 + i5 + i1) * F1175;
    const uint32_t z1 = 0u - (i7 + i1) * F0899, z2 = 0u - (i5 + i3) * F2562;
    const uint32_t z3 = z5 - (i7 + i3) * F1961, z4 = z5 - (i5 + i1) * F0390;
    const uint32_t o0 = i7 * F0298 + z1 + z3, o1 = i5 * F2053 + z2 + z4, o2 = i3 * F3072 + z2 + z3, o3 = i1 * F1501 + z1 + z4;
    auto d = [&](uint32_t x) { return (int32_t)(x + R) >> SHIFT; };
    out[0] = d(t10 + o3);
    out[7 * ostride] = d(t10 - o3);
    out[ostride] = d(t11 + o2);
    out[6 * ostride] = d(t11 - o2);
    out[2 * ostride] = d(t12 + o1);
    out[5 * ostride] = d(t12 - o1);
    out[3 * ostride] = d(t13 + o0);
    out[4 * ostride] = d(t13 - o0);
}
constexpr int kPass1Shift = 11, kPass2Shift = 18;          // CONST_BITS - PASS1_BITS; CONST_BITS + PASS1_BITS + 3

// the sample of a descaled row-pass value: libjpeg's range-limit table on the value's low 10 bits (+128 and clamp to 0..255 for every
// value within -512..511; beyond that the table's index wraps, as libjpeg's does)
JPEG_HD uint8_t sample_of(int32_t v) {
    const int t = v & 1023;
    return (uint8_t)(t < 128 ? t + 128 : t < 512 ? 255 : t < 896 ? 0 : t - 896);
}

// one block: coef[64] (natural order) -> 8 rows of 8 samples at out + r * row_stride.  ws: 64 words of working storage.
JPEG_HD void idct_block(const int16_t *coef, int32_t *ws, uint8_t *out, int row_stride) {
    int32_t in[8], o[8];
    for (int c = 0; c < 8; c++) {
        for (int r = 0; r < 8; r++) in[r] = coef[8 * r + c];
        idct8<kPass1Shift>(in, 1, ws + c, 8);
    }
    for (int r = 0; r < 8; r++) {
        idct8<kPass2Shift>(ws + 8 * r, 1, o, 1);
        for (int c = 0; c < 8; c++) out[r * row_stride + c] = sample_of(o[c]);
    }
}

// ---- planes -> pixels -----------------------------------------------------------------------------------------------------------
// The decoded planes of one stream: Y [16 mh][16 mw], Cb and Cr [8 mh][8 mw], of which ch x cw = ceil(H / 2) x ceil(W / 2) are real.
struct Planes {
    const uint8_t *y, *cb, *cr;
    int ystride, cstride, ch, cw;
};

// where block `blk` (0..5) of MCU (my, mx) lies: plane 0 / 1 / 2 = Y / Cb / Cr, the byte offset of its first sample inside that plane
JPEG_HD void block_place(int blk, int my, int mx, int mw, int *plane, int *offset, int *stride) {
    if (blk < 4) {
        *plane = 0; *stride = 16 * mw;
        *offset = (16 * my + 8 * (blk >> 1)) * 16 * mw + 16 * mx + 8 * (blk & 1);
    } else {
        *plane = blk - 3; *stride = 8 * mw;
        *offset = 8 * my * 8 * mw + 8 * mx;
    }
}

// libjpeg's "fancy" h2v2 upsampling of one chroma plane at pixel (y, x): vertically 3 x the nearer row + 1 x the farther one, then
// horizontally 3 x the nearer column sum + 1 x the farther, + 8 (even x) or + 7 (odd x), >> 4.  The first and the last REAL column
// count themselves four times, rows past the real ones repeat the edge row.
JPEG_HD int chroma_at(const uint8_t *p, int stride, int ch, int cw, int y, int x) {
    const int r = y >> 1, c = x >> 1;
    const int far = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
    const uint8_t *n = p + (size_t)r * stride, *f = p + (size_t)far * stride;
    const int self = 3 * n[c] + f[c];
    if (x & 1) return c == cw - 1 ? (4 * self + 7) >> 4 : (3 * self + 3 * n[c + 1] + f[c + 1] + 7) >> 4;
    return c == 0 ? (4 * self + 8) >> 4 : (3 * self + 3 * n[c - 1] + f[c - 1] + 8) >> 4;
}

JPEG_HD uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// libjpeg's 16-bit fixed-point YCbCr -> RGB
JPEG_HD void ycc_to_rgb(int y, int cb, int cr, uint8_t *rgb) {
    cb -= 128;
    cr -= 128;
    rgb[0] = clamp255(y + ((91881 * cr + 32768) >> 16));
    rgb[1] = clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = clamp255(y + ((116130 * cb + 32768) >> 16));
}

JPEG_HD void pixel_rgb(const Planes &p, int y, int x, uint8_t *rgb) {
    ycc_to_rgb(p.y[(size_t)y * p.ystride + x], chroma_at(p.cb, p.cstride, p.ch, p.cw, y, x), chroma_at(p.cr, p.cstride, p.ch, p.cw, y, x), rgb);
}

// ---- Host: one whole stream ------------------------------------------------------------------------------------------------------
// -> ST_*; pixel (y, x) at out + (y * img_w + x) * pix_stride, three bytes; zeros unless ST_OK.  scratch: mcus * (4 + 768 + 384) bytes.
inline size_t host_scratch_bytes(int img_h, int img_w) {
    return (size_t)((img_h + 15) / 16) * ((img_w + 15) / 16) * (4 + 768 + 384);
}

inline int decode_stream_host(const uint8_t *s, size_t len, int img_h, int img_w, uint8_t *out, int pix_stride, uint8_t *scratch) {
    static constexpr DecTables tables = make_dec_tables();
    const int mw = (img_w + 15) / 16, mh = (img_h + 15) / 16, nm = mw * mh;
    int32_t *ends = reinterpret_cast<int32_t *>(scratch);
    int16_t *coef = reinterpret_cast<int16_t *>(scratch + 4 * (size_t)nm);
    uint8_t *planes = scratch + (4 + 768) * (size_t)nm;
    int h = 0, w = 0;
    int st = probe_header(s, len, &h, &w);
    if (st == ST_OK && (h != img_h || w != img_w)) st = ST_HEADER;
    if (st == ST_OK) st = find_mcus_host(s, (int64_t)len, nm, ends);
    if (st == ST_OK) {
        memset(coef, 0, 768 * (size_t)nm);
        for (int m = 0; m < nm && st == ST_OK; m++)
            if (!decode_mcu(s, m ? (uint32_t)ends[m - 1] + 2u : (uint32_t)kHeaderBytes, (uint32_t)ends[m], s + kDqtAt[0], s + kDqtAt[1], tables, coef + 384 * (size_t)m))
                st = ST_DATA;
    }
    if (st != ST_OK) {
        for (size_t i = 0; i < (size_t)img_h * img_w; i++) out[i * pix_stride] = out[i * pix_stride + 1] = out[i * pix_stride + 2] = 0;
        return st;
    }
    uint8_t *pl[3] = {planes, planes + 256 * (size_t)nm, planes + 320 * (size_t)nm};
    int32_t ws[64];
    for (int m = 0; m < nm; m++)
        for (int blk = 0; blk < 6; blk++) {
            int plane, offset, stride;
            block_place(blk, m / mw, m % mw, mw, &plane, &offset, &stride);
            idct_block(coef + 384 * (size_t)m + 64 * blk, ws, pl[plane] + offset, stride);
        }
    const Planes p{pl[0], pl[1], pl[2], 16 * mw, 8 * mw, (img_h + 1) / 2, (img_w + 1) / 2};
    for (int y = 0; y < img_h; y++)
        for (int x = 0; x < img_w; x++) pixel_rgb(p, y, x, out + ((size_t)y * img_w + x) * pix_stride);
    return ST_OK;
}

}  // namespace srljpegdec
