// jpeg.hpp — the baseline JPEG encoder's per-MCU work (colour conversion, chroma downsampling, forward DCT, quantisation, entropy
// coding) as __host__ __device__ functions: the same text runs in jpeg.hip's kernels and, compiled for the host, behind
// srlhip_jpeg_encode_host / jpeg_hostcheck.cpp.  The arithmetic contract is written down in include/srlhip.h (srlhip_jpeg_encode).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif

namespace srljpeg {

constexpr int kHeaderBytes = 629;   // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14
constexpr int kMaxSide = 1024, kMinSide = 8;

// ---- tables of the JPEG specification (ITU-T T.81) ---------------------------------------------------------------------------
// Annex K.1 / K.2: luminance and chrominance quantisation tables, natural (row-major) order
constexpr uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Figure A.6: natural index of the i-th coefficient of the zigzag scan
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3: the "typical" Huffman tables, BITS (codes per length 1..16) and HUFFVAL
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// Everything the per-MCU functions look up, built once per call on the host (jpeg_build_tables) and handed to the kernels BY VALUE:
// a workgroup copies it into LDS.  huff entries are (code << 5) | length (Annex C: codes counted up within a length, shifted left
// between lengths); index 0 of dc / ac = luminance, 1 = chrominance.  The quantiser divides by d = 8 t (the DCT's output carries
// three fraction bits): half[i] = d / 2 and recip[i] = ceil(2^32 / d) for the i-th coefficient of the ZIGZAG scan, so that
// x / d == (x * recip) >> 32 for every x < 2^15 the DCT can produce (x * (recip * d - 2^32) < 2^15 * 2^11 < 2^32).
struct Tables {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
    uint32_t recip[2][64];
    uint16_t half[2][64];
    uint8_t zigzag[64];
};

// libjpeg's quality rule on an Annex K base entry
JPEG_HD int quant_entry(int base, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    int t = (base * scale + 50) / 100;
    return t < 1 ? 1 : t > 255 ? 255 : t;
}

inline void build_huff(const uint8_t *bits, const uint8_t *vals, uint32_t *out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < bits[len - 1]; i++) out[vals[k++]] = (code++ << 5) | (uint32_t)len;
        code <<= 1;
    }
}

inline void build_tables(int quality, Tables *t) {
    *t = Tables();
    for (int c = 0; c < 2; c++) {
        build_huff(kDcBits[c], kDcVals, t->dc[c]);
        build_huff(kAcBits[c], kAcVals[c], t->ac[c]);
        for (int i = 0; i < 64; i++) {
            const uint32_t d = 8u * (uint32_t)quant_entry(kBaseQ[c][kZigzag[i]], quality);
            t->half[c][i] = (uint16_t)(d / 2);
            t->recip[c][i] = (uint32_t)(((1ull << 32) + d - 1) / d);
        }
    }
    for (int i = 0; i < 64; i++) t->zigzag[i] = kZigzag[i];
}

// The kHeaderBytes in front of the entropy-coded data: SOI, APP0 (JFIF 1.01, no units, 1:1), DQT 0 / 1 (8-bit, zigzag order), SOF0
// (Y 2x2, Cb 1x1, Cr 1x1), DHT DC0 AC0 DC1 AC1, DRI (1 MCU), SOS.
inline int write_header(uint8_t *o, int img_h, int img_w, int quality) {
    int n = 0;
    auto put = [&](std::initializer_list<int> b) { for (int v : b) o[n++] = (uint8_t)v; };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; c++) {
        put({0xFF, 0xDB, 0, 67, c});
        for (int i = 0; i < 64; i++) o[n++] = (uint8_t)quant_entry(kBaseQ[c][kZigzag[i]], quality);
    }
    put({0xFF, 0xC0, 0, 17, 8, img_h >> 8, img_h & 255, img_w >> 8, img_w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int c = 0; c < 2; c++) {
        put({0xFF, 0xC4, 0, 19 + 12, 0x00 | c});
        for (int i = 0; i < 16; i++) o[n++] = kDcBits[c][i];
        for (int i = 0; i < 12; i++) o[n++] = kDcVals[i];
        put({0xFF, 0xC4, 0, 19 + 162, 0x10 | c});
        for (int i = 0; i < 16; i++) o[n++] = kAcBits[c][i];
        for (int i = 0; i < 162; i++) o[n++] = kAcVals[c][i];
    }
    put({0xFF, 0xDD, 0, 4, 0, 1});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return n;
}

// ---- per-MCU work ---------------------------------------------------------------------------------------------------------------
// One 8x8 block of int16 in the caller's storage: element k at p[k * stride] (a kernel lane: stride = workgroup size, the block
// lives in LDS with lanes interleaved; the host: stride 1).
struct Block {
    int16_t *p;
    int stride;
    JPEG_HD int16_t &operator[](int k) const { return p[k * stride]; }
};

// the image as the MCU functions read it: pixel (y, x) of the stream at px + (y * w + x) * pix_stride, three bytes R G B;
// coordinates past the frame are clamped (edge replication)
struct Image {
    const uint8_t *px;
    int h, w, pix_stride;
    JPEG_HD const uint8_t *at(int y, int x) const {
        y = y < h ? y : h - 1;
        x = x < w ? x : w - 1;
        return px + ((size_t)y * w + x) * pix_stride;
    }
};

JPEG_HD int luma(const uint8_t *p) { return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16; }
JPEG_HD int chroma_b(const uint8_t *p) { return (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + (128 << 16) + 32767) >> 16; }
JPEG_HD int chroma_r(const uint8_t *p) { return (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + (128 << 16) + 32767) >> 16; }

// 8-point DCT-II with the 13-bit matrix K[u][x] = round(4096 s(u) cos((2x + 1) u pi / 16)), s(0) = 1 / sqrt 2, s(u > 0) = 1, as exact
// integer sums (the even / odd split only reorders them), descaled by `shift` bits with round-to-nearest: (sum + 2^(shift-1)) >> shift,
// an arithmetic shift.
template <int SHIFT>
JPEG_HD void dct8(const Block &b, int base, int step) {
    constexpr int C1 = 4017, C2 = 3784, C3 = 3406, C4 = 2896, C5 = 2276, C6 = 1567, C7 = 799, R = 1 << (SHIFT - 1);
    const int s0 = b[base], s1 = b[base + step], s2 = b[base + 2 * step], s3 = b[base + 3 * step];
    const int s4 = b[base + 4 * step], s5 = b[base + 5 * step], s6 = b[base + 6 * step], s7 = b[base + 7 * step];
    const int a0 = s0 + s7, a1 = s1 + s6, a2 = s2 + s5, a3 = s3 + s4, b0 = s0 - s7, b1 = s1 - s6, b2 = s2 - s5, b3 = s3 - s4;
    b[base] = (int16_t)((C4 * (a0 + a1 + a2 + a3) + R) >> SHIFT);
    b[base + 4 * step] = (int16_t)((C4 * (a0 - a1 - a2 + a3) + R) >> SHIFT);
    b[base + 2 * step] = (int16_t)((C2 * (a0 - a3) + C6 * (a1 - a2) + R) >> SHIFT);
    b[base + 6 * step] = (int16_t)((C6 * (a0 - a3) - C2 * (a1 - a2) + R) >> SHIFT);
    b[base + step] = (int16_t)((C1 * b0 + C3 * b1 + C5 * b2 + C7 * b3 + R) >> SHIFT);
    b[base + 3 * step] = (int16_t)((C3 * b0 - C7 * b1 - C1 * b2 - C5 * b3 + R) >> SHIFT);
    b[base + 5 * step] = (int16_t)((C5 * b0 - C1 * b1 + C7 * b2 + C3 * b3 + R) >> SHIFT);
    b[base + 7 * step] = (int16_t)((C7 * b0 - C5 * b1 + C3 * b2 - C1 * b3 + R) >> SHIFT);
}

// level-shifted samples in, 8 x the orthonormal 2-D DCT out: rows first (descale 9: 16 x the 1-D transform, |value| <= 8034), then
// columns (descale 14; the sums stay below 2^28)
JPEG_HD void fdct(const Block &b) {
    for (int r = 0; r < 8; r++) dct8<9>(b, 8 * r, 1);
    for (int c = 0; c < 8; c++) dct8<14>(b, c, 8);
}

// Entropy-coded bytes of one MCU.  STORE = false only counts them (stuffing included).  A byte that would land at or past `end` is
// dropped, whatever the data: the caller sizes the destination from the count, the check makes that independent of its arithmetic.
template <bool STORE>
struct BitSink {
    uint8_t *out;
    const uint8_t *end;
    uint32_t len, acc;
    int nbits;
    JPEG_HD void byte(uint32_t v) {
        if (STORE) { if (out + len < end) out[len] = (uint8_t)v; }
        len++;
    }
    JPEG_HD void put(uint32_t code, int n) {       // n <= 16, fewer than 8 bits pending: 23 bits at most
        acc = (acc << n) | code;
        nbits += n;
        while (nbits >= 8) {
            const uint32_t v = (acc >> (nbits - 8)) & 255u;
            byte(v);
            if (v == 255u) byte(0);
            nbits -= 8;
        }
    }
    JPEG_HD void flush() { if (nbits) put((1u << (8 - nbits)) - 1u, 8 - nbits); }
};

JPEG_HD int bit_size(int a) {            // category of a magnitude: bits needed for |a|
    int n = 0;
    while (a) { n++; a >>= 1; }
    return n;
}

// quantise (round half away from zero: sign(c) * ((|c| + d / 2) / d), d = 8 t) and code one transformed block in zigzag order; returns
// the quantised DC (the next block's predictor)
template <bool STORE>
JPEG_HD int code_block(const Block &b, const Tables &t, int comp, int pred, BitSink<STORE> &s) {
    auto quant = [&](int i) {
        const int c = b[t.zigzag[i]];
        const uint32_t x = (uint32_t)(c < 0 ? -c : c) + t.half[comp][i];
        const int q = (int)(uint32_t)(((uint64_t)x * t.recip[comp][i]) >> 32);
        return c < 0 ? -q : q;
    };
    const int dc = quant(0);
    {
        const int diff = dc - pred, mag = diff < 0 ? -diff : diff, n = bit_size(mag);
        const uint32_t e = t.dc[comp][n];
        s.put(e >> 5, (int)(e & 31));
        if (n) s.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
    }
    int run = 0;
    for (int i = 1; i < 64; i++) {
        const int q = quant(i);
        if (!q) { run++; continue; }
        for (; run > 15; run -= 16) { const uint32_t z = t.ac[comp][0xF0]; s.put(z >> 5, (int)(z & 31)); }       // ZRL
        const int mag = q < 0 ? -q : q, n = bit_size(mag);
        const uint32_t e = t.ac[comp][(run << 4) | n];
        s.put(e >> 5, (int)(e & 31));
        s.put((uint32_t)(q < 0 ? q - 1 : q) & ((1u << n) - 1u), n);
        run = 0;
    }
    if (run) { const uint32_t e = t.ac[comp][0]; s.put(e >> 5, (int)(e & 31)); }                                   // EOB
    return dc;
}

// One 16x16 MCU at (my, mx): Y0 Y1 Y2 Y3 (DC predicted along that chain from 0), Cb, Cr (each from 0), padded to a byte with 1-bits.
// b0 / b1: two blocks of working storage.  Returns the byte count; with STORE they go to out[0 .. ) below `end`.
template <bool STORE>
JPEG_HD uint32_t encode_mcu(const Image &im, int my, int mx, const Tables &t, const Block &b0, const Block &b1, uint8_t *out, const uint8_t *end) {
    BitSink<STORE> s{out, end, 0u, 0u, 0};
    int pred = 0;
    for (int k = 0; k < 4; k++) {
        const int y0 = 16 * my + 8 * (k >> 1), x0 = 16 * mx + 8 * (k & 1);
        for (int y = 0; y < 8; y++)
            for (int x = 0; x < 8; x++) b0[8 * y + x] = (int16_t)(luma(im.at(y0 + y, x0 + x)) - 128);
        fdct(b0);
        pred = code_block<STORE>(b0, t, 0, pred, s);
    }
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++) {
            const uint8_t *p00 = im.at(16 * my + 2 * y, 16 * mx + 2 * x), *p01 = im.at(16 * my + 2 * y, 16 * mx + 2 * x + 1);
            const uint8_t *p10 = im.at(16 * my + 2 * y + 1, 16 * mx + 2 * x), *p11 = im.at(16 * my + 2 * y + 1, 16 * mx + 2 * x + 1);
            b0[8 * y + x] = (int16_t)(((chroma_b(p00) + chroma_b(p01) + chroma_b(p10) + chroma_b(p11) + 2) >> 2) - 128);
            b1[8 * y + x] = (int16_t)(((chroma_r(p00) + chroma_r(p01) + chroma_r(p10) + chroma_r(p11) + 2) >> 2) - 128);
        }
    fdct(b0);
    code_block<STORE>(b0, t, 1, 0, s);
    fdct(b1);
    code_block<STORE>(b1, t, 1, 0, s);
    s.flush();
    return s.len;
}

// what follows MCU m of n: RSTm (m mod 8), or EOI behind the last
JPEG_HD uint8_t mcu_trailer(int m, int n_mcus) { return (uint8_t)(m == n_mcus - 1 ? 0xD9 : 0xD0 + (m & 7)); }

// Host: one whole stream.  *len = the stream's size whether or not it fits; returns 0 when it was written, 1 when cap is too small
// (nothing is written then).
inline int encode_stream_host(const uint8_t *image, int img_h, int img_w, int pix_stride, int quality, uint8_t *out, size_t cap, size_t *len) {
    Tables t;
    build_tables(quality, &t);
    const Image im{image, img_h, img_w, pix_stride};
    const int mw = (img_w + 15) / 16, mh = (img_h + 15) / 16, nm = mw * mh;
    int16_t s0[64], s1[64];
    const Block b0{s0, 1}, b1{s1, 1};
    size_t total = kHeaderBytes;
    for (int m = 0; m < nm; m++) total += encode_mcu<false>(im, m / mw, m % mw, t, b0, b1, nullptr, nullptr) + 2;
    *len = total;
    if (total > cap) return 1;
    size_t at = (size_t)write_header(out, img_h, img_w, quality);
    for (int m = 0; m < nm; m++) {
        at += encode_mcu<true>(im, m / mw, m % mw, t, b0, b1, out + at, out + cap);
        out[at++] = 0xFF;
        out[at++] = mcu_trailer(m, nm);
    }
    return 0;
}

}  // namespace srljpeg
