// jpeg_baseline.hpp — the front half of a decoder for baseline JPEG streams that were not written to be decoded in parallel (what
// libjpeg writes by default: Pillow's save(), cv2.imwrite), as __host__ __device__ functions: the segment walk into a per-stream
// descriptor, a bit source that lives across MCUs and byte-aligns at a restart, the whole-scan entropy decode, and block placement for
// 4:2:0 and 4:4:4.  The arithmetic behind the coefficients (dequantisation, inverse DCT, upsampling, colour) is jpeg_decode.hpp's,
// included and not restated.  The same text runs in jpeg_baseline.hip's kernels and, compiled for the host, behind
// srlhip_jpeg_probe_baseline / srlhip_jpeg_decode_baseline_host / jpeg_baseline_hostcheck.cpp.  The contract is written down in
// include/srlhip.h (srlhip_jpeg_decode_baseline).  Every function here reads a stream only inside the byte range it is handed.
#pragma once
#include "jpeg_decode.hpp"

namespace srljpegbase {

using namespace srljpegdec;

constexpr int kMaxSegments = 64;

// ---- the Annex K.3 tables as a DHT segment spells them ---------------------------------------------------------------------------
// kind 0 / 1: DC luminance / chrominance, 2 / 3: AC luminance / chrominance (DecTables' numbering, whose vals[] hold HUFFVAL)
struct K3Bits {
    uint8_t bits[4][16];
    uint8_t count[4];
};
constexpr K3Bits make_k3_bits() {
    K3Bits b{};
    for (int k = 0; k < 4; k++) {
        int n = 0;
        for (int i = 0; i < 16; i++) n += b.bits[k][i] = k < 2 ? srljpeg::kDcBits[k][i] : srljpeg::kAcBits[k - 2][i];
        b.count[k] = (uint8_t)n;
    }
    return b;
}

// ---- descriptor -------------------------------------------------------------------------------------------------------------------
// What the segment walk leaves of a stream's header.  sel: four bits per component c at 4 c — Tq (2 bits), then 1 when the component's
// DC table is the chrominance one, then the same for its AC table.
struct Desc {
    uint32_t data_start;       // offset of the first byte behind SOS
    uint32_t ri;               // restart interval in MCUs, 0 = none
    uint32_t sel;
    uint32_t sampling;         // 1: 4:2:0 (Y 2x2), 0: 4:4:4
    uint8_t q[4][64];          // the DQT tables by id, zigzag order
};
static_assert(sizeof(Desc) == 272 && sizeof(Desc) % 16 == 0, "descriptors lie back to back in the 16-byte aligned workspace");

JPEG_HD int sel_tq(uint32_t sel, int comp) { return (int)(sel >> (4 * comp)) & 3; }
JPEG_HD int sel_dc(uint32_t sel, int comp) { return (int)(sel >> (4 * comp + 2)) & 1; }
JPEG_HD int sel_ac(uint32_t sel, int comp) { return (int)(sel >> (4 * comp + 3)) & 1; }

// ---- geometry of the two sampling modes -------------------------------------------------------------------------------------------
struct Geo {
    int mw, nm;                // MCUs per row, MCUs in all
    int bpm, nblocks;          // blocks per MCU, blocks in all
    int ystride, cstride;      // bytes per row of the Y plane, of a chroma plane
    int cb_at, cr_at;          // where the Cb and Cr planes begin behind the Y plane
};
JPEG_HD Geo geo_of(int h, int w, int sampling) {
    Geo g;
    if (sampling) {
        g.mw = (w + 15) / 16; g.nm = g.mw * ((h + 15) / 16); g.bpm = 6;
        g.ystride = 16 * g.mw; g.cstride = 8 * g.mw; g.cb_at = 256 * g.nm; g.cr_at = 320 * g.nm;
    } else {
        g.mw = (w + 7) / 8; g.nm = g.mw * ((h + 7) / 8); g.bpm = 3;
        g.ystride = g.cstride = 8 * g.mw; g.cb_at = 64 * g.nm; g.cr_at = 128 * g.nm;
    }
    g.nblocks = g.bpm * g.nm;
    return g;
}
// the blocks a stream of these sides can have at most: the worse of the two modes (one call may mix them)
JPEG_HD int blocks_cap(int h, int w) {
    const int a = 6 * ((h + 15) / 16) * ((w + 15) / 16), b = 3 * ((h + 7) / 8) * ((w + 7) / 8);
    return a > b ? a : b;
}

// where block b (0 .. nblocks) of the scan lies inside the stream's planes: the byte offset of its first sample, its row stride
JPEG_HD void block_place_scan(const Geo &g, int sampling, int b, int *offset, int *stride) {
    const int m = b / g.bpm, blk = b - m * g.bpm, my = m / g.mw, mx = m - my * g.mw;
    if (sampling) {
        int plane;
        block_place(blk, my, mx, g.mw, &plane, offset, stride);
        *offset += plane == 0 ? 0 : plane == 1 ? g.cb_at : g.cr_at;
    } else {
        *stride = g.ystride;
        *offset = (blk == 0 ? 0 : blk == 1 ? g.cb_at : g.cr_at) + 8 * my * g.ystride + 8 * mx;
    }
}

// pixel (y, x) of a decoded stream: 4:2:0 through chroma_at, 4:4:4 with Cb and Cr taken at the pixel
JPEG_HD void pixel_rgb_scan(const uint8_t *pl, const Geo &g, int sampling, int h, int w, int y, int x, uint8_t *rgb) {
    if (sampling) {
        const Planes p{pl, pl + g.cb_at, pl + g.cr_at, g.ystride, g.cstride, (h + 1) / 2, (w + 1) / 2};
        pixel_rgb(p, y, x, rgb);
    } else {
        const size_t i = (size_t)y * g.ystride + x;
        ycc_to_rgb(pl[i], pl[g.cb_at + i], pl[g.cr_at + i], rgb);
    }
}

// ---- the segment walk -------------------------------------------------------------------------------------------------------------
// which K.3 table of class tc (0 DC, 1 AC) the n bytes at p (16 BITS, then HUFFVAL) spell: 0 luminance, 1 chrominance, -1 neither
JPEG_HD int k3_kind(const uint8_t *p, int n, int tc, const K3Bits &kb, const DecTables &t) {
    for (int j = 0; j < 2; j++) {
        const int k = 2 * tc + j;
        if (n != 16 + kb.count[k]) continue;
        bool same = true;
        for (int i = 0; i < 16; i++) same = same && p[i] == kb.bits[k][i];
        for (int i = 0; i < kb.count[k]; i++) same = same && p[16 + i] == t.vals[k][i];
        if (same) return j;
    }
    return -1;
}

// SOI and the marker segments up to SOS of s[0 .. len) -> ST_OK and *d, *img_h, *img_w; ST_EMPTY for len 0; else ST_HEADER.
JPEG_HD int parse_baseline(const uint8_t *s, int64_t len, const K3Bits &kb, const DecTables &t, Desc *d, int *img_h, int *img_w) {
    if (len <= 0) return ST_EMPTY;
    if (len < 4 || s[0] != 0xFF || s[1] != 0xD8) return ST_HEADER;
    uint32_t qdef = 0, hdef = 0;               // DQT ids seen; per (class, id) at 2 (2 class + id): 0 none, 1 luminance, 2 chrominance
    uint32_t tq = 0;                           // Tq of component c at 2 c
    bool have_sof = false;
    int sampling = 0;
    uint32_t ri = 0;
    int64_t pos = 2;
    for (int seg = 0; seg < kMaxSegments; seg++) {
        if (pos + 4 > len || s[pos] != 0xFF) return ST_HEADER;
        const int m = s[pos + 1], L = (s[pos + 2] << 8) | s[pos + 3];
        if (L < 2 || pos + 2 + L > len) return ST_HEADER;
        const uint8_t *p = s + pos + 4;
        int n = L - 2;
        if ((m >= 0xE0 && m <= 0xED) || m == 0xEF || m == 0xFE) {
            // skipped by its length
        } else if (m == 0xDB) {
            for (; n > 0; n -= 65, p += 65) {
                if (n < 65 || p[0] > 3) return ST_HEADER;          // (precision in the high nibble: 8 bits only)
                for (int i = 0; i < 64; i++) d->q[p[0]][i] = p[1 + i];
                qdef |= 1u << p[0];
            }
        } else if (m == 0xC0) {
            if (have_sof || n != 15 || p[0] != 8 || p[5] != 3) return ST_HEADER;
            *img_h = (p[1] << 8) | p[2];
            *img_w = (p[3] << 8) | p[4];
            if (!sides_ok(*img_h, *img_w)) return ST_HEADER;
            for (int c = 0; c < 3; c++) {
                const uint8_t *q = p + 6 + 3 * c;
                if (q[0] != c + 1 || q[2] > 3) return ST_HEADER;
                if (c == 0 ? (q[1] != 0x22 && q[1] != 0x11) : q[1] != 0x11) return ST_HEADER;
                tq |= (uint32_t)q[2] << (2 * c);
            }
            sampling = p[7] == 0x22;
            have_sof = true;
        } else if (m == 0xC4) {
            while (n > 0) {
                if (n < 17) return ST_HEADER;
                const int tc = p[0] >> 4, th = p[0] & 15;
                if (tc > 1 || th > 1) return ST_HEADER;
                int count = 0;
                for (int i = 0; i < 16; i++) count += p[1 + i];
                if (n < 17 + count) return ST_HEADER;
                const int kind = k3_kind(p + 1, 16 + count, tc, kb, t);
                if (kind < 0) return ST_HEADER;
                const int at = 2 * (2 * tc + th);
                hdef = (hdef & ~(3u << at)) | (uint32_t)(kind + 1) << at;
                p += 17 + count;
                n -= 17 + count;
            }
        } else if (m == 0xDD) {
            if (n != 2) return ST_HEADER;
            ri = ((uint32_t)p[0] << 8) | p[1];
        } else if (m == 0xDA) {
            if (!have_sof || n != 10 || p[0] != 3 || p[7] != 0 || p[8] != 63 || p[9] != 0) return ST_HEADER;
            uint32_t sel = 0;
            for (int c = 0; c < 3; c++) {
                const int td = p[2 + 2 * c] >> 4, ta = p[2 + 2 * c] & 15, q = (int)(tq >> (2 * c)) & 3;
                if (p[1 + 2 * c] != c + 1 || td > 1 || ta > 1) return ST_HEADER;
                const int dk = (int)(hdef >> (2 * td)) & 3, ak = (int)(hdef >> (2 * (2 + ta))) & 3;
                if (!dk || !ak || !((qdef >> q) & 1u)) return ST_HEADER;
                sel |= (uint32_t)(q | (dk - 1) << 2 | (ak - 1) << 3) << (4 * c);
            }
            d->data_start = (uint32_t)(pos + 2 + L);
            d->ri = ri;
            d->sel = sel;
            d->sampling = (uint32_t)sampling;
            return ST_OK;
        } else {
            return ST_HEADER;                  // APP14, SOF1.., DAC, DNL, RST, EOI, a fill byte: not the accepted layout
        }
        pos += 2 + L;
    }
    return ST_HEADER;                          // more than kMaxSegments segments
}

// ---- the bit source of a whole scan -----------------------------------------------------------------------------------------------
// The bits of s[pos .. end), most significant first, the 0x00 behind every 0xFF removed.  The stream's bytes are fetched in ALIGNED
// 16-byte pieces (one load each; a piece that reaches across the stream's first or last byte is put together from single bytes, so
// that nothing outside [s, s + end) is read) and the accumulator is refilled from the piece held in w0..w3.  An 0xFF that is followed
// by anything but 0x00, or by nothing, stops the fetch: `marker` remembers what followed (256: the stream's end), pos stays at the
// 0xFF, and the source hands out zeros and counts them.  A caller that consumed one of those has run past the data (overrun()).
// (every member function is inlined into its caller: a call would put the whole source into memory)
#define JPEG_HDI JPEG_HD __attribute__((always_inline))
struct ScanBits {
    const uint8_t *s;
    uint32_t pos, end, a0, cur;
    uint32_t w0, w1, w2, w3;
    uint32_t acc;
    int nbits, fake, marker;

    JPEG_HDI void open(const uint8_t *stream, uint32_t start, uint32_t len) {
        s = stream; pos = start; end = len;
        a0 = (uint32_t)(reinterpret_cast<uintptr_t>(stream) & 15u);
        cur = 0xFFFFFFFFu;
        w0 = w1 = w2 = w3 = acc = 0u;
        nbits = fake = 0;
        marker = -1;
    }
    JPEG_HDI void load(uint32_t piece) {
        const uint32_t lo = piece << 4;                          // in bytes from the aligned address at or below s
        cur = piece;
        if (lo >= a0 && lo + 16u <= a0 + end) {
            uint32_t w[4];
            __builtin_memcpy(w, __builtin_assume_aligned(s + (lo - a0), 16), 16);
            w0 = w[0]; w1 = w[1]; w2 = w[2]; w3 = w[3];
        } else {
            w0 = edge_word(lo); w1 = edge_word(lo + 4u); w2 = edge_word(lo + 8u); w3 = edge_word(lo + 12u);
        }
    }
    // four bytes of a piece that reaches across the stream's first or last byte, one load each, zeros outside the stream
    JPEG_HDI uint32_t edge_word(uint32_t at) const {
        uint32_t r = 0u;
        for (uint32_t i = 0; i < 4u; i++)
            if (at + i >= a0 && at + i < a0 + end) r |= (uint32_t)s[at + i - a0] << (8 * i);
        return r;
    }
    JPEG_HDI uint32_t byte(uint32_t p) {                           // p < end
        const uint32_t v = p + a0;
        if ((v >> 4) != cur) load(v >> 4);
        // the word is picked with masks, not with ?: — a select between two loaded members becomes a load from a selected address,
        // and that keeps the whole source in memory
        const uint32_t j = v & 15u, i = j >> 2;
        const uint32_t word = (w0 & (0u - (i == 0u))) | (w1 & (0u - (i == 1u))) | (w2 & (0u - (i == 2u))) | (w3 & (0u - (i == 3u)));
        return (word >> (8 * (j & 3u))) & 255u;
    }
    JPEG_HDI void refill() {                                      // -> at least 25 bits
        bool ff = false;                                          // the byte at pos is 0xFF and what follows it is looked at next
        while (nbits <= 24) {
            uint32_t b = 0;
            if (marker < 0) {
                const uint32_t p = pos + (ff ? 1u : 0u);
                if (p < end) {
                    const uint32_t v = byte(p);
                    if (!ff) {
                        if (v == 0xFFu) { ff = true; continue; }
                        b = v;
                        pos++;
                    } else {
                        ff = false;
                        if (v == 0u) { b = 0xFFu; pos += 2u; }
                        else marker = (int)v;
                    }
                } else {
                    marker = 256;
                }
            }
            if (marker >= 0) fake += 8;
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    JPEG_HDI uint32_t peek16() const { return (acc >> (nbits - 16)) & 0xFFFFu; }
    JPEG_HDI void skip(int n) { nbits -= n; }
    JPEG_HDI uint32_t take(int n) {                                // n <= 16
        nbits -= n;
        return (acc >> nbits) & ((1u << n) - 1u);
    }
    JPEG_HDI bool overrun() const { return nbits < fake; }
    // the k-th restart (k counted mod 8): the rest of the current byte is dropped, the next two bytes must be FF D0+k
    JPEG_HDI bool restart(int k) {
        if (nbits < fake || nbits - fake >= 8) return false;      // ran past the data; a whole data byte where the marker must stand
        if (marker < 0) {                                         // not met yet: the very next fetch must stop at it
            acc = 0u;
            nbits = fake = 0;
            refill();
            if (nbits != fake) return false;
        }
        if (marker != 0xD0 + k) return false;
        pos += 2u;
        marker = -1;
        acc = 0u;
        nbits = fake = 0;
        return true;
    }
};

// ---- the whole scan ---------------------------------------------------------------------------------------------------------------
// s[d.data_start .. len) -> coef[nblocks][64], dequantised, natural order, block b of the scan at 64 b.  coef must come in ZEROED: only
// non-zero coefficients are stored.  One symbol per trip of the one loop, from the state (block, k, component): lanes that decode
// different streams side by side run the same instructions whatever block each is in.  At most nblocks x 64 symbols are read whatever
// the data holds.  q3: the three components' quantisation tables [3][64] (fill_q3), wherever the caller keeps them close — a kernel in LDS:
// a table entry is read for every coefficient.  ST_OK or ST_DATA.
JPEG_HD void fill_q3(const Desc &d, uint8_t *q3) {
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 64; i++) q3[64 * c + i] = d.q[sel_tq(d.sel, c)][i];
}

JPEG_HD int decode_scan(const uint8_t *s, uint32_t len, const Desc &d, const uint8_t *q3, const Geo &g, const DecTables &t, int16_t *coef) {
    ScanBits b;
    b.open(s, d.data_start, len);
    const uint32_t sel = d.sel;
    int p0 = 0, p1 = 0, p2 = 0, pred = 0;                         // DC predictors: of Y, Cb, Cr, of the current component
    int blk = 0, comp = 0, k = 0, mcus_left = g.nm, rst = 0;
    const uint32_t ri = d.ri;
    uint32_t togo = ri;
    const uint8_t *q = q3;
    int dct = sel_dc(sel, 0), act = 2 + sel_ac(sel, 0);
    int16_t *c = coef;
    for (int trips = g.nblocks * 64; trips > 0; trips--) {
        const int sym = decode_symbol(b, t, k ? act : dct);
        if (sym < 0) return ST_DATA;
        bool block_ends = false;
        if (k == 0) {
            if (sym > 11) return ST_DATA;
            if (sym) pred += extend_bits(b, sym);
            if (pred) c[0] = dequant(pred, q[0]);
            k = 1;
        } else {
            const int run = sym >> 4, size = sym & 15;
            if (!size) {
                if (run != 15) block_ends = true;                 // EOB
                else if ((k += 16) > 63) return ST_DATA;          // ZRL: a coefficient has to follow
            } else {
                k += run;
                if (k > 63) return ST_DATA;
                c[t.zigzag[k]] = dequant(extend_bits(b, size), q[k]);
                block_ends = ++k == 64;
            }
        }
        if (!block_ends) continue;
        if (b.overrun()) return ST_DATA;
        if (comp == 0) p0 = pred; else if (comp == 1) p1 = pred; else p2 = pred;
        c += 64;
        k = 0;
        if (++blk == g.bpm) {
            blk = 0;
            if (--mcus_left == 0) return ST_OK;
            if (togo && --togo == 0) {
                if (!b.restart(rst)) return ST_DATA;
                rst = (rst + 1) & 7;
                togo = ri;
                p0 = p1 = p2 = 0;
            }
        }
        comp = blk < g.bpm - 2 ? 0 : blk - (g.bpm - 3);
        pred = comp == 0 ? p0 : comp == 1 ? p1 : p2;
        q = q3 + 64 * comp;
        dct = sel_dc(sel, comp);
        act = 2 + sel_ac(sel, comp);
    }
    return ST_DATA;                                               // (not reached: every trip ends a block or moves k forward)
}

// ---- Host: one whole stream -------------------------------------------------------------------------------------------------------
// scratch for decode_stream_baseline_host: coefficients and planes of the worse mode
inline size_t host_scratch_bytes_baseline(int img_h, int img_w) { return (size_t)blocks_cap(img_h, img_w) * (128 + 64); }

struct HostTables {
    DecTables dec = make_dec_tables();
    K3Bits k3 = make_k3_bits();
};
inline const HostTables &host_tables() {
    static const HostTables t;
    return t;
}

// Host: ST_OK and the sides / sampling (420 or 444) when the header of s[0 .. len) is accepted, else ST_HEADER / ST_EMPTY
inline int probe_baseline(const uint8_t *s, size_t len, int *img_h, int *img_w, int *sampling) {
    Desc d;
    const int st = parse_baseline(s, (int64_t)len, host_tables().k3, host_tables().dec, &d, img_h, img_w);
    if (st == ST_OK && sampling) *sampling = d.sampling ? 420 : 444;
    return st;
}

// -> ST_*; pixel (y, x) at out + (y * img_w + x) * pix_stride, three bytes; zeros unless ST_OK.  scratch: 2-byte aligned.
inline int decode_stream_baseline_host(const uint8_t *s, size_t len, int img_h, int img_w, uint8_t *out, int pix_stride, uint8_t *scratch) {
    const HostTables &t = host_tables();
    Desc d;
    int h = 0, w = 0;
    int st = parse_baseline(s, (int64_t)len, t.k3, t.dec, &d, &h, &w);
    if (st == ST_OK && (h != img_h || w != img_w)) st = ST_HEADER;
    if (st == ST_OK && len >= (size_t)kMaxStreamBytes) st = ST_DATA;
    Geo g = geo_of(img_h, img_w, st == ST_OK ? (int)d.sampling : 1);
    int16_t *coef = reinterpret_cast<int16_t *>(scratch);
    uint8_t *planes = scratch + 128 * (size_t)blocks_cap(img_h, img_w);
    if (st == ST_OK) {
        uint8_t q3[192];
        fill_q3(d, q3);
        memset(coef, 0, 128 * (size_t)g.nblocks);
        st = decode_scan(s, (uint32_t)len, d, q3, g, t.dec, coef);
    }
    if (st != ST_OK) {
        for (size_t i = 0; i < (size_t)img_h * img_w; i++) out[i * pix_stride] = out[i * pix_stride + 1] = out[i * pix_stride + 2] = 0;
        return st;
    }
    int32_t ws[64];
    for (int b = 0; b < g.nblocks; b++) {
        int offset, stride;
        block_place_scan(g, (int)d.sampling, b, &offset, &stride);
        idct_block(coef + 64 * (size_t)b, ws, planes + offset, stride);
    }
    for (int y = 0; y < img_h; y++)
        for (int x = 0; x < img_w; x++) pixel_rgb_scan(planes, g, (int)d.sampling, img_h, img_w, y, x, out + ((size_t)y * img_w + x) * pix_stride);
    return ST_OK;
}

}  // namespace srljpegbase
