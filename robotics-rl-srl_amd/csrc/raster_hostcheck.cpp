// raster_hostcheck.cpp — csrc/raster.hpp (the rasteriser's geometry: ray tests, screen footprints, the chunk walk — the text the
// kernels of raster.hip run) compiled for the host alone.  TESTS ONLY: `make rasterhostcheck`; tests/test_raster_footprint_cpu.py
// checks on it that every footprint covers the pixels its primitive's own exact test hits.
#include <string.h>

#include "raster.hpp"

using namespace srlraster;

namespace {

// prims travel as float[13]: type, r g b, a xyz, b xyz, rad, cs, sn; cameras as float[13]: eye, forward, right, up, tan_half_fov
Prim load_prim(const float *v) {
    Prim p;
    p.type = (int)v[0]; p.r = v[1]; p.g = v[2]; p.b = v[3]; p.ax = v[4]; p.ay = v[5]; p.az = v[6]; p.bx = v[7]; p.by = v[8]; p.bz = v[9];
    p.rad = v[10]; p.cs = v[11]; p.sn = v[12];
    return p;
}

Camera load_camera(const float *v) {
    Camera c;
    c.ex = v[0]; c.ey = v[1]; c.ez = v[2]; c.fx = v[3]; c.fy = v[4]; c.fz = v[5]; c.rx = v[6]; c.ry = v[7]; c.rz = v[8];
    c.ux = v[9]; c.uy = v[10]; c.uz = v[11]; c.tan_half_fov = v[12];
    return c;
}

// the unit ray of a pixel, built as raster_bg_k stores it
void ray_of(const Camera &c, int row, int col, int h, int w, float &dx, float &dy, float &dz) {
    float sx, sy;
    pixel_centre(c, row, col, h, w, sx, sy);
    pixel_ray(c, sx, sy, dx, dy, dz);
}

// the exact test raster_k runs for one (primitive, pixel)
float kernel_hit(const Prim &p, const CapsK &ck, const Camera &c, float dx, float dy, float dz, int &code) {
    return p.type == PRIM_CAPSULE ? hit_capsule_k(ck, dx, dy, dz, code) : hit_prim(p, c, dx, dy, dz, code);
}

uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

constexpr uint32_t kNoHit = 0xffffffffu;

}  // namespace

extern "C" {

// out[0..3]: kMaxPrims, kBandPixels, kTilePixels, kRasterBlock
void hostcheck_raster_constants(int32_t *out) { out[0] = kMaxPrims; out[1] = kBandPixels; out[2] = kTilePixels; out[3] = kRasterBlock; }

// which: 0 / 1 the Kuka cameras, 2 MobileRobot top-down, 3 the same over the 1-D arena, 4 the fpv camera of a robot at (x, y)
int hostcheck_raster_camera(int which, double x, double y, float *out13) {
    Camera cam[2], c;
    if (which == 0 || which == 1) { kuka_cameras(cam); c = cam[which]; }
    else if (which == 2 || which == 3) { mobile_cameras(which == 3, cam); c = cam[0]; }
    else if (which == 4) { mobile_cameras(false, cam); c = cam[1]; c.ex += (float)x; c.ey += (float)y; }      // as raster_tiles_k moves it
    else return -1;
    const float v[13] = {c.ex, c.ey, c.ez, c.fx, c.fy, c.fz, c.rx, c.ry, c.rz, c.ux, c.uy, c.uz, c.tan_half_fov};
    memcpy(out13, v, sizeof v);
    return 0;
}

// Per primitive b of prims [B][13], seen by one camera in an h x w image:
//   span_i [B][8]   r0 r1 c0 c1 W rpc cch inv_w                    (prim_span)
//   span_f [B][7]   xc0 kx hw, then the screen rectangle x0 x1 y0 y1 (prim_screen_rect)
//   P  [B][h*w]     1 where the kernel's own exact test of the pixel's ray returns t > 0
//   F  [B][h*w]     how often the object-order walk of raster_k visits the pixel (saturating at 255): the band loop with
//                   span_band_chunks / span_locate over every chunk, the four wavefronts' chunk sequences, all 64 lanes
//   Ft [B][h*w]     1 in the pixels of the 8x8 tiles whose mask includes the primitive on the tile path (raster_tiles_k)
//   walk [B][6]     visits; visits outside the image; visits outside their band; valid visits with rr >= rpc or i outside 0..W-1;
//                   bands in which the footprint has chunks; bands of the tile path with more tiles than tile_masks holds
//   caps (each may be null) ta / tk [B][h*w] float, ca / ck [B][h*w] int8: t and code of hit_capsule and of hit_capsule_k at every pixel
//                   (capsules only; code starts from 0 before either call)
void hostcheck_raster_footprints(const float *prims, int B, const float *cam13, int h, int w, int32_t *span_i, float *span_f,
                                 uint8_t *P, uint8_t *F, uint8_t *Ft, int32_t *walk, float *ta, float *tk, int8_t *ca, int8_t *ck) {
    const Camera c = load_camera(cam13);
    const size_t npix = (size_t)h * w;
    for (int b = 0; b < B; b++) {
        const Prim p = load_prim(prims + 13 * (size_t)b);
        Span s;
        CapsK kk;
        float rect[4];
        prim_span(p, c, w, h, s);
        prim_screen_rect(p, c, rect);
        memset(&kk, 0, sizeof kk);
        if (p.type == PRIM_CAPSULE) capsule_constants(p, c, kk);
        int32_t *si = span_i + 8 * (size_t)b;
        float *sf = span_f + 7 * (size_t)b;
        si[0] = s.r0; si[1] = s.r1; si[2] = s.c0; si[3] = s.c1; si[4] = s.W; si[5] = s.rpc; si[6] = s.cch; si[7] = s.inv_w;
        sf[0] = s.xc0; sf[1] = s.kx; sf[2] = s.hw; sf[3] = rect[0]; sf[4] = rect[1]; sf[5] = rect[2]; sf[6] = rect[3];
        uint8_t *Pb = P + npix * b, *Fb = F + npix * b, *Tb = Ft + npix * b;
        memset(Pb, 0, npix); memset(Fb, 0, npix); memset(Tb, 0, npix);
        for (int row = 0; row < h; row++)
            for (int col = 0; col < w; col++) {
                float dx, dy, dz;
                int code = 0;
                const size_t i = (size_t)row * w + col;
                ray_of(c, row, col, h, w, dx, dy, dz);
                Pb[i] = kernel_hit(p, kk, c, dx, dy, dz, code) > 0.0f;
                if (p.type == PRIM_CAPSULE && ta && tk && ca && ck) {
                    int c1 = 0, c2 = 0;
                    ta[npix * b + i] = hit_capsule(p, c.ex, c.ey, c.ez, dx, dy, dz, c1);
                    tk[npix * b + i] = hit_capsule_k(kk, dx, dy, dz, c2);
                    ca[npix * b + i] = (int8_t)c1; ck[npix * b + i] = (int8_t)c2;
                }
            }
        // object-order walk: the band loop of raster_k for this one primitive
        int32_t *wk = walk + 6 * (size_t)b;
        memset(wk, 0, 6 * sizeof(int32_t));
        const int band_rows = span_band_rows(w);
        for (int row0 = 0; row0 < h; row0 += band_rows) {
            const int rows = imin(band_rows, h - row0), last_row = row0 + rows - 1;
            const int chunks = span_band_chunks(s, row0, last_row);
            if (chunks > 0) wk[4]++;
            for (int wave = 0; wave < kRasterBlock / 64; wave++)
                for (int q = wave; q < chunks; q += kRasterBlock / 64)
                    for (int lane = 0; lane < 64; lane++) {
                        const SpanPixel px = span_locate(s, row0, last_row, q, lane);
                        if (!px.valid) continue;
                        wk[0]++;
                        if (px.rr >= s.rpc || px.i < 0 || px.i >= s.W) wk[3]++;
                        if (px.row < row0 || px.row > last_row) wk[2]++;
                        if (px.row < 0 || px.row >= h || px.col < 0 || px.col >= w) { wk[1]++; continue; }
                        uint8_t &f = Fb[(size_t)px.row * w + px.col];
                        if (f < 255) f++;
                    }
        }
        // tile path: the band / tile loops of raster_tiles_k
        const int tband = tile_band_rows(w), tiles_x = (w + 7) >> 3;
        const float inv_w2 = 2.0f / (float)w, inv_h2 = 2.0f / (float)h;
        for (int row0 = 0; row0 < h; row0 += tband) {
            const int rows = imin(tband, h - row0), ntiles = ((rows + 7) >> 3) * tiles_x;
            if (ntiles > kTilePixels / 64) wk[5]++;
            for (int t = 0; t < ntiles; t++) {
                const int tyy = t / tiles_x, txx = t - tyy * tiles_x, col0 = txx * 8, r0 = row0 + tyy * 8;
                if (!tile_overlaps(rect, tile_rect(c, r0, col0, inv_w2, inv_h2))) continue;
                for (int ly = 0; ly < 8; ly++)
                    for (int lx = 0; lx < 8; lx++)
                        if (r0 + ly < h && col0 + lx < w) Tb[(size_t)(r0 + ly) * w + col0 + lx] = 1;
            }
        }
    }
}

// A scene of np primitives (the first nstatic static, as raster_bg_k takes them) drawn three ways; per pixel the winner as
// (primitive << 3) | code, or -1 where nothing is hit:
//   full   every primitive in index order, nearer-than test (the z-test of raster_bg_k / trace)
//   walk   raster_k: static depth and winner first, then the moving primitives in object order over their footprints with the
//          64-bit min on (t, primitive, code) — the four wavefronts' chunk sequences one after the other
//   tiles  raster_tiles_k without a cached background: per 8x8 tile the primitives whose rectangle overlaps it, index order
int hostcheck_raster_scene(const float *prims13, int np, int nstatic, const float *cam13, int h, int w, int32_t *full, int32_t *walk, int32_t *tiles) {
    if (np < 1 || np > kMaxPrims || nstatic < 0 || nstatic > np || w > kBandPixels) return -1;
    const Camera c = load_camera(cam13);
    Prim prims[kMaxPrims];
    Span spans[kMaxPrims];
    CapsK capsk[kMaxPrims];
    float rects[kMaxPrims][4];
    for (int k = 0; k < np; k++) {
        prims[k] = load_prim(prims13 + 13 * k);
        prim_span(prims[k], c, w, h, spans[k]);
        prim_screen_rect(prims[k], c, rects[k]);
        if (prims[k].type == PRIM_CAPSULE) capsule_constants(prims[k], c, capsk[k]);
    }
    for (int row = 0; row < h; row++)
        for (int col = 0; col < w; col++) {
            float dx, dy, dz, best = 3.0e38f;
            int win = -1;
            ray_of(c, row, col, h, w, dx, dy, dz);
            for (int k = 0; k < np; k++) {
                int code;
                const float t = hit_prim(prims[k], c, dx, dy, dz, code);
                if (t > 0.0f && t < best) { best = t; win = (k << 3) | code; }
            }
            full[(size_t)row * w + col] = win;
        }
    // object order
    const int band_rows = span_band_rows(w);
    static thread_local unsigned long long zbuf[kBandPixels];
    for (int row0 = 0; row0 < h; row0 += band_rows) {
        const int rows = imin(band_rows, h - row0), count = rows * w, last_row = row0 + rows - 1;
        int chunks[kMaxPrims];
        for (int i = 0; i < count; i++) zbuf[i] = ~0ull;
        for (int k = nstatic; k < np; k++) chunks[k] = span_band_chunks(spans[k], row0, last_row);
        for (int wave = 0; wave < kRasterBlock / 64; wave++) {
            int k = nstatic, kbase = 0, kcnt = k < np ? chunks[k] : 0;
            for (int q = wave;; q += kRasterBlock / 64) {
                while (k < np && q >= kbase + kcnt) { kbase += kcnt; k++; kcnt = k < np ? chunks[k] : 0; }
                if (k >= np) break;
                for (int lane = 0; lane < 64; lane++) {
                    const SpanPixel px = span_locate(spans[k], row0, last_row, q - kbase, lane);
                    if (!px.valid) continue;
                    if (px.row < row0 || px.row > last_row || px.col < 0 || px.col >= w) return -2;
                    float dx, dy, dz, depth = 3.0e38f;
                    ray_of(c, px.row, px.col, h, w, dx, dy, dz);
                    for (int j = 0; j < nstatic; j++) {
                        int code;
                        const float t = hit_prim(prims[j], c, dx, dy, dz, code);
                        if (t > 0.0f && t < depth) depth = t;
                    }
                    int code = 0;
                    const float t = kernel_hit(prims[k], capsk[k], c, dx, dy, dz, code);
                    if (t > 0.0f && t < depth) {
                        const unsigned long long key = ((unsigned long long)float_bits(t) << 32) | (unsigned long long)((k << 3) | code);
                        unsigned long long &z = zbuf[(px.row - row0) * w + px.col];
                        if (key < z) z = key;
                    }
                }
            }
        }
        for (int i = 0; i < count; i++) {
            const int row = row0 + i / w, col = i % w;
            if ((uint32_t)zbuf[i] != kNoHit) { walk[(size_t)row * w + col] = (int32_t)((uint32_t)zbuf[i] & 0xffu); continue; }
            float dx, dy, dz, best = 3.0e38f;
            int win = -1;
            ray_of(c, row, col, h, w, dx, dy, dz);
            for (int k = 0; k < nstatic; k++) {
                int code;
                const float t = hit_prim(prims[k], c, dx, dy, dz, code);
                if (t > 0.0f && t < best) { best = t; win = (k << 3) | code; }
            }
            walk[(size_t)row * w + col] = win;
        }
    }
    // tile order
    const int tband = tile_band_rows(w), tiles_x = (w + 7) >> 3;
    const float inv_w2 = 2.0f / (float)w, inv_h2 = 2.0f / (float)h;
    for (int row0 = 0; row0 < h; row0 += tband) {
        const int rows = imin(tband, h - row0), ntiles = ((rows + 7) >> 3) * tiles_x;
        for (int t = 0; t < ntiles; t++) {
            const int tyy = t / tiles_x, txx = t - tyy * tiles_x, col0 = txx * 8, r0 = row0 + tyy * 8;
            const TileRect tr = tile_rect(c, r0, col0, inv_w2, inv_h2);
            uint32_t m = 0;
            for (int k = 0; k < np; k++)
                if (tile_overlaps(rects[k], tr)) m |= 1u << k;
            for (int ly = 0; ly < 8; ly++)
                for (int lx = 0; lx < 8; lx++) {
                    const int row = r0 + ly, col = col0 + lx;
                    if (row >= h || col >= w) continue;
                    float dx, dy, dz, best = 3.0e38f;
                    int win = -1;
                    ray_of(c, row, col, h, w, dx, dy, dz);
                    for (int k = 0; k < np; k++) {
                        if (!((m >> k) & 1u)) continue;
                        int code;
                        const float tt = hit_prim(prims[k], c, dx, dy, dz, code);
                        if (tt > 0.0f && tt < best) { best = tt; win = (k << 3) | code; }
                    }
                    tiles[(size_t)row * w + col] = win;
                }
        }
    }
    return 0;
}

}
