// raster.hpp — the geometry of the rasteriser (raster.hip) as __host__ __device__ functions: primitives, cameras, the exact
// ray tests, the conservative screen footprints and the (chunk, lane) -> pixel walk of the object-order path.  The same text runs
// in raster.hip's kernels and, compiled for the host, behind raster_hostcheck.cpp (tests/test_raster_footprint_cpu.py), which
// checks that the footprints really are conservative.  No HIP builtins; float32 throughout, compile with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RASTER_HD __host__ __device__ inline __attribute__((always_inline))
#define RASTER_HDN __host__ __device__ inline
#else
#define RASTER_HD inline
#define RASTER_HDN inline
#endif

namespace srlraster {

constexpr int kRasterBlock = 256;
constexpr int kMaxPrims = 28;   // Kuka scene 16 (full model: body + two finger + two tip capsules; lumped 14) + second button 2 or ten distractors + ball 11
constexpr int kTilePixels = 8192;       // LDS band buffer (24 KiB): whole 8-row tile strips, image width <= 1024
constexpr int kBandPixels = 2048;          // 16 KiB z-buffer + 4 KiB hit list: seven workgroups per CU

enum { PRIM_PLANE = 0, PRIM_BOX = 1, PRIM_CYL = 2, PRIM_CAPSULE = 3 };

struct Prim {
    int type;
    float r, g, b;
    float ax, ay, az;      // plane: (., ., z0)  box: centre  cylinder: base centre  capsule: end a
    float bx, by, bz;      // box: half extents             cylinder: (radius, ., height)  capsule: end b
    float rad;             // capsule radius
    float cs, sn;          // box: cos/sin of the yaw about z
};

struct Camera {
    float ex, ey, ez;      // eye
    float fx, fy, fz;      // forward (unit)
    float rx, ry, rz;      // right   (unit)
    float ux, uy, uz;      // up      (unit)
    float tan_half_fov;
};

RASTER_HD int imin(int a, int b) { return a < b ? a : b; }
RASTER_HD int imax(int a, int b) { return a > b ? a : b; }

// ---- ray / primitive intersection: returns t (> 0) or -1, and the surface normal ----------------------
// The hit functions return t only, plus a 3-bit `code` that says which face / part was hit: normals are evaluated once, for
// the nearest hit (prim_normal), not for every candidate — their divisions were a third of a capsule test.
//   box: axis | 4 when the face normal points along +axis;  cylinder: 0 side, 1 cap;  capsule: 0 body, 1 sphere at a, 2 sphere at b
RASTER_HD float hit_plane(const Prim &p, float oz, float dz) {
    if (dz == 0.0f) return -1.0f;
    const float t = (p.az - oz) / dz;
    return t > 0.0f ? t : -1.0f;
}

RASTER_HD float hit_box(const Prim &p, float ox, float oy, float oz, float dx, float dy, float dz, int &code) {
    // into the box frame (rotation about z by -yaw)
    const float px = ox - p.ax, py = oy - p.ay, pz = oz - p.az;
    const float lox = p.cs * px + p.sn * py, loy = p.cs * py - p.sn * px;
    const float ldx = p.cs * dx + p.sn * dy, ldy = p.cs * dy - p.sn * dx;
    float tmin = -3.0e38f, tmax = 3.0e38f;
    int axis = 0; float sign = 0.0f;
    const float o[3] = {lox, loy, pz}, d[3] = {ldx, ldy, dz}, h[3] = {p.bx, p.by, p.bz};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (d[k] == 0.0f) {
            if (o[k] < -h[k] || o[k] > h[k]) return -1.0f;
        } else {
            const float inv = 1.0f / d[k];
            float t0 = (-h[k] - o[k]) * inv, t1 = (h[k] - o[k]) * inv;
            float s = -1.0f;
            if (t0 > t1) { const float tt = t0; t0 = t1; t1 = tt; s = 1.0f; }
            if (t0 > tmin) { tmin = t0; axis = k; sign = s; }
            if (t1 < tmax) tmax = t1;
        }
    }
    if (tmin > tmax || tmin <= 0.0f) return -1.0f;
    code = axis | (sign > 0.0f ? 4 : 0);
    return tmin;
}

RASTER_HD float hit_cylinder(const Prim &p, float ox, float oy, float oz, float dx, float dy, float dz, int &code) {
    const float R = p.bx, z0 = p.az, z1 = p.az + p.bz;
    const float px = ox - p.ax, py = oy - p.ay;
    float best = -1.0f;
    const float a = dx * dx + dy * dy;
    if (a > 0.0f) {
        const float b = px * dx + py * dy, c = px * px + py * py - R * R;
        const float disc = b * b - a * c;
        if (disc >= 0.0f) {
            const float t = (-b - sqrtf(disc)) / a;
            const float z = oz + t * dz;
            if (t > 0.0f && z >= z0 && z <= z1) { best = t; code = 0; }
        }
    }
    if (dz != 0.0f) {       // caps (the top one is what a camera above ever sees)
        const float zc = dz < 0.0f ? z1 : z0;
        const float t = (zc - oz) / dz;
        if (t > 0.0f && (best < 0.0f || t < best)) {
            const float hx = px + t * dx, hy = py + t * dy;
            if (hx * hx + hy * hy <= R * R) { best = t; code = 1; }
        }
    }
    return best;
}

RASTER_HD float hit_capsule(const Prim &p, float ox, float oy, float oz, float dx, float dy, float dz, int &code) {
    const float bax = p.bx - p.ax, bay = p.by - p.ay, baz = p.bz - p.az;
    const float oax = ox - p.ax, oay = oy - p.ay, oaz = oz - p.az;
    const float baba = bax * bax + bay * bay + baz * baz;
    const float bard = bax * dx + bay * dy + baz * dz;
    const float baoa = bax * oax + bay * oay + baz * oaz;
    const float rdoa = dx * oax + dy * oay + dz * oaz;
    const float oaoa = oax * oax + oay * oay + oaz * oaz;
    const float a = baba - bard * bard;
    float b = baba * rdoa - baoa * bard;
    float c = baba * oaoa - baoa * baoa - p.rad * p.rad * baba;
    float h = b * b - a * c;
    if (h < 0.0f || baba == 0.0f) return -1.0f;
    float t = -1.0f, y = 0.0f;
    bool body = false;
    code = 0;
    if (a > 0.0f) {
        t = (-b - sqrtf(h)) / a;
        y = baoa + t * bard;
        body = y > 0.0f && y < baba;
    }
    if (!body) {            // one of the two end spheres
        const float ocx = y <= 0.0f ? oax : ox - p.bx, ocy = y <= 0.0f ? oay : oy - p.by, ocz = y <= 0.0f ? oaz : oz - p.bz;
        b = dx * ocx + dy * ocy + dz * ocz;
        c = ocx * ocx + ocy * ocy + ocz * ocz - p.rad * p.rad;
        h = b * b - c;
        if (h < 0.0f) return -1.0f;
        t = -b - sqrtf(h);
        code = y <= 0.0f ? 1 : 2;
    }
    if (t <= 0.0f) return -1.0f;
    return t;
}

RASTER_HD float hit_prim(const Prim &p, const Camera &c, float dx, float dy, float dz, int &code) {
    code = 0;
    if (p.type == PRIM_PLANE) return hit_plane(p, c.ez, dz);
    if (p.type == PRIM_BOX) return hit_box(p, c.ex, c.ey, c.ez, dx, dy, dz, code);
    if (p.type == PRIM_CYL) return hit_cylinder(p, c.ex, c.ey, c.ez, dx, dy, dz, code);
    return hit_capsule(p, c.ex, c.ey, c.ez, dx, dy, dz, code);
}

RASTER_HD void pixel_ray(const Camera &c, float sx, float sy, float &dx, float &dy, float &dz) {
    dx = c.fx + sx * c.rx + sy * c.ux; dy = c.fy + sx * c.ry + sy * c.uy; dz = c.fz + sx * c.rz + sy * c.uz;
    const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
    dx *= inv; dy *= inv; dz *= inv;
}

// tangent-space position of the centre of pixel (row, col) of an h x w image: what pixel_ray takes
RASTER_HD void pixel_centre(const Camera &c, int row, int col, int h, int w, float &sx, float &sy) {
    sx = (((float)col + 0.5f) / (float)w * 2.0f - 1.0f) * c.tan_half_fov;
    sy = (1.0f - ((float)row + 0.5f) / (float)h * 2.0f) * c.tan_half_fov;
}

// Conservative screen rectangle (tangent-space x = X/Z, y = Y/Z in the camera frame) of a primitive: the eight
// corners of its world-space bounding box are projected; anything reaching behind the near plane covers the screen.
RASTER_HDN void prim_screen_rect(const Prim &p, const Camera &c, float rect[4]) {
    float lo[3], hi[3];
    if (p.type == PRIM_PLANE) { rect[0] = -3.0e38f; rect[1] = 3.0e38f; rect[2] = -3.0e38f; rect[3] = 3.0e38f; return; }
    if (p.type == PRIM_BOX) {
        const float hx = fabsf(p.cs) * p.bx + fabsf(p.sn) * p.by, hy = fabsf(p.sn) * p.bx + fabsf(p.cs) * p.by;
        lo[0] = p.ax - hx; hi[0] = p.ax + hx; lo[1] = p.ay - hy; hi[1] = p.ay + hy; lo[2] = p.az - p.bz; hi[2] = p.az + p.bz;
    } else if (p.type == PRIM_CYL) {
        lo[0] = p.ax - p.bx; hi[0] = p.ax + p.bx; lo[1] = p.ay - p.bx; hi[1] = p.ay + p.bx; lo[2] = p.az; hi[2] = p.az + p.bz;
    } else {
        lo[0] = fminf(p.ax, p.bx) - p.rad; hi[0] = fmaxf(p.ax, p.bx) + p.rad;
        lo[1] = fminf(p.ay, p.by) - p.rad; hi[1] = fmaxf(p.ay, p.by) + p.rad;
        lo[2] = fminf(p.az, p.bz) - p.rad; hi[2] = fmaxf(p.az, p.bz) + p.rad;
    }
    const float eps = 1.0e-3f;                      // slack for float rounding of the projection
    float x0 = 3.0e38f, x1 = -3.0e38f, y0 = 3.0e38f, y1 = -3.0e38f;
    bool behind = false;
    for (int k = 0; k < 8; k++) {
        const float wx = ((k & 1) ? hi[0] : lo[0]) - c.ex, wy = ((k & 2) ? hi[1] : lo[1]) - c.ey, wz = ((k & 4) ? hi[2] : lo[2]) - c.ez;
        const float z = wx * c.fx + wy * c.fy + wz * c.fz;
        if (z <= 0.05f) { behind = true; break; }
        const float x = (wx * c.rx + wy * c.ry + wz * c.rz) / z, y = (wx * c.ux + wy * c.uy + wz * c.uz) / z;
        x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
    }
    if (behind) { rect[0] = -3.0e38f; rect[1] = 3.0e38f; rect[2] = -3.0e38f; rect[3] = 3.0e38f; return; }
    rect[0] = x0 - eps; rect[1] = x1 + eps; rect[2] = y0 - eps; rect[3] = y1 + eps;
}

// ---- tile-order path: 8x8 pixel tiles against the primitives' rectangles ----------------------------------------------------
// rows of one band: whole 8-row tile strips that fit the LDS tile buffer — counted in whole tiles, so that a band never has more
// than kTilePixels / 64 of them (one mask word per tile) when the width is no multiple of 8
RASTER_HD int tile_band_rows(int w) { return imax(8, (kTilePixels / (((w + 7) >> 3) << 3)) & ~7); }

// the 8x8 tile whose first pixel is (r0, col0), in tangent space (pixel edges; y grows upwards while rows grow downwards); culling
// only — the primitives' rectangles carry 1e-3 of slack — so reciprocals (inv_w2 = 2 / w, inv_h2 = 2 / h) instead of divisions
struct TileRect { float x0, x1, y0, y1; };

RASTER_HD TileRect tile_rect(const Camera &c, int r0, int col0, float inv_w2, float inv_h2) {
    TileRect t;
    t.x0 = ((float)col0 * inv_w2 - 1.0f) * c.tan_half_fov;
    t.x1 = ((float)(col0 + 8) * inv_w2 - 1.0f) * c.tan_half_fov;
    t.y1 = (1.0f - (float)r0 * inv_h2) * c.tan_half_fov;
    t.y0 = (1.0f - (float)(r0 + 8) * inv_h2) * c.tan_half_fov;
    return t;
}

RASTER_HD bool tile_overlaps(const float rect[4], const TileRect &t) {
    return rect[0] <= t.x1 && rect[1] >= t.x0 && rect[2] <= t.y1 && rect[3] >= t.y0;
}

// ---- object-order path (cameras with a cached background) ------------------------------------------------------------------
// Screen footprint of one moving primitive in pixel units, conservative: rows r0..r1, columns c0..c1 and — for capsules — the
// slab around the projected axis: in row r the columns within hw of xc0 + (r - r0) * kx.  W bounds the columns of any one row.
struct Span {
    int32_t r0, r1, c0, c1, W;
    float xc0, kx, hw;
    int32_t rpc, cch, inv_w;       // chunking: row spans per 64-lane chunk, chunks per row (W > 64), ceil(65536 / W)
};

// what hit_capsule derives from the capsule and the eye alone, evaluated once per (env, camera) with the same expressions
struct CapsK { float bax, bay, baz, oax, oay, oaz, obx, oby, obz, baba, baoa, c, ca, cb; };

RASTER_HDN void capsule_constants(const Prim &p, const Camera &cam, CapsK &k) {
    k.bax = p.bx - p.ax; k.bay = p.by - p.ay; k.baz = p.bz - p.az;
    k.oax = cam.ex - p.ax; k.oay = cam.ey - p.ay; k.oaz = cam.ez - p.az;
    k.obx = cam.ex - p.bx; k.oby = cam.ey - p.by; k.obz = cam.ez - p.bz;
    k.baba = k.bax * k.bax + k.bay * k.bay + k.baz * k.baz;
    k.baoa = k.bax * k.oax + k.bay * k.oay + k.baz * k.oaz;
    const float oaoa = k.oax * k.oax + k.oay * k.oay + k.oaz * k.oaz;
    k.c = k.baba * oaoa - k.baoa * k.baoa - p.rad * p.rad * k.baba;
    k.ca = k.oax * k.oax + k.oay * k.oay + k.oaz * k.oaz - p.rad * p.rad;
    k.cb = k.obx * k.obx + k.oby * k.oby + k.obz * k.obz - p.rad * p.rad;
}

// hit_capsule with the per-capsule part taken from CapsK: same operations in the same order, so the same t
RASTER_HD float hit_capsule_k(const CapsK &k, float dx, float dy, float dz, int &code) {
    const float bard = k.bax * dx + k.bay * dy + k.baz * dz;
    const float rdoa = dx * k.oax + dy * k.oay + dz * k.oaz;
    const float a = k.baba - bard * bard;
    float b = k.baba * rdoa - k.baoa * bard;
    float h = b * b - a * k.c;
    if (h < 0.0f || k.baba == 0.0f) return -1.0f;
    float t = -1.0f, y = 0.0f;
    bool body = false;
    code = 0;
    if (a > 0.0f) {
        t = (-b - sqrtf(h)) / a;
        y = k.baoa + t * bard;
        body = y > 0.0f && y < k.baba;
    }
    if (!body) {            // one of the two end spheres
        const bool at_a = y <= 0.0f;
        b = dx * (at_a ? k.oax : k.obx) + dy * (at_a ? k.oay : k.oby) + dz * (at_a ? k.oaz : k.obz);
        h = b * b - (at_a ? k.ca : k.cb);
        if (h < 0.0f) return -1.0f;
        t = -b - sqrtf(h);
        code = at_a ? 1 : 2;
    }
    return t > 0.0f ? t : -1.0f;
}

// A capsule's surface point q = c + rad * n (c on the axis, |n| = 1) projects within rad * sqrt(1 + |c'|^2) / (Zc - rad) of
// c' = (Xc, Yc) / Zc (Cauchy-Schwarz on Zc * n_xy - n_z * (Xc, Yc)); c' runs along the 2-D segment a'b', |c'|^2 is convex on
// it and Zc is linear, so one radius R2 from the endpoints bounds the whole silhouette: a stadium around a'b'.
RASTER_HDN void prim_span(const Prim &p, const Camera &c, int w, int h, Span &s) {
    float rect[4];
    prim_screen_rect(p, c, rect);
    s.xc0 = 0.0f; s.kx = 0.0f; s.hw = 3.0e38f;
    const float half_w = 0.5f * (float)w, half_h = 0.5f * (float)h, inv_tan = 1.0f / c.tan_half_fov;
    bool slab = false;
    float xa = 0.0f, ya = 0.0f, xb = 0.0f, yb = 0.0f, R2 = 0.0f;
    if (p.type == PRIM_CAPSULE) {
        const float wax = p.ax - c.ex, way = p.ay - c.ey, waz = p.az - c.ez, wbx = p.bx - c.ex, wby = p.by - c.ey, wbz = p.bz - c.ez;
        const float za = wax * c.fx + way * c.fy + waz * c.fz, zb = wbx * c.fx + wby * c.fy + wbz * c.fz;
        const float zmin = fminf(za, zb) - p.rad;
        if (zmin > 0.05f) {
            xa = (wax * c.rx + way * c.ry + waz * c.rz) / za; ya = (wax * c.ux + way * c.uy + waz * c.uz) / za;
            xb = (wbx * c.rx + wby * c.ry + wbz * c.rz) / zb; yb = (wbx * c.ux + wby * c.uy + wbz * c.uz) / zb;
            R2 = p.rad * sqrtf(1.0f + fmaxf(xa * xa + ya * ya, xb * xb + yb * yb)) / zmin * 1.001f + 1.0e-3f;
            rect[0] = fmaxf(rect[0], fminf(xa, xb) - R2); rect[1] = fminf(rect[1], fmaxf(xa, xb) + R2);
            rect[2] = fmaxf(rect[2], fminf(ya, yb) - R2); rect[3] = fminf(rect[3], fmaxf(ya, yb) + R2);
            slab = true;
        }
    }
    // tangent space -> pixel index of the pixel whose centre is there: col = (x / tan + 1) * w / 2 - 1/2, row = (1 - y / tan) * h / 2 - 1/2
    const float cf0 = (rect[0] * inv_tan + 1.0f) * half_w - 0.5f, cf1 = (rect[1] * inv_tan + 1.0f) * half_w - 0.5f;
    const float rf0 = (1.0f - rect[3] * inv_tan) * half_h - 0.5f, rf1 = (1.0f - rect[2] * inv_tan) * half_h - 0.5f;
    s.c0 = (int)ceilf(fminf(fmaxf(cf0, 0.0f), (float)w)); s.c1 = (int)floorf(fminf(fmaxf(cf1, -1.0f), (float)(w - 1)));
    s.r0 = (int)ceilf(fminf(fmaxf(rf0, 0.0f), (float)h)); s.r1 = (int)floorf(fminf(fmaxf(rf1, -1.0f), (float)(h - 1)));
    s.W = imax(s.c1 - s.c0 + 1, 0);
    if (slab && s.W > 0 && s.r1 >= s.r0) {
        const float dx = xb - xa, dy = yb - ya, len = sqrtf(dx * dx + dy * dy);
        if (fabsf(dy) > 1.0e-4f * len && len > 0.0f) {
            // the axis' column in row r: x = xa + (y_r - ya) * dx / dy with y_r = (1 - (r + 1/2) * 2 / h) * tan
            const float slope = dx / dy, px = half_w * inv_tan;
            const float y0 = (1.0f - ((float)s.r0 + 0.5f) / half_h) * c.tan_half_fov;
            s.xc0 = ((xa + (y0 - ya) * slope) * inv_tan + 1.0f) * half_w - 0.5f;
            s.kx = -slope * px * c.tan_half_fov / half_h;
            s.hw = R2 * len / fabsf(dy) * px + 0.01f;
            if (s.hw < 0.5f * (float)w) s.W = imin(s.W, (int)floorf(2.0f * s.hw) + 2); else s.hw = 3.0e38f;
        }
    }
    const int W = imax(s.W, 1);
    s.rpc = imax(1, 64 / W); s.cch = (W + 63) >> 6; s.inv_w = W <= 64 ? (65536 + W - 1) / W : 0;
}

// rows of one band of the object-order path: whole rows that fit the LDS z-buffer
RASTER_HD int span_band_rows(int w) { return imax(1, kBandPixels / w); }

// 64-lane chunks that the band of rows row0..last_row takes of a footprint
RASTER_HD int span_band_chunks(const Span &s, int row0, int last_row) {
    const int pr0 = imax(s.r0, row0), pr1 = imin(s.r1, last_row);
    return (pr1 >= pr0 && s.W > 0) ? ((pr1 - pr0 + s.rpc) / s.rpc) * s.cch : 0;
}

// chunk qq (counted within the footprint, 0 .. span_band_chunks - 1) of the band row0..last_row -> the pixel of `lane`
struct SpanPixel { int row, col, rr, i; bool valid; };     // rr, i: the lane's row span within the chunk and its column within that span

RASTER_HD SpanPixel span_locate(const Span &s, int row0, int last_row, int qq, int lane) {
    SpanPixel it;
    const int W = s.W;
    int group = qq, cc = 0;
    if (s.cch > 1) { group = qq / s.cch; cc = qq - group * s.cch; }
    const int rr = (lane * s.inv_w) >> 16;                                      // lane / W (0 when W > 64)
    const int i = cc * 64 + lane - rr * W;
    it.row = imax(s.r0, row0) + group * s.rpc + rr;
    const float centre = s.xc0 + (float)(it.row - s.r0) * s.kx;
    const int lo = s.hw < 1.0e30f ? imax(s.c0, (int)ceilf(centre - s.hw)) : s.c0;
    const int hi = s.hw < 1.0e30f ? imin(s.c1, (int)floorf(centre + s.hw)) : s.c1;
    it.col = lo + i; it.rr = rr; it.i = i;
    it.valid = rr < s.rpc && i < W && it.row <= imin(s.r1, last_row) && it.col <= hi;
    return it;
}

// ---- cameras ----------------------------------------------------------------------------------------------------------------
// pybullet computeViewMatrixFromYawPitchRoll (upAxisIndex = 2): eye = target + Rz(yaw) Ry(roll) Rx(pitch) (0,-d,0),
// up = R (0,0,1); negative pitch looks down from above.
inline Camera make_camera(const double target[3], double dist, double yaw_deg, double pitch_deg, double roll_deg, double fov_deg) {
    const double d2r = 3.14159265358979323846 / 180.0;
    const double cy = cos(yaw_deg * d2r), sy = sin(yaw_deg * d2r), cp = cos(pitch_deg * d2r), sp = sin(pitch_deg * d2r);
    const double cr = cos(roll_deg * d2r), sr = sin(roll_deg * d2r);
    // R = Rz(yaw) * Ry(roll) * Rx(pitch)
    const double Rm[3][3] = {{cy * cr, cy * sr * sp - sy * cp, cy * sr * cp + sy * sp},
                             {sy * cr, sy * sr * sp + cy * cp, sy * sr * cp - cy * sp},
                             {-sr, cr * sp, cr * cp}};
    double eye[3], up[3], f[3], r[3], u[3];
    for (int k = 0; k < 3; k++) { eye[k] = target[k] + Rm[k][1] * (-dist); up[k] = Rm[k][2]; f[k] = target[k] - eye[k]; }
    double nf = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (int k = 0; k < 3; k++) f[k] /= nf;
    r[0] = f[1] * up[2] - f[2] * up[1]; r[1] = f[2] * up[0] - f[0] * up[2]; r[2] = f[0] * up[1] - f[1] * up[0];
    double nr = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (int k = 0; k < 3; k++) r[k] /= nr;
    u[0] = r[1] * f[2] - r[2] * f[1]; u[1] = r[2] * f[0] - r[0] * f[2]; u[2] = r[0] * f[1] - r[1] * f[0];
    Camera c;
    c.ex = (float)eye[0]; c.ey = (float)eye[1]; c.ez = (float)eye[2];
    c.fx = (float)f[0]; c.fy = (float)f[1]; c.fz = (float)f[2];
    c.rx = (float)r[0]; c.ry = (float)r[1]; c.rz = (float)r[2];
    c.ux = (float)u[0]; c.uy = (float)u[1]; c.uz = (float)u[2];
    c.tan_half_fov = (float)tan(fov_deg * d2r / 2);
    return c;
}

// the two cameras of a Kuka scene
inline void kuka_cameras(Camera cam[2]) {
    const double t1[3] = {0.316, -0.2, -0.1}, t2[3] = {0.316, 0.316, -0.105};
    cam[0] = make_camera(t1, 1.1, 145, -36, 0, 60);        // kuka_button_gym_env.py:94-102
    cam[1] = make_camera(t2, 1.05, 32, -13, 0, 60);        // :403-409 (multi_view)
}

// the two cameras of a MobileRobot scene (one_d: the 1-D arena)
inline void mobile_cameras(bool one_d, Camera cam[2]) {
    const double t[3] = {2, one_d ? 0.0 : 2.0, 0};
    cam[0] = make_camera(t, 4.4, 90, -90, 0, 60);          // mobile_robot_env.py:76-84, 1D :33
    // fpv=True (mobile_robot_env.py:313-332): camera target (robot_x - 0.25, robot_y, 0.15), distance 0.3, yaw = the
    // env's camera yaw, pitch -17, fov 90; stored relative to the robot, the kernel adds each env's (x, y)
    const double tf[3] = {-0.25, 0.0, 0.15};
    cam[1] = make_camera(tf, 0.3, 90, -17, 0, 90);
}

}  // namespace srlraster
