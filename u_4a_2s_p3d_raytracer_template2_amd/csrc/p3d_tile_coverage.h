// p3d_tile_coverage.h -- which tiles of the level-1 launch a primitive's projection can touch, seen through a pinhole camera:
// a CONSERVATIVE set (never a tile short), for the per-frame mask of tiles no primitive projects onto
// (LaunchParams::sky_mask: wf_primary_kernel_tiles fills those with the background and traces nothing).
// Compiled for the device (the pre-pass, tile_coverage_kernel of p3d_kernels.hip) and for the host (host/tile_coverage_host.cpp,
// tests/test_tile_coverage_host.py): plain arithmetic in double, no library calls, the same statements on both.
//
// Why the set is conservative.  Pixel (x, y) looks along uw * fx + vh * fy + vz with fx = (x + 0.5) / res_x - 0.5 (fy alike;
// p3d_pinhole.h), so a point eye + s * (that direction), s > 0, solves to exactly (fx, fy) under project() below, and in
// the continuous pixel coordinates used here -- px = (fx + 0.5) * res_x - 0.5 -- the ray of pixel x sits AT px = x.
// A triangle is the convex hull of its vertices and a sphere or a box lies inside the hull of the eight corners of its
// bounds; with every such point strictly in front of the eye the projection maps the hull into the convex hull of the
// projected points, so a hit point of pixel (x, y) projects inside that polygon.  What is not exact -- the ray's direction
// is rounded to float, the intersectors accept hits within rounding of an edge, e1 / e2 are rounded differences -- moves
// a projected hit by a small fraction of a pixel; every extent is widened by kCoverMarginPx pixels on each side.
// A point that is not in front of the eye by kCoverMinDepth, or does not project to a finite place, makes the answer
// "every tile" (CoverRow::all): the caller marks the whole frame active.
//
// Per tile ROW, not one rectangle: the rows of tiles a polygon spans each get the polygon's own horizontal extent inside
// the row's (widened) band of image rows -- the extreme x of the points inside the band and of every point-to-point segment
// where it crosses the band's two borders.  All segments are taken, not only the hull's edges: the others lie inside the
// hull and change nothing, and no hull has to be built for 3 or 8 points.
//
// Sharded frames (world > 1): a tile's compact rows are mapped to image rows exactly, as image_row() of p3d_kernels.hip
// does; a tile never straddles two row blocks because row_block is a multiple of 16 and a tile is 4 or 16 rows tall.
#ifndef P3D_TILE_COVERAGE_H
#define P3D_TILE_COVERAGE_H

#include <stdint.h>

#include "p3d_device_types.h"

namespace p3d {

constexpr double kCoverMarginPx = 2.0;      // widening of every extent, pixels on each side (the issue asks for at least one)
constexpr double kCoverMinDepth = 1e-3;     // a point must be this far in front of the eye, in units of the image plane's distance
constexpr int kCoverMaxPoints = 8;

// The camera as the frame kernels get it (camera_record() of p3d_render.cpp: uw = u * w, vh = v * h, vz = n * -plane_dist,
// float products) and the inverse of [uw vh vz] by cofactors, in double.
struct CoverCamera {
    double eye[3];
    double c0[3], c1[3], c2[3];     // vh x vz, vz x uw, uw x vh
    double det;                     // uw . c0
    bool ok;                        // the three vectors span space
};
P3D_HD inline CoverCamera cover_camera(const float eye[3], const float uw[3], const float vh[3], const float vz[3]) {
    CoverCamera c;
    const double a[3] = {uw[0], uw[1], uw[2]}, b[3] = {vh[0], vh[1], vh[2]}, d[3] = {vz[0], vz[1], vz[2]};
    for (int k = 0; k < 3; k++) c.eye[k] = eye[k];
    c.c0[0] = b[1] * d[2] - b[2] * d[1]; c.c0[1] = b[2] * d[0] - b[0] * d[2]; c.c0[2] = b[0] * d[1] - b[1] * d[0];
    c.c1[0] = d[1] * a[2] - d[2] * a[1]; c.c1[1] = d[2] * a[0] - d[0] * a[2]; c.c1[2] = d[0] * a[1] - d[1] * a[0];
    c.c2[0] = a[1] * b[2] - a[2] * b[1]; c.c2[1] = a[2] * b[0] - a[0] * b[2]; c.c2[2] = a[0] * b[1] - a[1] * b[0];
    c.det = a[0] * c.c0[0] + a[1] * c.c0[1] + a[2] * c.c0[2];
    const double la = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], lb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2],
                 ld = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    // det^2 against (|uw| |vh| |vz|)^2: a flat or non-finite frame (NaN fails the comparison) serves no mask
    c.ok = c.det * c.det > 1e-12 * (la * lb * ld) && la * lb * ld < 1e300;
    return c;
}

// What the level-1 launch covers this rank's rows with: tiles of 16 x tile_h pixels, tiles_y rows of them over the compact
// buffer (all bands of the frame), and the sharding of image_row().
struct CoverTiles {
    int32_t res_x, res_y;
    int32_t tile_h;                 // 4 * wg_waves
    int32_t tiles_x, tiles_y;
    int32_t row_block, rank, world;
};
// first image row of tile row ty (its tile_h rows are consecutive image rows: see the head of the file)
P3D_HD inline int32_t cover_tile_image_row(const CoverTiles& g, int32_t ty) {
    const int32_t row = ty * g.tile_h, blk = row / g.row_block;
    return (blk * g.world + g.rank) * g.row_block + (row - blk * g.row_block);
}

// continuous pixel coordinates of world point p; false: not in front of the eye by the margin, or not finite
P3D_HD inline bool cover_project(const CoverCamera& c, const CoverTiles& g, const double p[3], double& px, double& py) {
    const double q[3] = {p[0] - c.eye[0], p[1] - c.eye[1], p[2] - c.eye[2]};
    const double t = (q[0] * c.c2[0] + q[1] * c.c2[1] + q[2] * c.c2[2]) / c.det;
    if (!(t >= kCoverMinDepth)) return false;                                   // (NaN fails)
    const double fx = (q[0] * c.c0[0] + q[1] * c.c0[1] + q[2] * c.c0[2]) / c.det / t;
    const double fy = (q[0] * c.c1[0] + q[1] * c.c1[1] + q[2] * c.c1[2]) / c.det / t;
    px = (fx + 0.5) * (double)g.res_x - 0.5;
    py = (fy + 0.5) * (double)g.res_y - 0.5;
    return px > -1e15 && px < 1e15 && py > -1e15 && py < 1e15;                  // finite, and safe to turn into an int64
}

// floor / ceil of a double known to lie inside (-1e15, 1e15), without the math library
P3D_HD inline int64_t cover_floor(double v) { const int64_t i = (int64_t)v; return (double)i > v ? i - 1 : i; }
P3D_HD inline int64_t cover_ceil(double v) { const int64_t i = (int64_t)v; return (double)i < v ? i + 1 : i; }

// The projected points of one primitive of N points (3: a triangle, 8: the corners of a box; a template parameter so that the
// loops unroll and the points stay in registers on the device).  ok = false: the primitive asks for every tile.
template <int N> struct CoverPolygon { double px[N], py[N]; bool ok; };
template <int N>
P3D_HD inline CoverPolygon<N> cover_polygon(const CoverCamera& c, const CoverTiles& g, const double (*pts)[3]) {
    static_assert(N >= 1 && N <= kCoverMaxPoints, "3 or 8 points");
    CoverPolygon<N> poly;
    poly.ok = c.ok;
    for (int i = 0; i < N; i++) {
        poly.px[i] = 0.0; poly.py[i] = 0.0;
        if (poly.ok) poly.ok = cover_project(c, g, pts[i], poly.px[i], poly.py[i]);
    }
    return poly;
}

// The tile columns [tx0, tx1] of tile row ty the polygon can touch; false: none.  (poly.ok is the caller's to test first.)
template <int N>
P3D_HD inline bool cover_row_extent(const CoverPolygon<N>& poly, const CoverTiles& g, int32_t ty, int32_t& tx0, int32_t& tx1) {
    const int32_t y0 = cover_tile_image_row(g, ty);
    if (y0 >= g.res_y) return false;                                            // rows the compact buffer pads the image with
    const double m = kCoverMarginPx;
    const double lo_y = (double)y0 - m, hi_y = (double)(y0 + g.tile_h - 1) + m;  // the band: the tile's pixel centres, widened
    double lo = 1e300, hi = -1e300;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < N; i++) {
        const double xi = poly.px[i], yi = poly.py[i];
        if (yi >= lo_y && yi <= hi_y) { lo = xi < lo ? xi : lo; hi = xi > hi ? xi : hi; }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = i + 1; j < N; j++) {
            const double xj = poly.px[j], yj = poly.py[j];
            for (int b = 0; b < 2; b++) {
                const double yb = b ? hi_y : lo_y;
                if ((yi < yb && yj > yb) || (yi > yb && yj < yb)) {              // the segment crosses this border of the band
                    const double x = xi + (yb - yi) / (yj - yi) * (xj - xi);
                    lo = x < lo ? x : lo; hi = x > hi ? x : hi;
                }
            }
        }
    }
    if (!(lo <= hi)) return false;                                              // nothing of the polygon inside the band
    lo -= m; hi += m;
    if (hi < 0.0 || lo > (double)(g.res_x - 1)) return false;
    lo = lo < 0.0 ? 0.0 : lo; hi = hi > (double)(g.res_x - 1) ? (double)(g.res_x - 1) : hi;
    const int64_t x0 = cover_ceil(lo), x1 = cover_floor(hi);                    // the pixel columns inside [lo, hi]
    if (x0 > x1) return false;
    tx0 = (int32_t)(x0 >> 4); tx1 = (int32_t)(x1 >> 4);
    return true;
}

// The points of a primitive in scene order of their fields: a triangle's p0, p0 + e1, p0 + e2 (TriRec), and the eight
// corners of a box lo .. hi (a BoxRec's, or a sphere's centre -+ radius).
P3D_HD inline void cover_triangle_points(const float p0[3], const float e1[3], const float e2[3], double (*pts)[3]) {
    for (int a = 0; a < 3; a++) { pts[0][a] = p0[a]; pts[1][a] = (double)p0[a] + (double)e1[a]; pts[2][a] = (double)p0[a] + (double)e2[a]; }
}
P3D_HD inline void cover_box_points(const double lo[3], const double hi[3], double (*pts)[3]) {
    for (int k = 0; k < 8; k++)
        for (int a = 0; a < 3; a++) pts[k][a] = ((k >> a) & 1) ? hi[a] : lo[a];
}

// One primitive's part of tile row ty: the columns it can touch, or "every tile of the frame" (all).
struct CoverRow { bool all, any; int32_t tx0, tx1; };
template <int N>
P3D_HD inline CoverRow cover_row(const CoverCamera& c, const CoverTiles& g, const double (*pts)[3], int32_t ty) {
    CoverRow r = {false, false, 0, 0};
    const CoverPolygon<N> poly = cover_polygon<N>(c, g, pts);
    if (!poly.ok) { r.all = true; return r; }
    r.any = cover_row_extent<N>(poly, g, ty, r.tx0, r.tx1);
    return r;
}

// ---- the mask in memory (LaunchParams::sky_mask) and the pre-pass that writes it (p3d_kernels.hip: tile_coverage_kernel)
// Tile (tx, ty) -- ty counted over the rank's whole compact buffer, the bands of a frame included -- is bit tx & 31 of word
// ty * row_words + (tx >> 5); a set bit = some primitive may touch the tile.  status[ty] = active tiles of the row, with
// bit 31 set when a primitive asked for every tile (the whole frame is then marked active: every row says so).
constexpr uint32_t kCoverMaxRowWords = 64;          // tiles_x <= 2048
constexpr uint32_t kCoverAllFlag = 0x80000000u;
P3D_HD inline uint32_t cover_row_words(int32_t tiles_x) { return ((uint32_t)tiles_x + 31u) >> 5; }
// bits [tx0, tx1] that fall into word w
P3D_HD inline uint32_t cover_word_bits(int32_t tx0, int32_t tx1, uint32_t w) {
    const int64_t lo = (int64_t)tx0 - 32 * (int64_t)w, hi = (int64_t)tx1 - 32 * (int64_t)w;
    if (hi < 0 || lo > 31) return 0u;
    const uint32_t from = lo < 0 ? 0u : (uint32_t)lo, to = hi > 31 ? 31u : (uint32_t)hi;
    return (0xFFFFFFFFu >> (31u - to)) & (0xFFFFFFFFu << from);
}
struct TileCoverageJob {
    float eye[3], uw[3], vh[3], vz[3];
    CoverTiles tiles;
    const void* blob;                               // the scene blob on the device (LaunchParams::blob), sections in quads
    uint32_t off_spheres, off_tris, off_boxes, tri_quads;
    uint32_t n_spheres, n_tris, n_boxes;
    uint32_t row_words;
    uint32_t* mask;                                 // [tiles_y][row_words]
    uint32_t* status;                               // [tiles_y]
};

}  // namespace p3d
#endif
