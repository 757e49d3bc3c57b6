// accumulate_device.h -- the device code the launches of p3d_accumulate (accumulate.hip) and of p3d_accumulate_moving
// (accumulate_motion.hip) share: the frame record in the launch arguments, the tile numbering, the taps, and everything of
// the definition after the point whose history is looked for (steps 2 to 4 of DESIGN "Temporal accumulation", from q on).
// Included by those two files only, inside their own unnamed namespace's reach: every name here has internal linkage.
#ifndef P3D_ACCUMULATE_DEVICE_H
#define P3D_ACCUMULATE_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "accumulate.h"
#include "p3d_device_math.h"
#include "p3d_pinhole.h"

namespace p3d {

namespace {

#ifndef P3D_ACCUMULATE_TILE_W
#define P3D_ACCUMULATE_TILE_W 64         // a power of two up to 256; up to 64 a wave is TILE_W x (64 / TILE_W) pixels.  Measured: DESIGN "Temporal accumulation"
#endif
constexpr int kThreads = 256, kTileW = P3D_ACCUMULATE_TILE_W, kTileH = kThreads / kTileW;
constexpr int kXcds = 8;
static_assert(kTileW * kTileH == kThreads && kTileW >= 1, "a tile is one workgroup");

// One frame of the sequence: the pointers are the frame's own first pixel.
struct AccumulateFrame {
    const float *color, *depth, *normal;     // the frame: [res_y][res_x][3], [res_y][res_x], [res_y][res_x][3]
    const int32_t* hit;                      // [res_y][res_x] or NULL
    const float *pcolor, *pdepth, *pnormal, *plength;    // the frame it looks back at (HISTORY only)
    const int32_t* phit;                     // or NULL
    float *out_color, *out_length;           // each may be NULL
    int32_t res_x, res_y, tiles_x, tiles_y;
    float tol, normal_min, max_history;
    float eye[3], uw[3], vh[3], vz[3];       // the frame's camera, as the frame kernels hold it: u * w, v * h, n * -plane_dist
    float peye[3], pu[3], pv[3], pn[3], pw, ph, ppd;     // the previous camera
};

// The tile this workgroup runs: XCD x (workgroups x, x + 8, ...) takes the x-th contiguous share of the tiles.
__device__ __forceinline__ uint32_t logical_block() {
    const uint32_t n = gridDim.x, b = blockIdx.x, q = n / kXcds, r = n % kXcds, xcd = b % kXcds;
    return xcd * q + (xcd < r ? xcd : r) + b / kXcds;
}

struct Blend { V3 sum; float sl, sw; };

// One tap of step 3: (tx, ty) may lie outside the frame.
__device__ __forceinline__ void tap(const AccumulateFrame& F, int64_t tx, int64_t ty, float wgt, float dist, float lim, V3 N, int32_t I,
                                    bool ids, Blend& B) {
    if (tx < 0 || tx >= F.res_x || ty < 0 || ty >= F.res_y) return;
    const size_t at = (size_t)ty * (size_t)F.res_x + (size_t)tx;
    const float zq = F.pdepth[at];
    if (!valid_depth(zq)) return;
    if (!(fabsf(zq - dist) <= lim)) return;
    const float* n = F.pnormal + 3 * at;
    if (!((N.x * n[0] + N.y * n[1]) + N.z * n[2] >= F.normal_min)) return;
    if (ids && F.phit[at] != I) return;
    const float* c = F.pcolor + 3 * at;
    B.sum.x = B.sum.x + wgt * c[0]; B.sum.y = B.sum.y + wgt * c[1]; B.sum.z = B.sum.z + wgt * c[2];
    B.sl = B.sl + wgt * F.plength[at];
    B.sw = B.sw + wgt;
}

// Steps 2 to 4 for the point Q whose history is looked for (the pixel's hit point, or where that surface point was one
// frame ago): operation by operation.  false: no history.  XY: xy[0..1] receive (px, py) once the window test has passed.
template <bool XY>
__device__ __forceinline__ bool reproject_point(const AccumulateFrame& F, size_t pixel, V3 C, V3 Q, V3& out, float& len, float* xy) {
    // 2. the point seen through the previous camera
    const V3 q = mk(Q.x - F.peye[0], Q.y - F.peye[1], Q.z - F.peye[2]);
    const float a = (q.x * F.pu[0] + q.y * F.pu[1]) + q.z * F.pu[2];
    const float b = (q.x * F.pv[0] + q.y * F.pv[1]) + q.z * F.pv[2];
    const float c = -((q.x * F.pn[0] + q.y * F.pn[1]) + q.z * F.pn[2]);
    if (!(c > 0.0f)) return false;
    const float s = fdiv(c, F.ppd);
    const float gx = fdiv(a, F.pw * s), gy = fdiv(b, F.ph * s);
    const float rx = (float)F.res_x, ry = (float)F.res_y;
    const float px = (gx + 0.5f) * rx - 0.5f, py = (gy + 0.5f) * ry - 0.5f;
    if (!(px > -1.0f && px < rx && py > -1.0f && py < ry)) return false;      // NaN too; below, -1 <= floor < 2^31
    if (XY) { xy[0] = px; xy[1] = py; }
    const float x0f = floorf(px), y0f = floorf(py);
    const float tx = px - x0f, ty = py - y0f;
    const int64_t x0 = (int64_t)x0f, y0 = (int64_t)y0f;
    const float dist = fsqrt((q.x * q.x + q.y * q.y) + q.z * q.z), lim = F.tol * dist;
    // 3. the taps
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    const float* n = F.normal + 3 * pixel;
    const V3 N = mk(n[0], n[1], n[2]);
    const bool ids = F.hit != nullptr && F.phit != nullptr;
    const int32_t I = ids ? F.hit[pixel] : 0;
    Blend B = {mk(0.0f, 0.0f, 0.0f), 0.0f, 0.0f};
    tap(F, x0, y0, ux * uy, dist, lim, N, I, ids, B);
    tap(F, x0 + 1, y0, tx * uy, dist, lim, N, I, ids, B);
    tap(F, x0, y0 + 1, ux * ty, dist, lim, N, I, ids, B);
    tap(F, x0 + 1, y0 + 1, tx * ty, dist, lim, N, I, ids, B);
    // 4. the blend
    if (!(B.sw > 0.0f)) return false;
    const V3 H = mk(fdiv(B.sum.x, B.sw), fdiv(B.sum.y, B.sw), fdiv(B.sum.z, B.sw));
    float l = fdiv(B.sl, B.sw) + 1.0f;
    if (l > F.max_history) l = F.max_history;
    const float alpha = fdiv(1.0f, l);
    out = mk(H.x + (C.x - H.x) * alpha, H.y + (C.y - H.y) * alpha, H.z + (C.z - H.z) * alpha);
    len = l;
    return true;
}

// HOST: the record of a sequence before its first frame; -> the workgroups of a launch (at most the pixel count).
inline uint32_t first_frame_record(AccumulateFrame& F, const p3d_accumulate_params& p) {
    memset(&F, 0, sizeof F);
    F.res_x = p.res_x; F.res_y = p.res_y;
    F.tiles_x = (int32_t)(((int64_t)p.res_x + kTileW - 1) / kTileW); F.tiles_y = (int32_t)(((int64_t)p.res_y + kTileH - 1) / kTileH);
    F.tol = p.depth_tolerance; F.normal_min = p.normal_min; F.max_history = p.max_history;
    return (uint32_t)((uint64_t)F.tiles_x * (uint64_t)F.tiles_y);
}

// HOST: turns the record of frame f - 1 (or of first_frame_record) into that of frame f.  false: frame f has nothing to look
// back at.
inline bool next_frame_record(AccumulateFrame& F, const p3d_accumulate_params& p, const AccumulatePlanes& A, const p3d_camera* cams,
                              const p3d_camera* hist_cam, size_t f) {
    const size_t frame = (size_t)p.res_x * (size_t)p.res_y;
    F.color = A.rgb32f + 3 * f * frame; F.depth = A.depth + f * frame; F.normal = A.normal + 3 * f * frame;
    F.hit = A.hit_id ? A.hit_id + f * frame : nullptr;
    float* const prev_color = F.out_color;       // what the launch of frame f - 1 wrote
    float* const prev_length = F.out_length;
    F.out_color = A.out_rgb32f ? A.out_rgb32f + 3 * f * frame : (p.n_frames > 1 ? A.spare_rgb32f + 3 * (f & 1) * frame : nullptr);
    F.out_length = A.out_length ? A.out_length + f * frame : (p.n_frames > 1 ? A.spare_length + (f & 1) * frame : nullptr);
    const p3d_camera* pc = nullptr;
    if (f > 0) {
        F.pcolor = prev_color; F.plength = prev_length;
        F.pdepth = A.depth + (f - 1) * frame; F.pnormal = A.normal + 3 * (f - 1) * frame;
        F.phit = A.hit_id ? A.hit_id + (f - 1) * frame : nullptr;
        pc = &cams[f - 1];
    } else if (A.hist_rgb32f) {
        F.pcolor = A.hist_rgb32f; F.plength = A.hist_length; F.pdepth = A.hist_depth; F.pnormal = A.hist_normal; F.phit = A.hist_hit_id;
        pc = hist_cam;
    }
    const p3d_camera& c = cams[f];
    // the float products Camera::PrimaryRay forms per call, as camera_record() of p3d_render.cpp hands them to the frame kernels
    for (int k = 0; k < 3; k++) { F.eye[k] = c.eye[k]; F.uw[k] = c.u[k] * c.w; F.vh[k] = c.v[k] * c.h; F.vz[k] = c.n[k] * -c.plane_dist; }
    if (!pc) return false;
    for (int k = 0; k < 3; k++) { F.peye[k] = pc->eye[k]; F.pu[k] = pc->u[k]; F.pv[k] = pc->v[k]; F.pn[k] = pc->n[k]; }
    F.pw = pc->w; F.ph = pc->h; F.ppd = pc->plane_dist;
    return true;
}

}  // namespace

}  // namespace p3d
#endif
