// accumulate_device.h -- the device code the launches of p3d_accumulate (accumulate.hip), of p3d_accumulate_moving
// (accumulate_motion.hip) and of p3d_accumulate_variance (accumulate_variance.hip) share: the frame record in the launch
// arguments, the tile numbering, the taps, everything of the definition after the point whose history is looked for (steps
// 2 to 4 of DESIGN "Temporal accumulation", from q on; with the luminance moments as a compile-time variant), and the map of
// a hit point to where it was one frame ago (previous_point).
// Included by those three files only, inside their own unnamed namespace's reach: every name here has internal linkage.
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

// The luminance moments p3d_accumulate_variance carries through the same taps (MOMENTS only): prev the moments plane of the
// frame looked back at ([res_y][res_x][2]), m the pixel's own (l, l * l), sm the taps' sums, out the blended moments --
// written by step 4 only, so they stay what the caller set them to (m) when there is no history.
struct Moments { const float* prev; float m[2], sm[2], out[2]; };

// One tap of step 3: (tx, ty) may lie outside the frame.
template <bool MOMENTS = false>
__device__ __forceinline__ void tap(const AccumulateFrame& F, int64_t tx, int64_t ty, float wgt, float dist, float lim, V3 N, int32_t I,
                                    bool ids, Blend& B, Moments* M = nullptr) {
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
    if constexpr (MOMENTS) {
        const float* m = M->prev + 2 * at;
        M->sm[0] = M->sm[0] + wgt * m[0]; M->sm[1] = M->sm[1] + wgt * m[1];
    }
    B.sw = B.sw + wgt;
}

// Steps 2 to 4 for the point Q whose history is looked for (the pixel's hit point, or where that surface point was one
// frame ago): operation by operation.  false: no history.  XY: xy[0..1] receive (px, py) once the window test has passed.
template <bool XY, bool MOMENTS = false>
__device__ __forceinline__ bool reproject_point(const AccumulateFrame& F, size_t pixel, V3 C, V3 Q, V3& out, float& len, float* xy,
                                                Moments* M = nullptr) {
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
    tap<MOMENTS>(F, x0, y0, ux * uy, dist, lim, N, I, ids, B, M);
    tap<MOMENTS>(F, x0 + 1, y0, tx * uy, dist, lim, N, I, ids, B, M);
    tap<MOMENTS>(F, x0, y0 + 1, ux * ty, dist, lim, N, I, ids, B, M);
    tap<MOMENTS>(F, x0 + 1, y0 + 1, tx * ty, dist, lim, N, I, ids, B, M);
    // 4. the blend
    if (!(B.sw > 0.0f)) return false;
    const V3 H = mk(fdiv(B.sum.x, B.sw), fdiv(B.sum.y, B.sw), fdiv(B.sum.z, B.sw));
    float l = fdiv(B.sl, B.sw) + 1.0f;
    if (l > F.max_history) l = F.max_history;
    const float alpha = fdiv(1.0f, l);
    out = mk(H.x + (C.x - H.x) * alpha, H.y + (C.y - H.y) * alpha, H.z + (C.z - H.z) * alpha);
    if constexpr (MOMENTS) {
        const float h0 = fdiv(M->sm[0], B.sw), h1 = fdiv(M->sm[1], B.sw);
        M->out[0] = h0 + (M->m[0] - h0) * alpha; M->out[1] = h1 + (M->m[1] - h1) * alpha;
    }
    len = l;
    return true;
}

// A frame of p3d_accumulate_moving: accumulate.hip's record and the geometry of the two frames.
struct MovingFrame {
    AccumulateFrame F;
    const uint32_t* type;           // [n_prims]
    const float *cur, *prev;        // [n_prims][12]: what the frame was rendered with, and the frame it looks back at (HISTORY only)
    float* out_xy;                  // [res_y][res_x][2] or NULL
    uint32_t n_prims;
};

// 16 bytes of a record as words; the records and the prev_xy plane are only as aligned as their floats
typedef uint32_t Words4A __attribute__((ext_vector_type(4)));
typedef Words4A Words4 __attribute__((aligned(4)));
typedef float Float2A __attribute__((ext_vector_type(2)));
typedef Float2A Float2 __attribute__((aligned(4)));

struct Record { Words4A w[3]; };

__device__ __forceinline__ Record load_record(const float* records, uint32_t i) {
    const Words4* p = (const Words4*)(records + 12 * (size_t)i);
    return {{p[0], p[1], p[2]}};
}
__device__ __forceinline__ float fl(uint32_t w) { return __uint_as_float(w); }
__device__ __forceinline__ float dot3(V3 p, V3 q) { return (p.x * q.x + p.y * q.y) + p.z * q.z; }

// P_prev of include/p3d_hip.h for the hit point P on primitive I.  false: the primitive has changed and its kind gives no point
// one frame ago (a plane): no history.
__device__ __forceinline__ bool previous_point(const MovingFrame& M, int32_t I, V3 P, V3& Q) {
    Q = P;
    if (I < 0 || (uint32_t)I >= M.n_prims) return true;
    const uint32_t k = M.type[I];
    const Record a = load_record(M.cur, (uint32_t)I), b = load_record(M.prev, (uint32_t)I);
    const bool same4 = a.w[0].x == b.w[0].x && a.w[0].y == b.w[0].y && a.w[0].z == b.w[0].z && a.w[0].w == b.w[0].w;
    const bool same6 = same4 && a.w[1].x == b.w[1].x && a.w[1].y == b.w[1].y;
    const bool same9 = same6 && a.w[1].z == b.w[1].z && a.w[1].w == b.w[1].w && a.w[2].x == b.w[2].x;
    if (k == P3D_SPHERE) {
        if (same4) return true;
        const float s = fdiv(fl(b.w[0].w), fl(a.w[0].w));
        Q = mk(fl(b.w[0].x) + (P.x - fl(a.w[0].x)) * s, fl(b.w[0].y) + (P.y - fl(a.w[0].y)) * s, fl(b.w[0].z) + (P.z - fl(a.w[0].z)) * s);
        return true;
    }
    if (k == P3D_TRIANGLE) {
        if (same9) return true;
        const V3 p0 = mk(fl(a.w[0].x), fl(a.w[0].y), fl(a.w[0].z)), p1 = mk(fl(a.w[0].w), fl(a.w[1].x), fl(a.w[1].y));
        const V3 p2 = mk(fl(a.w[1].z), fl(a.w[1].w), fl(a.w[2].x));
        const V3 e1 = mk(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z), e2 = mk(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z);
        const V3 w = mk(P.x - p0.x, P.y - p0.y, P.z - p0.z);
        const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), w1 = dot3(w, e1), w2 = dot3(w, e2);
        const float den = d11 * d22 - d12 * d12;
        const float beta = fdiv(d22 * w1 - d12 * w2, den), gamma = fdiv(d11 * w2 - d12 * w1, den);
        const V3 q0 = mk(fl(b.w[0].x), fl(b.w[0].y), fl(b.w[0].z)), q1 = mk(fl(b.w[0].w), fl(b.w[1].x), fl(b.w[1].y));
        const V3 q2 = mk(fl(b.w[1].z), fl(b.w[1].w), fl(b.w[2].x));
        const V3 f1 = mk(q1.x - q0.x, q1.y - q0.y, q1.z - q0.z), f2 = mk(q2.x - q0.x, q2.y - q0.y, q2.z - q0.z);
        Q = mk((q0.x + f1.x * beta) + f2.x * gamma, (q0.y + f1.y * beta) + f2.y * gamma, (q0.z + f1.z * beta) + f2.z * gamma);
        return true;
    }
    if (k == P3D_BOX) {
        if (same6) return true;
        const float mn[3] = {fl(a.w[0].x), fl(a.w[0].y), fl(a.w[0].z)}, mx[3] = {fl(a.w[0].w), fl(a.w[1].x), fl(a.w[1].y)};
        const float pmn[3] = {fl(b.w[0].x), fl(b.w[0].y), fl(b.w[0].z)}, pmx[3] = {fl(b.w[0].w), fl(b.w[1].x), fl(b.w[1].y)};
        const float p[3] = {P.x, P.y, P.z};
        float r[3];
        for (int c = 0; c < 3; c++) {
            const float e = mx[c] - mn[c];
            const float t = e != 0.0f ? fdiv(p[c] - mn[c], e) : 0.0f;
            r[c] = pmn[c] + (pmx[c] - pmn[c]) * t;
        }
        Q = mk(r[0], r[1], r[2]);
        return true;
    }
    return same4;                    // a plane, or a kind this library does not know: unchanged, or no point to look at
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
