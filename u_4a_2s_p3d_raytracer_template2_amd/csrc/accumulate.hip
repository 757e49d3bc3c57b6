// accumulate.hip -- the device side of p3d_accumulate, p3d_accumulate_moving and p3d_accumulate_variance: temporal
// reprojection of history over the AOV planes of a sequence.  A pixel's primary hit (the pinhole ray through its centre,
// times its depth) is projected into the previous frame's camera; the four pixels around that point which show the same
// surface (depth, normal, hit id) give the accumulated colour and its history length by bilinear weights, and the current
// colour is blended in with weight 1 / length.  IEEE basic operations only, in one fixed order (DESIGN "Temporal
// accumulation", include/p3d_hip.h) -- so the device, the host restatement (host/accumulate_host.cpp) and the NumPy ones
// (tests/accumulate_reference.py, accumulate_moving_reference.py, accumulate_variance_reference.py) agree in every bit.
// Built with the ray kernels' flags (-ffp-contract=off, correctly rounded division and square root).
//   It is one algorithm (temporal_pixel) with two additions, each a compile-time switch:
//   - MOVING (p3d_accumulate_moving): the reprojection through primitives that p3d_scene_update moved.  The pixel's hit
//     point P on primitive I is mapped to the same surface point of primitive I one frame ago (sphere: the same direction
//     from the centre; triangle: the same barycentric coordinates; box: the same fraction of every axis), and that point,
//     not P, is projected into the previous camera.  The map is fused into the gather pass: the lane that will read the four
//     taps reads its primitive's kind and its two 48-byte records first -- one more dependent load stage, no per-pixel
//     motion plane in memory.  The records are read with three 16-byte loads each.  Pixels of one primitive read the same
//     100 bytes, so inside a silhouette a wave's lookup is a handful of cache lines; lanes whose depth is not valid (misses)
//     and lanes whose id is outside the primitives read nothing.  profiles/accumulate_moving_cost.txt has the cost against
//     p3d_accumulate.
//   - MOMENTS (p3d_accumulate_variance): the first two moments of every pixel's luminance carried through the same gather,
//     8 more bytes per tap and no second reprojection, and turned into the variance that steers p3d_denoise_variance (SVGF,
//     Schied et al. 2017).  Colour, length and prev_xy are the other entries' in every bit.
//   One temporal launch per frame of the sequence, in stream order: frame f reads what the launch of frame f - 1 wrote.  One
//   thread per pixel; a workgroup of 256 threads owns a tile of kTileW x kTileH pixels.  The taps are read where they lie,
//   through L2 (profiles/denoise_cost.txt: staging does not pay once taps scatter); under a smooth camera motion the taps of
//   neighbouring pixels are neighbours.  The tile is 64 x 4: a wave is ONE row of 64 pixels, so its own 12-byte pixels and,
//   mostly, its taps are contiguous runs of 768 bytes.  Compact 2-D footprints were tried and lost: 32 x 8 (a wave 32 x 2)
//   is 1 % slower, 16 x 16 (16 x 4) 8 %, 8 x 32 (8 x 8) 37 % -- their rows are fragments of cache lines, and the four taps of
//   a pixel overlap those of its row neighbours whatever the tile (profiles/accumulate_cost.txt).  Workgroups are numbered
//   so that each XCD (workgroup index mod 8) runs a contiguous range of tiles.
//   Both cameras travel in the launch arguments: no camera buffer exists on the device.  Each entry keeps a kernel of its
//   own name whose argument record holds what that entry reads and no more.
//   With a variance wanted, a second launch per frame follows the temporal one, for pixels whose history is shorter than
//   min_temporal: the variance of the luminance over the (2 radius + 1)^2 neighbours of the frame's INPUT colour, weighted
//   by p3d_denoise's depth and normal stops.  (The temporal launch writes the moments and the temporal variance
//   max(0, m2 - m1^2) beside colour and length; which pixels take the estimate is known only once their lengths are.)  A
//   workgroup (32 x 8 pixels, denoise.hip's tile) none of whose pixels needs it returns after reading its lengths; the
//   others stage the tile and a halo of `radius` pixels of colour, depth and normal in LDS, in the planes' own layout and in
//   coalesced rows, as denoise.hip does (at radius 3: 38 x 14 pixels of 28 bytes, 14.9 KB), pack the pixels that take the
//   estimate into their first lanes and run the taps from LDS.  It is not launched at all when min_temporal == 1 (no length
//   is below 1) or when nobody wants the variance.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <type_traits>

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

// A frame of p3d_accumulate_moving: the record above and the geometry of the two frames.
struct MovingFrame {
    AccumulateFrame F;
    const uint32_t* type;           // [n_prims]
    const float *cur, *prev;        // [n_prims][12]: what the frame was rendered with, and the frame it looks back at (HISTORY only)
    float* out_xy;                  // [res_y][res_x][2] or NULL
    uint32_t n_prims;
};

// A frame of p3d_accumulate_variance: the record above (its geometry unused without a motion) and the moments.
struct VarianceFrame {
    MovingFrame M;
    const float* pmoments;          // [res_y][res_x][2]: of the frame looked back at (HISTORY only)
    float* out_moments;             // [res_y][res_x][2] or NULL
    float* out_variance;            // [res_y][res_x] or NULL
};

__device__ __forceinline__ const AccumulateFrame& frame_of(const AccumulateFrame& F) { return F; }
__device__ __forceinline__ const AccumulateFrame& frame_of(const MovingFrame& M) { return M.F; }
__device__ __forceinline__ const AccumulateFrame& frame_of(const VarianceFrame& V) { return V.M.F; }
__device__ __forceinline__ const MovingFrame& motion_of(const MovingFrame& M) { return M; }
__device__ __forceinline__ const MovingFrame& motion_of(const VarianceFrame& V) { return V.M; }

// The tile this workgroup runs: XCD x (workgroups x, x + 8, ...) takes the x-th contiguous share of the tiles.
__device__ __forceinline__ uint32_t logical_block() {
    const uint32_t n = gridDim.x, b = blockIdx.x, q = n / kXcds, r = n % kXcds, xcd = b % kXcds;
    return xcd * q + (xcd < r ? xcd : r) + b / kXcds;
}

struct Blend { V3 sum; float sl, sw; };

// The luminance moments carried through the same taps (MOMENTS only): prev the moments plane of the frame looked back at
// ([res_y][res_x][2]), m the pixel's own (l, l * l), sm the taps' sums, out the blended moments -- written by step 4 only,
// so they stay what the caller set them to (m) when there is no history.
struct Moments { const float* prev; float m[2], sm[2], out[2]; };

// One tap of step 3: (tx, ty) may lie outside the frame.
template <bool MOMENTS>
__device__ __forceinline__ void tap(const AccumulateFrame& F, int64_t tx, int64_t ty, float wgt, float dist, float lim, V3 N, int32_t I,
                                    bool ids, Blend& B, Moments* M) {
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
template <bool XY, bool MOMENTS>
__device__ __forceinline__ bool reproject_point(const AccumulateFrame& F, size_t pixel, V3 C, V3 Q, V3& out, float& len, float* xy, Moments* M) {
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

__device__ __forceinline__ float lum(V3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
__device__ __forceinline__ float max0(float v) { return v > 0.0f ? v : 0.0f; }

// One pixel of the temporal launch: DESIGN "Temporal accumulation", operation by operation.  HISTORY: the frame has a frame
// to look back at.  MOVING: Rec has a geometry (motion_of) and the history is looked for where the hit point was one frame
// ago.  The moments travel when Rec is the record that has them.
template <bool HISTORY, bool MOVING, class Rec>
__device__ __forceinline__ void temporal_pixel(const Rec& R) {
    constexpr bool MOMENTS = std::is_same<Rec, VarianceFrame>::value;
    static_assert(!MOVING || !std::is_same<Rec, AccumulateFrame>::value, "p3d_accumulate's record has no geometry");
    const AccumulateFrame& F = frame_of(R);
    const uint32_t blk = logical_block(), tile_x = blk % (uint32_t)F.tiles_x, tile_y = blk / (uint32_t)F.tiles_x;
    const int64_t x = (int64_t)tile_x * kTileW + (int)threadIdx.x % kTileW, y = (int64_t)tile_y * kTileH + (int)threadIdx.x / kTileW;
    if (x >= F.res_x || y >= F.res_y) return;
    const size_t pixel = (size_t)y * (size_t)F.res_x + (size_t)x;
    const float* cp = F.color + 3 * pixel;
    const V3 C = mk(cp[0], cp[1], cp[2]);            // read before anything is written: out_color may be color
    Moments mo = {};
    if constexpr (MOMENTS) {
        const float l = lum(C), l2 = l * l;
        mo = {R.pmoments, {l, l2}, {0.0f, 0.0f}, {l, l2}};
    }
    V3 out = C;
    float len = 1.0f;
    float xy[2] = {__uint_as_float(0x7FC00000u), __uint_as_float(0x7FC00000u)};
    float Z = 0.0f;
    if (HISTORY || MOMENTS) Z = F.depth[pixel];      // the variance of a miss is 0, history or none
    if (HISTORY) {
        if (valid_depth(Z)) {                        // 0.; a miss reads no id and no record
            // 1. the ray of the frame kernels and the point it reaches (p3d_pinhole.h)
            const V3 d = pinhole_dir(F.uw, F.vh, F.vz, (int32_t)x, (int32_t)y, F.res_x, F.res_y);
            const V3 P = pinhole_point(F.eye, d, Z);
            V3 Q = P, o;
            float ln;
            bool found = true;
            if constexpr (MOVING) found = previous_point(motion_of(R), F.hit[pixel], P, Q);
            // 2. to 4. from where that surface point was one frame ago, the moments with the colour
            if (found && reproject_point<MOVING, MOMENTS>(F, pixel, C, Q, o, ln, xy, &mo)) { out = o; len = ln; }
        }
    }
    if (F.out_color) { float* o = F.out_color + 3 * pixel; o[0] = out.x; o[1] = out.y; o[2] = out.z; }
    if (F.out_length) F.out_length[pixel] = len;
    if constexpr (MOVING) {
        if (motion_of(R).out_xy) { Float2A v; v.x = xy[0]; v.y = xy[1]; *(Float2*)(motion_of(R).out_xy + 2 * pixel) = v; }
    }
    if constexpr (MOMENTS) {
        if (R.out_moments) { Float2A v; v.x = mo.out[0]; v.y = mo.out[1]; *(Float2*)(R.out_moments + 2 * pixel) = v; }
        if (R.out_variance) R.out_variance[pixel] = valid_depth(Z) ? max0(mo.out[1] - mo.out[0] * mo.out[0]) : 0.0f;
    }
}

// The three entries' kernels: the record of each holds what its entry reads and no more.
template <bool HISTORY>
__global__ void __launch_bounds__(kThreads) accumulate_kernel(AccumulateFrame F) { temporal_pixel<HISTORY, false>(F); }
template <bool HISTORY>
__global__ void __launch_bounds__(kThreads) accumulate_moving_kernel(MovingFrame M) { temporal_pixel<HISTORY, true>(M); }
template <bool HISTORY, bool MOVING>
__global__ void __launch_bounds__(kThreads) accumulate_variance_kernel(VarianceFrame V) { temporal_pixel<HISTORY, MOVING>(V); }

template <bool HISTORY>
void launch_temporal(const VarianceFrame& V, bool moving, bool moments, uint32_t blocks, hipStream_t stream) {
    const dim3 grid(blocks), threads(kThreads);
    if (moments && moving) hipLaunchKernelGGL((accumulate_variance_kernel<HISTORY, true>), grid, threads, 0, stream, V);
    else if (moments) hipLaunchKernelGGL((accumulate_variance_kernel<HISTORY, false>), grid, threads, 0, stream, V);
    else if (moving) hipLaunchKernelGGL(accumulate_moving_kernel<HISTORY>, grid, threads, 0, stream, V.M);
    else hipLaunchKernelGGL(accumulate_kernel<HISTORY>, grid, threads, 0, stream, V.M.F);
}

// ---------------------------------------------------------------- the spatial estimate
constexpr int kSpatialW = 32, kSpatialH = 8, kSpatialThreads = kSpatialW * kSpatialH;

struct SpatialFrame {
    const float *color, *depth, *normal;     // the frame's INPUT planes
    const float* length;                     // the frame's OUTPUT length
    float* variance;                         // the temporal launch has written it; pixels that take the estimate are overwritten
    int32_t res_x, res_y, tiles_x, tiles_y;
    int32_t npow;
    float min_temporal, sigma_depth;
};

template <int R>
__global__ void __launch_bounds__(kSpatialThreads) spatial_variance_kernel(SpatialFrame S) {
    constexpr int W = kSpatialW + 2 * R, H = kSpatialH + 2 * R;
    __shared__ float sz[W * H], sn[3 * W * H], sc[3 * W * H];
    __shared__ uint16_t list[kSpatialThreads];
    __shared__ int count;
    const uint32_t blk = logical_block(), tile_x = blk % (uint32_t)S.tiles_x, tile_y = blk / (uint32_t)S.tiles_x;
    const int tid = (int)threadIdx.x, lx = tid % kSpatialW, ly = tid / kSpatialW;
    const int64_t x0 = (int64_t)tile_x * kSpatialW, y0 = (int64_t)tile_y * kSpatialH, x = x0 + lx, y = y0 + ly;
    const bool inside = x < S.res_x && y < S.res_y;
    const size_t pixel = inside ? (size_t)y * (size_t)S.res_x + (size_t)x : 0;
    const bool wanted = inside && S.length[pixel] < S.min_temporal;
    if (tid == 0) count = 0;
    if (!__syncthreads_or(wanted)) return;           // every history of the tile is long enough
    const int64_t hx0 = x0 - R, hy0 = y0 - R;        // the halo's corner: may lie outside the frame
    for (int i = tid; i < W * H; i += kSpatialThreads) {
        const int64_t gy = hy0 + i / W, gx = hx0 + i % W;
        const bool in = gy >= 0 && gy < S.res_y && gx >= 0 && gx < S.res_x;
        sz[i] = in ? S.depth[(size_t)gy * (size_t)S.res_x + (size_t)gx] : 0.0f;      // outside the frame: not valid
    }
    for (int i = tid; i < 3 * W * H; i += kSpatialThreads) {       // rows of 3 W floats, as they lie in the planes
        const int64_t gy = hy0 + i / (3 * W), g3 = 3 * hx0 + i % (3 * W);
        const bool in = gy >= 0 && gy < S.res_y && g3 >= 0 && g3 < 3 * (int64_t)S.res_x;
        const size_t at = 3 * ((size_t)gy * (size_t)S.res_x) + (size_t)g3;
        sn[i] = in ? S.normal[at] : 0.0f;
        sc[i] = in ? S.color[at] : 0.0f;
    }
    __syncthreads();
    // The pixels that take the estimate are packed into the first lanes: after a few frames they are the disocclusions, a
    // few per tile, and spread over the waves every one of them would hold a whole wave in the loop below.  (The order in
    // the list is that of the LDS atomic and does not matter: a pixel's estimate depends on the pixel alone.)
    const int own = (ly + R) * W + lx + R;
    if (wanted && valid_depth(sz[own])) list[atomicAdd(&count, 1)] = (uint16_t)tid;      // not valid: the temporal launch wrote 0
    __syncthreads();
    if (tid >= count) return;
    const int px = list[tid] % kSpatialW, py = list[tid] / kSpatialW;
    const int at = (py + R) * W + px + R;
    const float zp = sz[at];
    const V3 np = mk(sn[3 * at], sn[3 * at + 1], sn[3 * at + 2]);
    const float inv_z = 1.0f / (S.sigma_depth * zp);
    float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -R; dy <= R; dy++) {
#pragma unroll
        for (int dx = -R; dx <= R; dx++) {
            const int q = at + dy * W + dx;
            const float zq = sz[q];
            if (!valid_depth(zq)) continue;
            const float tz = max0(1.0f - fabsf(zq - zp) * inv_z), wz = tz * tz;
            const float dn = (np.x * sn[3 * q] + np.y * sn[3 * q + 1]) + np.z * sn[3 * q + 2];
            float wn = max0(dn);
            for (int j = 0; j < S.npow; j++) wn = wn * wn;
            const float w = wz * wn;
            const float lq = lum(mk(sc[3 * q], sc[3 * q + 1], sc[3 * q + 2]));
            s1 = s1 + w * lq;
            s2 = s2 + w * (lq * lq);
            sw = sw + w;
        }
    }
    if (!(sw > 0.0f)) return;                        // the temporal variance stays
    const float a = s1 / sw, b = s2 / sw;
    S.variance[(size_t)(y0 + py) * (size_t)S.res_x + (size_t)(x0 + px)] = max0(b - a * a);
}

void launch_spatial(const SpatialFrame& S, int radius, hipStream_t stream) {
    const dim3 blocks((uint32_t)((uint64_t)S.tiles_x * (uint64_t)S.tiles_y)), threads(kSpatialThreads);     // at most the pixel count
    switch (radius) {
    case 1: hipLaunchKernelGGL(spatial_variance_kernel<1>, blocks, threads, 0, stream, S); break;
    case 2: hipLaunchKernelGGL(spatial_variance_kernel<2>, blocks, threads, 0, stream, S); break;
    default: hipLaunchKernelGGL(spatial_variance_kernel<3>, blocks, threads, 0, stream, S); break;
    }
}

// ---------------------------------------------------------------- the frame records (host)
// The record of a sequence before its first frame; -> the workgroups of a launch (at most the pixel count).
uint32_t first_frame_record(AccumulateFrame& F, const p3d_accumulate_params& p) {
    memset(&F, 0, sizeof F);
    F.res_x = p.res_x; F.res_y = p.res_y;
    F.tiles_x = (int32_t)(((int64_t)p.res_x + kTileW - 1) / kTileW); F.tiles_y = (int32_t)(((int64_t)p.res_y + kTileH - 1) / kTileH);
    F.tol = p.depth_tolerance; F.normal_min = p.normal_min; F.max_history = p.max_history;
    return (uint32_t)((uint64_t)F.tiles_x * (uint64_t)F.tiles_y);
}

// Turns the record of frame f - 1 (or of first_frame_record) into that of frame f.  false: frame f has nothing to look back at.
bool next_frame_record(AccumulateFrame& F, const p3d_accumulate_params& p, const AccumulatePlanes& A, const p3d_camera* cams,
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

int accumulate_check_request(const AccumulateRequest& r, const char** why) {
    *why = "";
    const bool variance = r.entry == kAccumulateVariance, moving = r.entry != kAccumulate;     // moving: the wording of the two later entries
    const p3d_accumulate_frames* frames = r.frames;
    const p3d_accumulate_history* history = r.history;
    const p3d_accumulate_motion* motion = r.motion;
    if (!r.params || (variance && !r.variance_params) || !frames || !r.has_out) {
        *why = variance ? "params / variance_params / frames / out is NULL" : "params / frames / out is NULL"; return P3D_ERR_ARG;
    }
    const bool no_output = !r.out_rgb32f && !r.out_length && !r.out_prev_xy && !r.out_moments && !r.out_variance;
    if (variance) {
        if (r.out_memory != 0 && r.out_memory != 1) { *why = "p3d_accumulate_variance_outputs::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
        if (!motion && r.out_prev_xy) { *why = "out->prev_xy needs a motion: without one the world is static and no previous position is formed"; return P3D_ERR_ARG; }
        if (no_output) { *why = "every output plane is NULL"; return P3D_ERR_ARG; }
    }
    // the motion's own rules
    if (r.entry == kAccumulateMoving && !motion) { *why = "motion is NULL: p3d_accumulate is the entry for a static world"; return P3D_ERR_ARG; }
    if (motion) {
        if (!motion->prim_type || !motion->prim_data) { *why = "the motion needs prim_type and prim_data"; return P3D_ERR_ARG; }
        if (motion->n_prims == 0) { *why = "p3d_accumulate_motion::n_prims is 0"; return P3D_ERR_ARG; }
        if (history && !motion->history_prim_data) { *why = "a history needs p3d_accumulate_motion::history_prim_data, the geometry it was rendered with"; return P3D_ERR_ARG; }
        if (motion->memory != 0 && motion->memory != 1) { *why = "p3d_accumulate_motion::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
        if (!frames->hit_id) { *why = "p3d_accumulate_moving needs frames->hit_id: the motion is looked up by it"; return P3D_ERR_ARG; }
    }
    // the planes, memory fields, params, sizes and cameras every entry has
    if (!frames->rgb32f || !frames->depth || !frames->normal) { *why = "the frames need rgb32f, depth and normal"; return P3D_ERR_ARG; }
    if (!frames->cams) { *why = "p3d_accumulate_frames::cams is NULL: every frame needs its camera"; return P3D_ERR_ARG; }
    if (history && (!history->rgb32f || !history->depth || !history->normal || !history->length)) {
        *why = "a history needs rgb32f, depth, normal and length (pass a NULL history for none)"; return P3D_ERR_ARG;
    }
    if (history && !history->cam) { *why = "p3d_accumulate_history::cam is NULL: the history needs the camera it was seen through"; return P3D_ERR_ARG; }
    if (no_output) { *why = moving ? "every output plane is NULL" : "both output planes are NULL"; return P3D_ERR_ARG; }
    if (frames->memory != 0 && frames->memory != 1) { *why = "p3d_accumulate_frames::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (history && history->memory != 0 && history->memory != 1) { *why = "p3d_accumulate_history::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (r.out_memory != 0 && r.out_memory != 1) { *why = moving ? "p3d_accumulate_moving_outputs::memory must be 0 (host) or 1 (device)" : "p3d_accumulate_outputs::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    const p3d_accumulate_params& p = *r.params;
    if (p.res_x < 1 || p.res_y < 1 || p.n_frames < 1) { *why = "res_x, res_y and n_frames must be at least 1"; return P3D_ERR_ARG; }
    if (!std::isfinite(p.depth_tolerance) || !(p.depth_tolerance > 0.0f)) { *why = "depth_tolerance must be finite and positive"; return P3D_ERR_ARG; }
    if (!(p.normal_min >= -1.0f && p.normal_min <= 1.0f)) { *why = "normal_min must be in [-1, 1]"; return P3D_ERR_ARG; }
    if (!std::isfinite(p.max_history) || !(p.max_history >= 1.0f)) { *why = "max_history must be finite and at least 1"; return P3D_ERR_ARG; }
    // 64-bit products of 31-bit factors, compared step by step so that none of them wraps
    const uint64_t limit = 0x7FFFFFFFull, pixels = (uint64_t)p.res_x * (uint64_t)p.res_y;
    if (pixels > limit || pixels * (uint64_t)p.n_frames > limit) { *why = "n_frames * res_x * res_y does not fit 31 bits"; return P3D_ERR_LIMIT; }
    for (int f = 0; f < p.n_frames; f++)
        if (frames->cams[f].res_x != p.res_x || frames->cams[f].res_y != p.res_y) { *why = "a camera of the frames has another res_x / res_y than the params"; return P3D_ERR_ARG; }
    if (history && (history->cam->res_x != p.res_x || history->cam->res_y != p.res_y)) { *why = "the history's camera has another res_x / res_y than the params"; return P3D_ERR_ARG; }
    // aliasing of colour, length and prev_xy: out->rgb32f may be frames->rgb32f (colour onto colour); no other of them may be
    // anything the launches read.  Requests for moments or variance alone have always had the first of these held to the
    // rules (and the words) of out->length as well, ahead of the rules below: they keep their answers.
    const void* olds[3] = {r.out_rgb32f, r.out_length, r.out_prev_xy};
    if (!olds[0] && !olds[1] && !olds[2]) olds[1] = r.out_moments ? r.out_moments : r.out_variance;
    for (int i = 0; i < 3; i++) {
        const void* o = olds[i];
        if (!o) continue;
        if (o == frames->depth || o == frames->normal || o == frames->hit_id) { *why = "an output plane is the frames' depth, normal or hit_id"; return P3D_ERR_ARG; }
        if (history && (o == history->rgb32f || o == history->depth || o == history->normal || o == history->length || o == history->hit_id)) {
            *why = "an output plane is a plane of the history: the launches read it while they write"; return P3D_ERR_ARG;
        }
        if (i > 0 && o == (const void*)frames->rgb32f) { *why = moving ? "out->length or out->prev_xy is the frames' rgb32f" : "out->length is the frames' rgb32f"; return P3D_ERR_ARG; }
        for (int j = 0; j < i; j++)
            if (o == olds[j]) { *why = moving ? "two output planes are one plane" : "out->rgb32f and out->length are one plane"; return P3D_ERR_ARG; }
    }
    if (motion) {
        // the first comparison keeps the product of the second (31 bits x 32 bits x 12) inside 64 bits
        if ((uint64_t)p.n_frames * (uint64_t)motion->n_prims > limit || (uint64_t)p.n_frames * (uint64_t)motion->n_prims * 12 > limit) {
            *why = "n_frames * n_prims * 12 does not fit 31 bits"; return P3D_ERR_LIMIT;
        }
        if (motion->memory == 0)
            for (uint32_t i = 0; i < motion->n_prims; i++)
                if (motion->prim_type[i] > P3D_PLANE) { *why = "a prim_type is not P3D_SPHERE .. P3D_PLANE"; return P3D_ERR_ARG; }
        for (const void* o : olds)
            if (o && (o == motion->prim_type || o == motion->prim_data || o == motion->history_prim_data)) { *why = "an output plane is an array of the motion"; return P3D_ERR_ARG; }
    }
    if (!variance) return P3D_OK;
    if (history && !r.history_moments) { *why = "a history needs history_moments, the moments it had accumulated"; return P3D_ERR_ARG; }
    if (!history && r.history_moments) { *why = "history_moments without a history: pass both or neither"; return P3D_ERR_ARG; }
    const p3d_accumulate_variance_params& v = *r.variance_params;
    if (!std::isfinite(v.min_temporal) || !(v.min_temporal >= 1.0f)) { *why = "min_temporal must be finite and at least 1 (1: no spatial estimate)"; return P3D_ERR_ARG; }
    if (v.radius < 1 || v.radius > kAccumulateVarianceMaxRadius) { *why = "radius must be in 1..3"; return P3D_ERR_ARG; }
    if (!std::isfinite(v.sigma_depth) || !(v.sigma_depth > 0.0f)) { *why = "sigma_depth must be finite and positive"; return P3D_ERR_ARG; }
    if (v.normal_power_log2 < 0 || v.normal_power_log2 > 8) { *why = "normal_power_log2 must be in 0..8"; return P3D_ERR_ARG; }
    // aliasing of the new planes: moments and variance may be nothing the launches read and no other output plane
    const void* const news[2] = {r.out_moments, r.out_variance};
    const void* const others[3] = {r.out_rgb32f, r.out_length, r.out_prev_xy};
    for (int i = 0; i < 2; i++) {
        const void* o = news[i];
        if (!o) continue;
        if (o == frames->rgb32f || o == frames->depth || o == frames->normal || o == frames->hit_id) { *why = "out->moments or out->variance is a plane of the frames"; return P3D_ERR_ARG; }
        if (history && (o == history->rgb32f || o == history->depth || o == history->normal || o == history->length || o == history->hit_id || o == r.history_moments)) {
            *why = "out->moments or out->variance is a plane of the history: the launches read it while they write"; return P3D_ERR_ARG;
        }
        if (motion && (o == motion->prim_type || o == motion->prim_data || o == motion->history_prim_data)) { *why = "out->moments or out->variance is an array of the motion"; return P3D_ERR_ARG; }
        for (const void* q : others) if (o == q) { *why = "two output planes are one plane"; return P3D_ERR_ARG; }
        if (i == 1 && o == news[0]) { *why = "two output planes are one plane"; return P3D_ERR_ARG; }
    }
    if (history)
        for (const void* q : others) if (q && q == r.history_moments) { *why = "an output plane is history_moments: the launches read it while they write"; return P3D_ERR_ARG; }
    return P3D_OK;
}

hipError_t launch_accumulate(const p3d_accumulate_params& p, const AccumulatePlanes& A, const AccumulateMotion* motion,
                             const AccumulateVariance* variance, const p3d_camera* cams, const p3d_camera* hist_cam, hipStream_t stream) {
    const size_t frame = (size_t)p.res_x * (size_t)p.res_y, records = motion ? 12 * (size_t)motion->n_prims : 0;
    const AccumulateVariancePlanes* VP = variance ? &variance->planes : nullptr;
    const bool many = p.n_frames > 1, spatial = variance && accumulate_variance_spatial(variance->params, VP->out_variance);
    const bool detour = variance && accumulate_variance_colour_detour(variance->params, A.rgb32f, A.out_rgb32f, VP->out_variance);
    // the colour of an in-place call goes through the spare plane: the spatial launch still reads the frame's input colour
    AccumulatePlanes B = A;
    if (detour) B.out_rgb32f = nullptr;
    VarianceFrame V;                 // the record of the temporal launch: each kernel is given the part it knows
    memset(&V, 0, sizeof V);
    const uint32_t blocks = first_frame_record(V.M.F, p);
    if (motion) { V.M.type = motion->prim_type; V.M.n_prims = motion->n_prims; }
    SpatialFrame S;
    memset(&S, 0, sizeof S);
    if (spatial) {
        S.res_x = p.res_x; S.res_y = p.res_y;
        S.tiles_x = (int32_t)(((int64_t)p.res_x + kSpatialW - 1) / kSpatialW); S.tiles_y = (int32_t)(((int64_t)p.res_y + kSpatialH - 1) / kSpatialH);
        S.npow = variance->params.normal_power_log2; S.min_temporal = variance->params.min_temporal; S.sigma_depth = variance->params.sigma_depth;
    }
    for (size_t f = 0; f < (size_t)p.n_frames; f++) {
        if (motion) {
            V.M.cur = motion->prim_data + f * records;
            V.M.prev = f > 0 ? motion->prim_data + (f - 1) * records : motion->hist_prim_data;
            V.M.out_xy = motion->out_prev_xy ? motion->out_prev_xy + 2 * f * frame : nullptr;
        }
        if (variance) {
            V.pmoments = f > 0 ? V.out_moments : VP->hist_moments;       // what the launch of frame f - 1 wrote
            V.out_moments = VP->out_moments ? VP->out_moments + 2 * f * frame : (many ? VP->spare_moments + 2 * (f & 1) * frame : nullptr);
            V.out_variance = VP->out_variance ? VP->out_variance + f * frame : nullptr;
        }
        const bool history = next_frame_record(V.M.F, p, B, cams, hist_cam, f);
        // a single frame has no next frame to keep a plane for, but the spatial launch reads the length, and a detour needs its plane
        if (!V.M.F.out_color && detour) V.M.F.out_color = A.spare_rgb32f;
        if (!V.M.F.out_length && spatial) V.M.F.out_length = A.spare_length;
        if (history) launch_temporal<true>(V, motion != nullptr, variance != nullptr, blocks, stream);
        else launch_temporal<false>(V, motion != nullptr, variance != nullptr, blocks, stream);
        if (spatial) {
            S.color = V.M.F.color; S.depth = V.M.F.depth; S.normal = V.M.F.normal;
            S.length = V.M.F.out_length; S.variance = V.out_variance;
            launch_spatial(S, variance->params.radius, stream);
        }
        if (detour) {
            const hipError_t e = hipMemcpyAsync(A.out_rgb32f + 3 * f * frame, V.M.F.out_color, frame * 12, hipMemcpyDeviceToDevice, stream);
            if (e != hipSuccess) return e;
        }
    }
    return hipGetLastError();
}

}  // namespace p3d
