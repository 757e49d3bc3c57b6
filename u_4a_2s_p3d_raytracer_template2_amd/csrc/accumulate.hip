// accumulate.hip -- p3d_accumulate: temporal reprojection of history over the AOV planes of a sequence.  A pixel's primary
// hit (the pinhole ray through its centre, times its depth) is projected into the previous frame's camera; the four pixels
// around that point which show the same surface (depth, normal, hit id) give the accumulated colour and its history length
// by bilinear weights, and the current colour is blended in with weight 1 / length.  IEEE basic operations only, in one
// fixed order (DESIGN "Temporal accumulation") -- so the device, the host restatement (host/accumulate_host.cpp) and the
// NumPy one (tests/accumulate_reference.py) agree in every bit.  Built with the ray kernels' flags (-ffp-contract=off,
// correctly rounded division and square root).
//   One launch per frame of the sequence, in stream order: frame f reads what the launch of frame f - 1 wrote.  One thread
//   per pixel; a workgroup of 256 threads owns a tile of kTileW x kTileH pixels.  The taps are read where they lie, through
//   L2 (profiles/denoise_cost.txt: staging does not pay once taps scatter); under a smooth camera motion the taps of
//   neighbouring pixels are neighbours.  The tile is 64 x 4: a wave is ONE row of 64 pixels, so its own 12-byte pixels and,
//   mostly, its taps are contiguous runs of 768 bytes.  Compact 2-D footprints were tried and lost: 32 x 8 (a wave 32 x 2)
//   is 1 % slower, 16 x 16 (16 x 4) 8 %, 8 x 32 (8 x 8) 37 % -- their rows are fragments of cache lines, and the four taps of
//   a pixel overlap those of its row neighbours whatever the tile (profiles/accumulate_cost.txt).  Workgroups are numbered
//   so that each XCD (workgroup index mod 8) runs a contiguous range of tiles.
//   Both cameras travel in the launch arguments: no camera buffer exists on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
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

// One pixel with a frame to look back at: DESIGN "Temporal accumulation", operation by operation.  false: no history.
__device__ __forceinline__ bool reproject(const AccumulateFrame& F, int32_t x, int32_t y, size_t pixel, V3 C, float Z, V3& out, float& len) {
    if (!valid_depth(Z)) return false;
    // 1. the ray of the frame kernels and the point it reaches (p3d_pinhole.h)
    const V3 d = pinhole_dir(F.uw, F.vh, F.vz, x, y, F.res_x, F.res_y);
    const V3 P = pinhole_point(F.eye, d, Z);
    // 2. its hit seen through the previous camera
    const V3 q = mk(P.x - F.peye[0], P.y - F.peye[1], P.z - F.peye[2]);
    const float a = (q.x * F.pu[0] + q.y * F.pu[1]) + q.z * F.pu[2];
    const float b = (q.x * F.pv[0] + q.y * F.pv[1]) + q.z * F.pv[2];
    const float c = -((q.x * F.pn[0] + q.y * F.pn[1]) + q.z * F.pn[2]);
    if (!(c > 0.0f)) return false;
    const float s = fdiv(c, F.ppd);
    const float gx = fdiv(a, F.pw * s), gy = fdiv(b, F.ph * s);
    const float rx = (float)F.res_x, ry = (float)F.res_y;
    const float px = (gx + 0.5f) * rx - 0.5f, py = (gy + 0.5f) * ry - 0.5f;
    if (!(px > -1.0f && px < rx && py > -1.0f && py < ry)) return false;      // NaN too; below, -1 <= floor < 2^31
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

template <bool HISTORY>
__global__ void __launch_bounds__(kThreads) accumulate_kernel(AccumulateFrame F) {
    const uint32_t blk = logical_block(), tile_x = blk % (uint32_t)F.tiles_x, tile_y = blk / (uint32_t)F.tiles_x;
    const int64_t x = (int64_t)tile_x * kTileW + (int)threadIdx.x % kTileW, y = (int64_t)tile_y * kTileH + (int)threadIdx.x / kTileW;
    if (x >= F.res_x || y >= F.res_y) return;
    const size_t pixel = (size_t)y * (size_t)F.res_x + (size_t)x;
    const float* cp = F.color + 3 * pixel;
    const V3 C = mk(cp[0], cp[1], cp[2]);            // read before anything is written: out_color may be color
    V3 out = C;
    float len = 1.0f;
    if (HISTORY) {
        V3 o; float l;
        if (reproject(F, (int32_t)x, (int32_t)y, pixel, C, F.depth[pixel], o, l)) { out = o; len = l; }
    }
    if (F.out_color) { float* o = F.out_color + 3 * pixel; o[0] = out.x; o[1] = out.y; o[2] = out.z; }
    if (F.out_length) F.out_length[pixel] = len;
}

}  // namespace

int accumulate_check_request(const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                             const p3d_accumulate_history* history, const p3d_accumulate_outputs* out, const char** why) {
    *why = "";
    if (!params || !frames || !out) { *why = "params / frames / out is NULL"; return P3D_ERR_ARG; }
    if (!frames->rgb32f || !frames->depth || !frames->normal) { *why = "the frames need rgb32f, depth and normal"; return P3D_ERR_ARG; }
    if (!frames->cams) { *why = "p3d_accumulate_frames::cams is NULL: every frame needs its camera"; return P3D_ERR_ARG; }
    if (history && (!history->rgb32f || !history->depth || !history->normal || !history->length)) {
        *why = "a history needs rgb32f, depth, normal and length (pass a NULL history for none)"; return P3D_ERR_ARG;
    }
    if (history && !history->cam) { *why = "p3d_accumulate_history::cam is NULL: the history needs the camera it was seen through"; return P3D_ERR_ARG; }
    if (!out->rgb32f && !out->length) { *why = "both output planes are NULL"; return P3D_ERR_ARG; }
    if (frames->memory != 0 && frames->memory != 1) { *why = "p3d_accumulate_frames::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (history && history->memory != 0 && history->memory != 1) { *why = "p3d_accumulate_history::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (out->memory != 0 && out->memory != 1) { *why = "p3d_accumulate_outputs::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    const p3d_accumulate_params& p = *params;
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
    // aliasing: an output plane may be frames->rgb32f (colour onto colour) and nothing else the launches read
    const void* const outs[2] = {out->rgb32f, out->length};
    for (int i = 0; i < 2; i++) {
        const void* o = outs[i];
        if (!o) continue;
        if (o == frames->depth || o == frames->normal || o == frames->hit_id) { *why = "an output plane is the frames' depth, normal or hit_id"; return P3D_ERR_ARG; }
        if (history && (o == history->rgb32f || o == history->depth || o == history->normal || o == history->length || o == history->hit_id)) {
            *why = "an output plane is a plane of the history: the launches read it while they write"; return P3D_ERR_ARG;
        }
    }
    if (out->length && (const void*)out->length == (const void*)frames->rgb32f) { *why = "out->length is the frames' rgb32f"; return P3D_ERR_ARG; }
    if (out->rgb32f && out->rgb32f == out->length) { *why = "out->rgb32f and out->length are one plane"; return P3D_ERR_ARG; }
    return P3D_OK;
}

hipError_t launch_accumulate(const p3d_accumulate_params& p, const AccumulatePlanes& A, const p3d_camera* cams,
                             const p3d_camera* hist_cam, hipStream_t stream) {
    const size_t frame = (size_t)p.res_x * (size_t)p.res_y;
    AccumulateFrame F;
    memset(&F, 0, sizeof F);
    F.res_x = p.res_x; F.res_y = p.res_y;
    F.tiles_x = (int32_t)(((int64_t)p.res_x + kTileW - 1) / kTileW); F.tiles_y = (int32_t)(((int64_t)p.res_y + kTileH - 1) / kTileH);
    F.tol = p.depth_tolerance; F.normal_min = p.normal_min; F.max_history = p.max_history;
    const uint32_t blocks = (uint32_t)((uint64_t)F.tiles_x * (uint64_t)F.tiles_y);      // at most the pixel count
    for (size_t f = 0; f < (size_t)p.n_frames; f++) {
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
        if (pc) {
            for (int k = 0; k < 3; k++) { F.peye[k] = pc->eye[k]; F.pu[k] = pc->u[k]; F.pv[k] = pc->v[k]; F.pn[k] = pc->n[k]; }
            F.pw = pc->w; F.ph = pc->h; F.ppd = pc->plane_dist;
            hipLaunchKernelGGL(accumulate_kernel<true>, dim3(blocks), dim3(kThreads), 0, stream, F);
        } else {
            hipLaunchKernelGGL(accumulate_kernel<false>, dim3(blocks), dim3(kThreads), 0, stream, F);
        }
    }
    return hipGetLastError();
}

}  // namespace p3d
