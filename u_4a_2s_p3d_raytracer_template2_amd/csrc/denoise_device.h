// denoise_device.h -- the device code the passes of p3d_denoise (denoise.hip) and of p3d_denoise_variance
// (denoise_variance.hip) share: the pass record in the launch arguments, the tile and its numbering, the taps in LDS and
// in the planes, and the store of a filtered pixel.  The filters themselves (filter_pixel) are each file's own.
// Included by those two files only, inside their own unnamed namespace's reach: every name here has internal linkage.
#ifndef P3D_DENOISE_DEVICE_H
#define P3D_DENOISE_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "denoise.h"
#include "p3d_device_math.h"

namespace p3d {

namespace {

#ifndef P3D_DENOISE_STAGED_MAX_STEP
#define P3D_DENOISE_STAGED_MAX_STEP 2    // passes up to this step (1, 2 or 4) stage their tile in LDS; 0: none.  Measured: DESIGN "Denoising"
#endif
constexpr int kTileW = 32, kTileH = 8, kThreads = kTileW * kTileH;
constexpr int kXcds = 8;

struct DenoisePass {
    const float* color;      // what the pass reads: [frames][res_y][res_x][3]
    const float* depth;      // [frames][res_y][res_x]
    const float* normal;     // [frames][res_y][res_x][3]
    const float* albedo;     // [frames][res_y][res_x][3]
    float* out32;            // what it writes (may be NULL) ...
    uint8_t* out8;           // ... and the quantised colour (the last pass only; else NULL)
    int32_t res_x, res_y, tiles_x, tiles_y;
    int32_t step, npow;
    float sigma_depth, inv_a, inv_c;
};

__device__ __forceinline__ bool valid_depth(float z) { return z > 0.0f && z <= 3.402823466e+38f; }   // finite and > 0; not NaN
__device__ __forceinline__ float max0(float v) { return v > 0.0f ? v : 0.0f; }
__device__ __forceinline__ float lum(V3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
__device__ __forceinline__ constexpr float k1(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// The tile this workgroup runs: XCD x (workgroups x, x + 8, ...) takes the x-th contiguous share of the tiles.
__device__ __forceinline__ uint32_t logical_block() {
    const uint32_t n = gridDim.x, b = blockIdx.x, q = n / kXcds, r = n % kXcds, xcd = b % kXcds;
    return xcd * q + (xcd < r ? xcd : r) + b / kXcds;
}

// A pixel's neighbourhood in LDS: the planes of the tile and its halo, `at` the pixel's own index.
template <int S>
struct LdsTaps {
    static constexpr int W = kTileW + 4 * S, H = kTileH + 4 * S;
    const float *sz, *sn, *sa, *sc;
    int at;
    __device__ __forceinline__ float z(int dx, int dy) const { return sz[at + (dy * W + dx) * S]; }
    __device__ __forceinline__ V3 v3(const float* p, int dx, int dy) const {
        const float* q = p + 3 * (at + (dy * W + dx) * S);
        return mk(q[0], q[1], q[2]);
    }
    __device__ __forceinline__ V3 n(int dx, int dy) const { return v3(sn, dx, dy); }
    __device__ __forceinline__ V3 a(int dx, int dy) const { return v3(sa, dx, dy); }
    __device__ __forceinline__ V3 c(int dx, int dy) const { return v3(sc, dx, dy); }
};

// ... and in the planes themselves (frame bases).  z() answers 0 -- not valid -- outside the frame; n, a and c are read for
// taps with a valid depth only, which lie inside.
struct GlobalTaps {
    const float *pz, *pn, *pa, *pc;
    int32_t x, y, res_x, res_y, step;
    __device__ __forceinline__ size_t index(int dx, int dy) const {
        return (size_t)((int64_t)y + dy * step) * (size_t)res_x + (size_t)((int64_t)x + dx * step);
    }
    __device__ __forceinline__ float z(int dx, int dy) const {
        const int64_t qx = (int64_t)x + dx * step, qy = (int64_t)y + dy * step;
        if (qx < 0 || qx >= res_x || qy < 0 || qy >= res_y) return 0.0f;
        return pz[index(dx, dy)];
    }
    __device__ __forceinline__ V3 v3(const float* p, int dx, int dy) const {
        const float* q = p + 3 * index(dx, dy);
        return mk(q[0], q[1], q[2]);
    }
    __device__ __forceinline__ V3 n(int dx, int dy) const { return v3(pn, dx, dy); }
    __device__ __forceinline__ V3 a(int dx, int dy) const { return v3(pa, dx, dy); }
    __device__ __forceinline__ V3 c(int dx, int dy) const { return v3(pc, dx, dy); }
};

__device__ __forceinline__ void store_pixel(const DenoisePass& P, size_t pixel, V3 c) {
    if (P.out32) { float* o = P.out32 + 3 * pixel; o[0] = c.x; o[1] = c.y; o[2] = c.z; }
    if (P.out8) {
        uint8_t* o = P.out8 + 3 * pixel;
        o[0] = (uint8_t)u8fromfloat(clamp01(c.x)); o[1] = (uint8_t)u8fromfloat(clamp01(c.y)); o[2] = (uint8_t)u8fromfloat(clamp01(c.z));
    }
}

// the workgroup's tile: its corner pixel and the first pixel of its frame
struct Tile { int64_t x0, y0; size_t frame; };
__device__ __forceinline__ Tile this_tile(const DenoisePass& P) {
    const uint32_t b = logical_block(), tx = b % (uint32_t)P.tiles_x, rest = b / (uint32_t)P.tiles_x;
    Tile t;
    t.x0 = (int64_t)tx * kTileW; t.y0 = (int64_t)(rest % (uint32_t)P.tiles_y) * kTileH;
    t.frame = (size_t)(rest / (uint32_t)P.tiles_y) * (size_t)P.res_x * (size_t)P.res_y;
    return t;
}

// HOST: the part of the record every pass of a call shares; -> the workgroups of a launch (at most the pixel count).
inline uint32_t pass_record(DenoisePass& P, const p3d_denoise_params& p, const float* depth, const float* normal, const float* albedo) {
    P.depth = depth; P.normal = normal; P.albedo = albedo;
    P.res_x = p.res_x; P.res_y = p.res_y;
    P.tiles_x = (int32_t)(((int64_t)p.res_x + kTileW - 1) / kTileW); P.tiles_y = (int32_t)(((int64_t)p.res_y + kTileH - 1) / kTileH);
    P.npow = p.normal_power_log2;
    P.sigma_depth = p.sigma_depth;
    P.inv_a = 1.0f / p.sigma_albedo;
    return (uint32_t)((uint64_t)P.tiles_x * (uint64_t)P.tiles_y * (uint64_t)p.n_frames);
}

}  // namespace

}  // namespace p3d
#endif
