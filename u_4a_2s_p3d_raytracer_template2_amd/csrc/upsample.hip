// upsample.hip -- p3d_upsample: joint bilateral upsampling (Kopf et al. 2007) of a low-resolution plane along the full
// frame's depth and normal.  The four bilinear taps of a full-resolution pixel are weighted by the denoiser's depth and
// normal stops -- squares of clamped linear ramps, IEEE basic operations only, in one fixed order (DESIGN "Guided
// upsampling") -- so the device, the host restatement (host/upsample_host.cpp) and the NumPy one
// (tests/upsample_reference.py) agree in every bit.  Built with the ray kernels' flags (-ffp-contract=off, correctly rounded
// division).
//   ONE launch, all frames of a batch in it; a workgroup of 256 threads owns denoise.hip's tile of 32 x 8 pixels, here of
//   the FULL resolution.  The kernel is a template of the factor s and of the channel count c: the tap index and its
//   fraction are divisions by a constant.
//   The low pixels a tile's taps can reach -- at most (31 / s + 3) x (7 / s + 3) of them, 16 + 4 c bytes each: 34 x 10 at
//   s = 1, 18 x 6 at s = 2 -- are copied into LDS first, every plane in its own layout (depth [H][W], the others [H][W][3]
//   or [H][W][c]), row by row in coalesced dwords, as denoise_staged_kernel does; a texel outside the low frame is stored as
//   0 and never read as a tap (a lane knows from the tap's coordinates that it lies outside).  Every lane reads its own Z_p and
//   N_p from the full-resolution planes (coalesced; asked for before the staging, so that the two latencies overlap) and
//   runs the four taps from LDS.
//   P3D_UPSAMPLE_STAGED=0 builds the other variant: no LDS, the four taps read through the vector cache, where s
//   neighbouring lanes share a texel.
//   Workgroups are numbered as the denoiser's (denoise_device.h): each XCD runs a contiguous range of tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "denoise_device.h"
#include "p3d_device_math.h"
#include "upsample.h"

#ifndef P3D_UPSAMPLE_STAGED
#define P3D_UPSAMPLE_STAGED 1    // 1: the tile's low footprint is staged in LDS; 0: taps read where they lie.  Measured: DESIGN "Guided upsampling"
#endif

namespace p3d {

namespace {

struct UpsamplePass {
    const float* low;          // [frames][res_y][res_x][c]
    const float* low_depth;    // [frames][res_y][res_x]
    const float* low_normal;   // [frames][res_y][res_x][3]
    const float* depth;        // [frames][res_y s][res_x s]
    const float* normal;       // [frames][res_y s][res_x s][3]
    float* plane;              // [frames][res_y s][res_x s][c] (may be NULL)
    uint8_t* fallback;         // [frames][res_y s][res_x s] (may be NULL)
    int32_t res_x, res_y;      // the LOW resolution
    int32_t tiles_x, tiles_y;  // tiles of the full resolution
    int32_t npow;
    float sigma_depth;
};

// One axis of a pixel's taps: t = 2 x + 1 - s, i0 = floor(t / 2s), r = t - 2s i0.  t + 2s = 2 x + 1 + s is positive and below
// 2^32 (x < 2^31), so the floor division is an unsigned one, by a constant.
template <int S>
__device__ __forceinline__ void axis_taps(uint32_t x, int32_t& i0, uint32_t& r) {
    const uint32_t u = 2u * x + (uint32_t)(1 + S), q = u / (uint32_t)(2 * S);
    i0 = (int32_t)q - 1;
    r = u - (uint32_t)(2 * S) * q;
}

// The low pixels a pixel's taps read: staged in LDS (the footprint's corner at (lx0, ly0), rows of W texels) ...
template <int S, int C>
struct LdsLow {
    static constexpr int W = (kTileW - 1) / S + 3, H = (kTileH - 1) / S + 3;
    const float *sz, *sn, *sc;
    int32_t lx0, ly0;
    __device__ __forceinline__ int at(int32_t i, int32_t j) const { return (j - ly0) * W + (i - lx0); }
    __device__ __forceinline__ float z(int32_t i, int32_t j) const { return sz[at(i, j)]; }
    __device__ __forceinline__ V3 n(int32_t i, int32_t j) const { const float* q = sn + 3 * at(i, j); return mk(q[0], q[1], q[2]); }
    __device__ __forceinline__ float c(int32_t i, int32_t j, int k) const { return sc[C * at(i, j) + k]; }
};

// ... or in the planes themselves (frame bases)
template <int C>
struct GlobalLow {
    const float *pz, *pn, *pc;
    int32_t res_x;
    __device__ __forceinline__ size_t at(int32_t i, int32_t j) const { return (size_t)j * (size_t)res_x + (size_t)i; }
    __device__ __forceinline__ float z(int32_t i, int32_t j) const { return pz[at(i, j)]; }
    __device__ __forceinline__ V3 n(int32_t i, int32_t j) const { const float* q = pn + 3 * at(i, j); return mk(q[0], q[1], q[2]); }
    __device__ __forceinline__ float c(int32_t i, int32_t j, int k) const { return pc[C * at(i, j) + k]; }
};

// One pixel: DESIGN "Guided upsampling", operation by operation.  The taps run dy outer, dx inner: the sums depend on it.
// The guided sums and the plain bilinear ones are formed side by side; each is the definition's own sequence of operations.
template <int S, int C, typename Low>
__device__ __forceinline__ bool upsample_pixel(const Low& T, const UpsamplePass& P, uint32_t x, uint32_t y, float zp, V3 np, float (&out)[C]) {
    int32_t i0, j0;
    uint32_t rx, ry;
    axis_taps<S>(x, i0, rx);
    axis_taps<S>(y, j0, ry);
    const float fx = (float)rx / (float)(2 * S), fy = (float)ry / (float)(2 * S);
    const float bx[2] = {1.0f - fx, fx}, by[2] = {1.0f - fy, fy};
    const bool centre = valid_depth(zp);
    const float inv_z = centre ? 1.0f / (P.sigma_depth * zp) : 0.0f;
    float sum[C], bsum[C], sw = 0.0f, bsw = 0.0f;
#pragma unroll
    for (int k = 0; k < C; k++) sum[k] = bsum[k] = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const int32_t i = i0 + dx, j = j0 + dy;
            if (i < 0 || i >= P.res_x || j < 0 || j >= P.res_y) continue;
            const float b = bx[dx] * by[dy];
            float cq[C];
#pragma unroll
            for (int k = 0; k < C; k++) cq[k] = T.c(i, j, k);
#pragma unroll
            for (int k = 0; k < C; k++) bsum[k] = bsum[k] + b * cq[k];
            bsw = bsw + b;
            const float zq = T.z(i, j);
            float w = b;
            if (centre) {
                if (!valid_depth(zq)) continue;
                const V3 nq = T.n(i, j);
                const float tz = max0(1.0f - fabsf(zq - zp) * inv_z), wz = tz * tz;
                const float dn = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
                float wn = max0(dn);
                for (int e = 0; e < P.npow; e++) wn = wn * wn;
                w = (b * wz) * wn;
            } else if (valid_depth(zq)) continue;
#pragma unroll
            for (int k = 0; k < C; k++) sum[k] = sum[k] + w * cq[k];
            sw = sw + w;
        }
    }
    const bool explained = sw > 0.0f;
    const float den = explained ? sw : bsw;           // one division per channel: the sums are chosen first
#pragma unroll
    for (int k = 0; k < C; k++) out[k] = (explained ? sum[k] : bsum[k]) / den;
    return !explained;
}

template <int S, int C>
__global__ void __launch_bounds__(kThreads) upsample_kernel(UpsamplePass P) {
    const uint32_t blk = logical_block(), tx = blk % (uint32_t)P.tiles_x, rest = blk / (uint32_t)P.tiles_x;
    const uint32_t x0 = tx * kTileW, y0 = (rest % (uint32_t)P.tiles_y) * kTileH, frame = rest / (uint32_t)P.tiles_y;
    const size_t low_frame = (size_t)frame * (size_t)P.res_x * (size_t)P.res_y;
    const uint32_t W = (uint32_t)P.res_x * S, H = (uint32_t)P.res_y * S;
    const int tid = (int)threadIdx.x;
    // the pixel's own depth and normal are asked for first: their latency passes while the footprint is staged
    const uint32_t x = x0 + (uint32_t)(tid % kTileW), y = y0 + (uint32_t)(tid / kTileW);
    const bool inside = x < W && y < H;
    const size_t pixel = (size_t)frame * (size_t)W * (size_t)H + (size_t)y * (size_t)W + (size_t)x;
    float zp = 0.0f;
    V3 np = mk(0.0f, 0.0f, 0.0f);
    if (inside) {
        const float* n = P.normal + 3 * pixel;
        zp = P.depth[pixel];
        np = mk(n[0], n[1], n[2]);
    }
#if P3D_UPSAMPLE_STAGED
    using Low = LdsLow<S, C>;
    constexpr int LW = Low::W, LH = Low::H;
    __shared__ float sz[LW * LH], sn[3 * LW * LH], sc[C * LW * LH];
    int32_t lx0, ly0;
    uint32_t unused;
    axis_taps<S>(x0, lx0, unused);          // the first tap of the tile's first column and row: may be -1
    axis_taps<S>(y0, ly0, unused);
    for (int i = tid; i < LW * LH; i += kThreads) {
        const int32_t gy = ly0 + i / LW, gx = lx0 + i % LW;
        const bool in = gy >= 0 && gy < P.res_y && gx >= 0 && gx < P.res_x;
        sz[i] = in ? P.low_depth[low_frame + (size_t)gy * (size_t)P.res_x + (size_t)gx] : 0.0f;
    }
    for (int i = tid; i < 3 * LW * LH; i += kThreads) {            // rows of 3 LW floats, as they lie in the plane
        const int32_t gy = ly0 + i / (3 * LW);
        const int64_t g3 = 3 * (int64_t)lx0 + i % (3 * LW);
        const bool in = gy >= 0 && gy < P.res_y && g3 >= 0 && g3 < 3 * (int64_t)P.res_x;
        sn[i] = in ? P.low_normal[3 * (low_frame + (size_t)gy * (size_t)P.res_x) + (size_t)g3] : 0.0f;
    }
    for (int i = tid; i < C * LW * LH; i += kThreads) {
        const int32_t gy = ly0 + i / (C * LW);
        const int64_t gc = C * (int64_t)lx0 + i % (C * LW);
        const bool in = gy >= 0 && gy < P.res_y && gc >= 0 && gc < C * (int64_t)P.res_x;
        sc[i] = in ? P.low[C * (low_frame + (size_t)gy * (size_t)P.res_x) + (size_t)gc] : 0.0f;
    }
    __syncthreads();
    const Low taps = {sz, sn, sc, lx0, ly0};
#else
    const GlobalLow<C> taps = {P.low_depth + low_frame, P.low_normal + 3 * low_frame, P.low + C * low_frame, P.res_x};
#endif
    if (!inside) return;
    float out[C];
    const bool fell_back = upsample_pixel<S, C>(taps, P, x, y, zp, np, out);
    if (P.plane) {
#pragma unroll
        for (int k = 0; k < C; k++) P.plane[C * pixel + k] = out[k];
    }
    if (P.fallback) P.fallback[pixel] = fell_back ? (uint8_t)1 : (uint8_t)0;
}

template <int C>
void launch_factor(const UpsamplePass& P, int factor, uint32_t blocks, hipStream_t stream) {
    switch (factor) {
    case 1: hipLaunchKernelGGL((upsample_kernel<1, C>), dim3(blocks), dim3(kThreads), 0, stream, P); break;
    case 2: hipLaunchKernelGGL((upsample_kernel<2, C>), dim3(blocks), dim3(kThreads), 0, stream, P); break;
    case 3: hipLaunchKernelGGL((upsample_kernel<3, C>), dim3(blocks), dim3(kThreads), 0, stream, P); break;
    default: hipLaunchKernelGGL((upsample_kernel<4, C>), dim3(blocks), dim3(kThreads), 0, stream, P); break;
    }
}

}  // namespace

hipError_t launch_upsample(const p3d_upsample_params& p, const float* low, const float* low_depth, const float* low_normal,
                           const float* depth, const float* normal, float* out_plane, uint8_t* out_fallback, hipStream_t stream) {
    UpsamplePass P;
    P.low = low; P.low_depth = low_depth; P.low_normal = low_normal; P.depth = depth; P.normal = normal;
    P.plane = out_plane; P.fallback = out_fallback;
    P.res_x = p.res_x; P.res_y = p.res_y;
    const int64_t W = (int64_t)p.res_x * p.factor, H = (int64_t)p.res_y * p.factor;
    P.tiles_x = (int32_t)((W + kTileW - 1) / kTileW); P.tiles_y = (int32_t)((H + kTileH - 1) / kTileH);
    P.npow = p.normal_power_log2;
    P.sigma_depth = p.sigma_depth;
    const uint32_t blocks = (uint32_t)((uint64_t)P.tiles_x * (uint64_t)P.tiles_y * (uint64_t)p.n_frames);   // at most the pixel count
    if (p.channels == 1) launch_factor<1>(P, p.factor, blocks, stream); else launch_factor<3>(P, p.factor, blocks, stream);
    return hipGetLastError();
}

}  // namespace p3d
