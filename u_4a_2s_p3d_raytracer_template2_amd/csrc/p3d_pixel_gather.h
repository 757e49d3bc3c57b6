// p3d_pixel_gather.h -- what the per-pixel gather kernels (wf_ao_kernel of ao.hip, wf_indirect_kernel of indirect.hip,
// wf_indirect_paths_kernel of indirect_paths.hip) do alike: the lane mapping and the origin of a pixel's rays on the device,
// the choice among a kernel's five builds and the launch on the host.  IO is AoIO, IndirectIO or PathIO
// (p3d_device_types.h): of it the code reads what they have in common.
//   Lane mapping: a lane is one (pixel, sample); the S lanes of a pixel are consecutive and a wave covers 64 / S consecutive
//   pixels of one row.  The workgroup of a scene served from LDS is 4 such waves of one row.  All frames of a call go in ONE
//   launch; workgroup index = (frame, row, group of the row), the frame slowest.  (LANE_PER_PIXEL: the mapping ao.hip
//   measures against it, a lane is a pixel.)
#ifndef P3D_PIXEL_GATHER_H
#define P3D_PIXEL_GATHER_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_launch.h"
#include "p3d_pinhole.h"
#include "p3d_scene_view.h"

namespace p3d {

// A lane's pixel, in steps with the kernel's two wave-uniform branches between them:
//   in_row = gather_lane();                            if (__ballot(in_row) == 0) return;   -- a wave past the row's end
//   gather_surface(); need = in_row && valid_depth(Z); if (__ballot(need) != 0) {           -- a wave without a query skips the walk
//   gather_origin();  pk = gather_key();               ...
// The steps are cut where they are, and in_row, need and pk are the kernels' own values instead of members, because the
// kernels then compile to the bytes they had when every step stood in them (tools/kdiff.py): one function for the origin
// and the key, or `need` formed in gather_surface(), reorders instructions of one build or another.
struct PixelGather {
    uint32_t f, y, x, lane, S;      // gather_lane: frame, row, column; lane of the wave; samples per pixel
    size_t pixel;                   // gather_surface: index into the planes
    V3 N; float Z;                  // ... their normal and depth
    V3 Ns, O;                       // gather_origin: the normal facing the eye, the origin biased along it
};

// workgroup -> (frame, row, group of the row), all wave-uniform, then the lane's pixel.  Returns in_row: the lane has one.
template <bool LDS, bool LANE_PER_PIXEL, typename IO>
__device__ inline bool gather_lane(const IO& A, PixelGather& g) {
    const uint32_t group = blockIdx.x % A.row_groups, fy = blockIdx.x / A.row_groups;
    g.y = fy % (uint32_t)A.res_y; g.f = fy / (uint32_t)A.res_y;
    g.lane = threadIdx.x & 63u;
    const uint32_t wave = group * (LDS ? 4u : 1u) + (threadIdx.x >> 6);
    g.S = 1u << A.log2_samples;
    // (x < res_x + 64 <= 2^31 + 63: the host keeps n * res_y * res_x * samples below 2^31)
    g.x = LANE_PER_PIXEL ? wave * 64u + g.lane : wave * (64u >> A.log2_samples) + (g.lane >> A.log2_samples);
    return g.x < (uint32_t)A.res_x;
}

// The pixel's index, Z and N.  (1. an invalid depth: no query -- the kernel's `need`.)
template <typename IO>
__device__ inline void gather_surface(const IO& A, bool in_row, PixelGather& g) {
    g.pixel = ((size_t)g.f * (size_t)A.res_y + g.y) * (size_t)A.res_x + g.x;
    g.Z = 0.0f;
    g.N = mk(0.0f, 0.0f, 0.0f);
    if (in_row) {                                                // row tails neither read nor write
        g.Z = A.depth[g.pixel];
        const float* n = A.normal + 3 * g.pixel;
        g.N = mk(n[0], n[1], n[2]);
    }
}

// 2. the hit point, 3. the normal facing the eye and the origin.  For a wave with a query; lanes without one stay for the
// wave-wide walk steps, and the kernel gives them an origin.
template <typename IO>
__device__ inline void gather_origin(const IO& A, PixelGather& g) {
    const FrameCam& C = A.cams[g.f];
    const V3 d = pinhole_dir(C.uw, C.vh, C.vz, (int32_t)g.x, (int32_t)g.y, A.res_x, A.res_y);
    const V3 Pt = pinhole_point(C.eye, d, g.Z);
    const bool away = (g.N.x * d.x + g.N.y * d.y) + g.N.z * d.z > 0.0f;
    g.Ns = away ? mk(-g.N.x, -g.N.y, -g.N.z) : g.N;
    g.O = mk(Pt.x + g.Ns.x * A.bias, Pt.y + g.Ns.y * A.bias, Pt.z + g.Ns.z * A.bias);
}

// 4. the pixel's key of the random streams
template <typename IO>
__device__ inline uint32_t gather_key(const IO& A, const PixelGather& g) { return rng_mix(A.seed + g.f, g.y * (uint32_t)A.res_x + g.x); }

// The build of a gather kernel that serves `request` at level L.  K<LDS, WALK>::fn() is the address of the kernel's build for
// a scene placement and a walk, at OCC = 1 for the grid walk and kRaysOcc otherwise (kGatherOcc).  The five builds:
// LDS x {lane, grid}, HBM x {lane, shared, grid}.
template <int WALK> constexpr int kGatherOcc = WALK == WALK_GRID ? 1 : kRaysOcc;
template <template <bool, int> class K, Level L>
const void* pixel_gather_kernel_for(const KernelVariant& request) {
    const KernelVariant v = canonical_level(request, L);
    if (v.lds) return v.walk == WALK_GRID ? K<true, WALK_GRID>::fn() : v.walk == WALK_LANE ? K<true, WALK_LANE>::fn() : nullptr;
    return v.walk == WALK_GRID ? K<false, WALK_GRID>::fn() : v.walk == WALK_SHARED ? K<false, WALK_SHARED>::fn()
           : v.walk == WALK_LANE ? K<false, WALK_LANE>::fn() : nullptr;
}

// That build's launch: one workgroup per wg_waves waves of a row, all frames at once; a wave covers per_wave pixels
// (io.row_waves and io.row_groups are set here).
template <template <bool, int> class K, Level L, typename IO>
hipError_t launch_pixel_gather(LaunchParams P, IO io, const KernelVariant& v, uint32_t per_wave, hipStream_t stream) {
    const void* fn = pixel_gather_kernel_for<K, L>(v);
    if (!fn) return hipErrorInvalidDeviceFunction;
    const size_t shmem = wavefront_lds_bytes(P, v.lds);
    hipError_t e = allow_lds(fn, shmem);
    if (e != hipSuccess) return e;
    io.row_waves = (uint32_t)(((uint64_t)io.res_x + per_wave - 1) / per_wave);
    io.row_groups = (io.row_waves + (uint32_t)P.wg_waves - 1) / (uint32_t)P.wg_waves;
    void* args[] = {&P, &io};
    const uint64_t blocks = (uint64_t)io.n_frames * (uint64_t)io.res_y * io.row_groups;      // at most the pixel count
    return hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(64u * (unsigned)P.wg_waves), args, shmem, stream);
}

}  // namespace p3d
#endif
