// ao.hip -- p3d_ambient_occlusion: hemisphere any-hit queries fused per pixel.  A pixel's primary hit (the pinhole ray
// through its centre times its depth, p3d_pinhole.h) is the origin of `samples` cosine-weighted segments of length
// `radius`; each is what p3d_occluded would be asked -- shadow_segment() / light_occluded() of p3d_shade.h, as
// wf_occlusion_kernel calls them -- and the pixel's ambient occlusion is the share that is not occluded.  The segments are
// made in lanes from the depth and normal planes and the counter-based random streams of p3d_shade.h and never exist in
// memory.  The definition, operation by operation: include/p3d_hip.h; the host restatement: host/ao_host.cpp.
//   Lane mapping: a lane is one (pixel, sample); the S lanes of a pixel are consecutive and a wave covers 64 / S consecutive
//   pixels of one row, so a lane group shares its origin and its rays start coherent.  The S lanes of a pixel read the same
//   Z and N (64 / S distinct addresses per wave), the count is a popcount of the wave's ballot under the group's mask, and
//   lane 0 of the group writes: no atomics, no LDS for the count.  The workgroup of a scene served from LDS is 4 such waves
//   of one row.  All frames of a call go in ONE launch; workgroup index = (frame, row, group of the row), the frame
//   slowest; the frames' cameras are read from a device buffer a launch of the same stream wrote (launch_frame_cams).
//   -DP3D_AO_LANE_PER_PIXEL=1 builds the mapping that was measured against it: a lane is a pixel and loops over its samples
//   (DESIGN "Ambient occlusion").
//   One build per scene placement and walk (p3d_kernel_variant.h: Level::AmbientOcclusion).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_ao_segment.h"
#include "p3d_launch.h"
#include "p3d_pinhole.h"
#include "p3d_scene_view.h"

namespace p3d {

namespace {

#ifndef P3D_AO_LANE_PER_PIXEL
#define P3D_AO_LANE_PER_PIXEL 0          // 1: a lane is a pixel and loops over its samples.  Measured: DESIGN "Ambient occlusion"
#endif
constexpr bool kLanePerPixel = P3D_AO_LANE_PER_PIXEL != 0;

template <bool LDS, int WALK, int OCC>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void wf_ao_kernel(const LaunchParams P, const AoIO A) {
    const typename View<LDS>::type sv = View<LDS>::make(P);
    // workgroup -> (frame, row, group of the row); all wave-uniform
    const uint32_t group = blockIdx.x % A.row_groups, fy = blockIdx.x / A.row_groups;
    const uint32_t y = fy % (uint32_t)A.res_y, f = fy / (uint32_t)A.res_y;
    const uint32_t lane = threadIdx.x & 63u, wave = group * (LDS ? 4u : 1u) + (threadIdx.x >> 6);
    const uint32_t S = 1u << A.log2_samples;
    // (x < res_x + 64 <= 2^31 + 63: the host keeps n * res_y * res_x * samples below 2^31)
    const uint32_t x = kLanePerPixel ? wave * 64u + lane : wave * (64u >> A.log2_samples) + (lane >> A.log2_samples);
    const bool in_row = x < (uint32_t)A.res_x;
    if (__ballot(in_row) == 0) return;                           // past the row's end; no barrier follows the scene copy's
    const size_t pixel = ((size_t)f * (size_t)A.res_y + y) * (size_t)A.res_x + x;
    float Z = 0.0f;
    V3 N = mk(0.0f, 0.0f, 0.0f);
    if (in_row) {                                                // row tails neither read nor write
        Z = A.depth[pixel];
        const float* n = A.normal + 3 * pixel;
        N = mk(n[0], n[1], n[2]);
    }
    const bool need = in_row && valid_depth(Z);                  // 1. an invalid depth: no query, ao = 1
    uint32_t occ = 0;
    if (__ballot(need) != 0) {                                   // a wave without a query skips the walk
        const FrameCam& C = A.cams[f];
        // 2. the hit point, 3. the normal facing the eye and the origin
        const V3 d = pinhole_dir(C.uw, C.vh, C.vz, (int32_t)x, (int32_t)y, A.res_x, A.res_y);
        const V3 Pt = pinhole_point(C.eye, d, Z);
        const bool away = (N.x * d.x + N.y * d.y) + N.z * d.z > 0.0f;
        const V3 Ns = away ? mk(-N.x, -N.y, -N.z) : N;
        V3 O = mk(Pt.x + Ns.x * A.bias, Pt.y + Ns.y * A.bias, Pt.z + Ns.z * A.bias);
        if (!need) O = mk(0.0f, 0.0f, 0.0f);                     // lanes without a query stay for the wave-wide walk steps
        const uint32_t pk = rng_mix(A.seed + f, y * (uint32_t)A.res_x + x);      // 4.
        TravCtx tc = wave_stack<LDS>(P, 0);
        Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
        if (kLanePerPixel) {
#pragma nounroll
            for (uint32_t s = 0; s < S; s++) {
                V3 L = ao_segment(Ns, pk, s, A.radius, need);
                if (!need) L = mk(1.0f, 0.0f, 0.0f);
                { Ray given; given.o = O; given.d = L; tc.lane.walk_all = !slab_can_cull(given); }
                occ += light_occluded<false, WALK>(P, sv, shadow_segment(L), O, need, tc, ctr) && need ? 1u : 0u;
            }
        } else {
            V3 L = ao_segment(Ns, pk, lane & (S - 1u), A.radius, need);
            if (!need) L = mk(1.0f, 0.0f, 0.0f);
            // 7. the query of wf_occlusion_kernel on (O, L)
            { Ray given; given.o = O; given.d = L; tc.lane.walk_all = !slab_can_cull(given); }
            const bool occluded = light_occluded<false, WALK>(P, sv, shadow_segment(L), O, need, tc, ctr);
            const uint64_t mine = (S == 64u ? ~0ull : (1ull << S) - 1ull) << (lane & ~(S - 1u));
            occ = (uint32_t)__popcll(__ballot(need && occluded) & mine);
        }
    }
    // 8. lane 0 of the pixel's group writes
    if (!in_row || (!kLanePerPixel && (lane & (S - 1u)) != 0u)) return;
    const float ao = fdiv((float)(S - occ), (float)S);
    if (A.ao) A.ao[pixel] = ao;
    if (A.rgb) {
        V3 c = mk(ao, ao, ao);
        if (A.color) { const float* in = A.color + 3 * pixel; c = mk(ao * in[0], ao * in[1], ao * in[2]); }
        float* o = A.rgb + 3 * pixel;
        o[0] = c.x; o[1] = c.y; o[2] = c.z;
    }
}

using AoKernelFn = void (*)(const LaunchParams, const AoIO);
template <bool LDS, int WALK> constexpr AoKernelFn ao_kernel() { return wf_ao_kernel<LDS, WALK, WALK == WALK_GRID ? 1 : kRaysOcc>; }

// the five builds: LDS x {lane, grid}, HBM x {lane, shared, grid}
const void* ao_kernel_for(const KernelVariant& request) {
    const KernelVariant v = canonical_level(request, Level::AmbientOcclusion);
    AoKernelFn fn = nullptr;
    if (v.lds) fn = v.walk == WALK_GRID ? ao_kernel<true, WALK_GRID>() : v.walk == WALK_LANE ? ao_kernel<true, WALK_LANE>() : nullptr;
    else fn = v.walk == WALK_GRID ? ao_kernel<false, WALK_GRID>() : v.walk == WALK_SHARED ? ao_kernel<false, WALK_SHARED>()
              : v.walk == WALK_LANE ? ao_kernel<false, WALK_LANE>() : nullptr;
    return reinterpret_cast<const void*>(fn);
}

}  // namespace

// p3d_ambient_occlusion: one workgroup per wg_waves waves of a row, all frames in one launch (A.row_waves and A.row_groups
// are set here)
hipError_t launch_wf_ao(const LaunchParams& P, const AoIO& A, const KernelVariant& v, hipStream_t stream) {
    const void* fn = ao_kernel_for(v);
    if (!fn) return hipErrorInvalidDeviceFunction;
    const size_t shmem = wavefront_lds_bytes(P, v.lds);
    hipError_t e = allow_lds(fn, shmem);
    if (e != hipSuccess) return e;
    LaunchParams Pc = P;
    AoIO Ac = A;
    const uint32_t per_wave = kLanePerPixel ? 64u : 64u >> A.log2_samples;
    Ac.row_waves = (uint32_t)(((uint64_t)A.res_x + per_wave - 1) / per_wave);
    Ac.row_groups = (Ac.row_waves + (uint32_t)P.wg_waves - 1) / (uint32_t)P.wg_waves;
    void* args[] = {&Pc, &Ac};
    const uint64_t blocks = (uint64_t)A.n_frames * (uint64_t)A.res_y * Ac.row_groups;      // at most the pixel count
    return hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(64u * (unsigned)P.wg_waves), args, shmem, stream);
}

}  // namespace p3d
