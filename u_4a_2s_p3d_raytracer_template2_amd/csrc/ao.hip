// ao.hip -- p3d_ambient_occlusion: hemisphere any-hit queries fused per pixel.  A pixel's primary hit (the pinhole ray
// through its centre times its depth, p3d_pinhole.h) is the origin of `samples` cosine-weighted segments of length
// `radius`; each is what p3d_occluded would be asked -- shadow_segment() / light_occluded() of p3d_shade.h, as
// wf_occlusion_kernel calls them -- and the pixel's ambient occlusion is the share that is not occluded.  The segments are
// made in lanes from the depth and normal planes and the counter-based random streams of p3d_shade.h and never exist in
// memory.  The definition, operation by operation: include/p3d_hip.h; the host restatement: host/ao_host.cpp.
//   Lane mapping (p3d_pixel_gather.h): a lane is one (pixel, sample); the S lanes of a pixel are consecutive and a wave covers
//   64 / S consecutive pixels of one row, so a lane group shares its origin and its rays start coherent.  The S lanes of a pixel read the same
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
#include "p3d_pixel_gather.h"

namespace p3d {

namespace {

#ifndef P3D_AO_LANE_PER_PIXEL
#define P3D_AO_LANE_PER_PIXEL 0          // 1: a lane is a pixel and loops over its samples.  Measured: DESIGN "Ambient occlusion"
#endif
constexpr bool kLanePerPixel = P3D_AO_LANE_PER_PIXEL != 0;

template <bool LDS, int WALK, int OCC>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void wf_ao_kernel(const LaunchParams P, const AoIO A) {
    const typename View<LDS>::type sv = View<LDS>::make(P);
    PixelGather g;
    const bool in_row = gather_lane<LDS, kLanePerPixel>(A, g);
    if (__ballot(in_row) == 0) return;                           // past the row's end; no barrier follows the scene copy's
    gather_surface(A, in_row, g);
    const bool need = in_row && valid_depth(g.Z);                // 1. an invalid depth: no query, ao = 1
    const uint32_t lane = g.lane, S = g.S;
    const size_t pixel = g.pixel;
    uint32_t occ = 0;
    if (__ballot(need) != 0) {                                   // a wave without a query skips the walk
        gather_origin(A, g);                                     // 2., 3.
        const V3 Ns = g.Ns;
        V3 O = mk(g.O.x, g.O.y, g.O.z);                          // (formed by mk() as when step 3 stood here: the same selects below)
        if (!need) O = mk(0.0f, 0.0f, 0.0f);                     // lanes without a query stay for the wave-wide walk steps
        const uint32_t pk = gather_key(A, g);                    // 4.
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

template <bool LDS, int WALK> struct AoKernel {
    static const void* fn() { return reinterpret_cast<const void*>(&wf_ao_kernel<LDS, WALK, kGatherOcc<WALK>>); }
};

}  // namespace

// p3d_ambient_occlusion: p3d_pixel_gather.h's launch of wf_ao_kernel
hipError_t launch_wf_ao(const LaunchParams& P, const AoIO& A, const KernelVariant& v, hipStream_t stream) {
    return launch_pixel_gather<AoKernel, Level::AmbientOcclusion>(P, A, v, kLanePerPixel ? 64u : 64u >> A.log2_samples, stream);
}

}  // namespace p3d
