// indirect.hip -- p3d_indirect_diffuse: one bounce of diffuse indirect light, gathered per pixel in one launch.  A pixel's
// primary hit (the pinhole ray through its centre times its depth, p3d_pinhole.h) is the origin of `samples` cosine-weighted
// rays; each returns what p3d_trace_rays returns for it at max_depth 1 -- find_closest() and the depth >= max_depth return of
// shade_hit() (p3d_shade.h), as wf_rays_kernel calls them: the clamped direct lighting of what it hits, shadow queries
// included, or the background -- and the pixel's indirect light is their mean.  The rays are p3d_ambient_occlusion's segments
// at radius 1 (p3d_ao_segment.h) and never exist in memory, and neither do their colours: no queues, no workspace.  The
// definition, operation by operation: include/p3d_hip.h; the host restatement of the sum: host/indirect_host.cpp.
//   Lane mapping: wf_ao_kernel's (p3d_pixel_gather.h).  A lane is one (pixel, sample); the S lanes of a pixel are consecutive and a wave
//   covers 64 / S consecutive pixels of one row.  The sum over a pixel's samples is log2 S xor-shuffle steps among its lanes:
//   lanes l and l ^ m add the same two values, so every lane of the group holds the balanced tree's sum in the same bits,
//   and lane 0 of the group -- whose operands are (lower half) + (upper half) at every step -- writes.  No LDS and no atomics
//   for the sum.  The workgroup of a scene served from LDS is 4 such waves of one row; all frames of a call go in ONE
//   launch, workgroup index = (frame, row, group of the row), the frame slowest.
//   One build per scene placement and walk (p3d_kernel_variant.h: Level::IndirectDiffuse).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_ao_segment.h"
#include "p3d_pixel_gather.h"

namespace p3d {

namespace {

template <bool LDS, int WALK, int OCC>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void wf_indirect_kernel(const LaunchParams P, const IndirectIO A) {
    using SV = typename View<LDS>::type;
    const SV sv = View<LDS>::make_shading(P);
    PixelGather g;
    const bool in_row = gather_lane<LDS, false>(A, g);
    if (__ballot(in_row) == 0) return;                           // past the row's end; no barrier follows the scene copy's
    gather_surface(A, in_row, g);
    const bool need = in_row && valid_depth(g.Z);                // 1. an invalid depth: no query, indirect = 0
    const uint32_t lane = g.lane, S = g.S;
    const size_t pixel = g.pixel;
    V3 r = mk(0.0f, 0.0f, 0.0f);
    if (__ballot(need) != 0) {                                   // a wave without a query skips the walk
        gather_origin(A, g);                                     // 2., 3.
        Ray ray;
        ray.o = g.O;
        const uint32_t pk = gather_key(A, g);                    // 4.
        ray.d = ao_segment(g.Ns, pk, lane & (S - 1u), 1.0f, need);              // 5., 6.: the segment at radius 1
        if (!need) {                                             // lanes without a query stay for the wave-wide walk steps
            ray.o = mk(0.0f, 0.0f, 0.0f); ray.d = mk(1.0f, 0.0f, 0.0f);
        }
        TravCtx tc = wave_stack<LDS>(P, 0);
        Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
        // 7. wf_rays_kernel's steps on Ray(O, D), at the depth where rayTracing() returns its direct lighting (the host
        // passes max_depth = 1: launch_wf_indirect)
        tc.lane.walk_all = !slab_can_cull(ray);                  // its shadow rays too
        const Hit h = find_closest<false, WALK>(P, sv, ray, need, tc, ctr);
        const NodeOut o = shade_hit<false, WALK, SV, false, false>(P, sv, ray, h, need, 1, 1.0f, tc, ctr, 0u);
        if (need) r = o.ret;
    }
    // 8. the balanced tree in sample order, reached by the whole wave: t[i] = t[2 i] + t[2 i + 1], log2 S times
    for (uint32_t m = 1u; m < S; m <<= 1) {
        const float px = __shfl_xor(r.x, (int)m), py = __shfl_xor(r.y, (int)m), pz = __shfl_xor(r.z, (int)m);
        const bool low = (lane & m) == 0u;                       // (lower + upper in both partners: one sum, the same bits)
        r = mk(low ? r.x + px : px + r.x, low ? r.y + py : py + r.y, low ? r.z + pz : pz + r.z);
    }
    // 9. lane 0 of the pixel's group writes
    if (!in_row || (lane & (S - 1u)) != 0u) return;
    const float inv = fdiv(1.0f, (float)S);                      // a power of two: exact
    const V3 m = mk(r.x * inv, r.y * inv, r.z * inv);            // (a pixel without a query: r = 0, m = 0)
    if (A.indirect) { float* o = A.indirect + 3 * pixel; o[0] = m.x; o[1] = m.y; o[2] = m.z; }
    if (A.rgb) {
        V3 a = mk(1.0f, 1.0f, 1.0f), c = mk(0.0f, 0.0f, 0.0f);
        if (A.albedo) { const float* in = A.albedo + 3 * pixel; a = mk(in[0], in[1], in[2]); }
        if (A.color) { const float* in = A.color + 3 * pixel; c = mk(in[0], in[1], in[2]); }
        V3 out = c;                                              // a pixel without a query: c, or 0 without a colour
        if (need) {
            out = mk(a.x * m.x, a.y * m.y, a.z * m.z);
            if (A.color) out = mk(c.x + out.x, c.y + out.y, c.z + out.z);
        }
        float* o = A.rgb + 3 * pixel;
        o[0] = out.x; o[1] = out.y; o[2] = out.z;
    }
}

template <bool LDS, int WALK> struct IndirectKernel {
    static const void* fn() { return reinterpret_cast<const void*>(&wf_indirect_kernel<LDS, WALK, kGatherOcc<WALK>>); }
};

}  // namespace

// p3d_indirect_diffuse: p3d_pixel_gather.h's launch of wf_indirect_kernel.  The launch parameters go with max_depth = 1,
// whatever the caller's: a sample's ray is a ray of depth 1 that returns its direct lighting.
hipError_t launch_wf_indirect(const LaunchParams& P, const IndirectIO& A, const KernelVariant& v, hipStream_t stream) {
    LaunchParams Pc = P;
    Pc.max_depth = 1;
    return launch_pixel_gather<IndirectKernel, Level::IndirectDiffuse>(Pc, A, v, 64u >> A.log2_samples, stream);
}

}  // namespace p3d
