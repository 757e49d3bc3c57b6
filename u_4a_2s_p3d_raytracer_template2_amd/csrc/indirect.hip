// indirect.hip -- p3d_indirect_diffuse: one bounce of diffuse indirect light, gathered per pixel in one launch.  A pixel's
// primary hit (the pinhole ray through its centre times its depth, p3d_pinhole.h) is the origin of `samples` cosine-weighted
// rays; each returns what p3d_trace_rays returns for it at max_depth 1 -- find_closest() and the depth >= max_depth return of
// shade_hit() (p3d_shade.h), as wf_rays_kernel calls them: the clamped direct lighting of what it hits, shadow queries
// included, or the background -- and the pixel's indirect light is their mean.  The rays are p3d_ambient_occlusion's segments
// at radius 1 (p3d_ao_segment.h) and never exist in memory, and neither do their colours: no queues, no workspace.  The
// definition, operation by operation: include/p3d_hip.h; the host restatement of the sum: host/indirect_host.cpp.
//   Lane mapping: wf_ao_kernel's (ao.hip).  A lane is one (pixel, sample); the S lanes of a pixel are consecutive and a wave
//   covers 64 / S consecutive pixels of one row.  The sum over a pixel's samples is log2 S xor-shuffle steps among its lanes:
//   lanes l and l ^ m add the same two values, so every lane of the group holds the balanced tree's sum in the same bits,
//   and lane 0 of the group -- whose operands are (lower half) + (upper half) at every step -- writes.  No LDS and no atomics
//   for the sum.  The workgroup of a scene served from LDS is 4 such waves of one row; all frames of a call go in ONE
//   launch, workgroup index = (frame, row, group of the row), the frame slowest.
//   One build per scene placement and walk (p3d_kernel_variant.h: Level::IndirectDiffuse).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_ao_segment.h"
#include "p3d_launch.h"
#include "p3d_pinhole.h"
#include "p3d_scene_view.h"

namespace p3d {

namespace {

template <bool LDS, int WALK, int OCC>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void wf_indirect_kernel(const LaunchParams P, const IndirectIO A) {
    using SV = typename View<LDS>::type;
    const SV sv = View<LDS>::make_shading(P);
    // workgroup -> (frame, row, group of the row); all wave-uniform
    const uint32_t group = blockIdx.x % A.row_groups, fy = blockIdx.x / A.row_groups;
    const uint32_t y = fy % (uint32_t)A.res_y, f = fy / (uint32_t)A.res_y;
    const uint32_t lane = threadIdx.x & 63u, wave = group * (LDS ? 4u : 1u) + (threadIdx.x >> 6);
    const uint32_t S = 1u << A.log2_samples;
    // (x < res_x + 64 <= 2^31 + 63: the host keeps n * res_y * res_x * samples below 2^31)
    const uint32_t x = wave * (64u >> A.log2_samples) + (lane >> A.log2_samples);
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
    const bool need = in_row && valid_depth(Z);                  // 1. an invalid depth: no query, indirect = 0
    V3 r = mk(0.0f, 0.0f, 0.0f);
    if (__ballot(need) != 0) {                                   // a wave without a query skips the walk
        const FrameCam& C = A.cams[f];
        // 2. the hit point, 3. the normal facing the eye and the origin
        const V3 d = pinhole_dir(C.uw, C.vh, C.vz, (int32_t)x, (int32_t)y, A.res_x, A.res_y);
        const V3 Pt = pinhole_point(C.eye, d, Z);
        const bool away = (N.x * d.x + N.y * d.y) + N.z * d.z > 0.0f;
        const V3 Ns = away ? mk(-N.x, -N.y, -N.z) : N;
        Ray ray;
        ray.o = mk(Pt.x + Ns.x * A.bias, Pt.y + Ns.y * A.bias, Pt.z + Ns.z * A.bias);
        const uint32_t pk = rng_mix(A.seed + f, y * (uint32_t)A.res_x + x);      // 4.
        ray.d = ao_segment(Ns, pk, lane & (S - 1u), 1.0f, need);                  // 5., 6.: the segment at radius 1
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

using IndirectKernelFn = void (*)(const LaunchParams, const IndirectIO);
template <bool LDS, int WALK> constexpr IndirectKernelFn indirect_kernel() { return wf_indirect_kernel<LDS, WALK, WALK == WALK_GRID ? 1 : kRaysOcc>; }

// the five builds: LDS x {lane, grid}, HBM x {lane, shared, grid}
const void* indirect_kernel_for(const KernelVariant& request) {
    const KernelVariant v = canonical_level(request, Level::IndirectDiffuse);
    IndirectKernelFn fn = nullptr;
    if (v.lds) fn = v.walk == WALK_GRID ? indirect_kernel<true, WALK_GRID>() : v.walk == WALK_LANE ? indirect_kernel<true, WALK_LANE>() : nullptr;
    else fn = v.walk == WALK_GRID ? indirect_kernel<false, WALK_GRID>() : v.walk == WALK_SHARED ? indirect_kernel<false, WALK_SHARED>()
              : v.walk == WALK_LANE ? indirect_kernel<false, WALK_LANE>() : nullptr;
    return reinterpret_cast<const void*>(fn);
}

}  // namespace

// p3d_indirect_diffuse: one workgroup per wg_waves waves of a row, all frames in one launch (A.row_waves and A.row_groups
// are set here).  The launch parameters go with max_depth = 1, whatever the caller's: a sample's ray is a ray of depth 1
// that returns its direct lighting.
hipError_t launch_wf_indirect(const LaunchParams& P, const IndirectIO& A, const KernelVariant& v, hipStream_t stream) {
    const void* fn = indirect_kernel_for(v);
    if (!fn) return hipErrorInvalidDeviceFunction;
    const size_t shmem = wavefront_lds_bytes(P, v.lds);
    hipError_t e = allow_lds(fn, shmem);
    if (e != hipSuccess) return e;
    LaunchParams Pc = P;
    Pc.max_depth = 1;
    IndirectIO Ac = A;
    const uint32_t per_wave = 64u >> A.log2_samples;
    Ac.row_waves = (uint32_t)(((uint64_t)A.res_x + per_wave - 1) / per_wave);
    Ac.row_groups = (Ac.row_waves + (uint32_t)P.wg_waves - 1) / (uint32_t)P.wg_waves;
    void* args[] = {&Pc, &Ac};
    const uint64_t blocks = (uint64_t)A.n_frames * (uint64_t)A.res_y * Ac.row_groups;      // at most the pixel count
    return hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(64u * (unsigned)P.wg_waves), args, shmem, stream);
}

}  // namespace p3d
