// indirect_paths.hip -- p3d_indirect_paths: up to `bounces` bounces of diffuse indirect light, a path per lane, gathered per
// pixel in one launch.  Ray 0 of a path is the ray wf_indirect_kernel (indirect.hip) traces for its sample; at every hit the
// path goes on from the hit point along a cosine-weighted direction (p3d_ao_segment.h at radius 1, keyed by the pixel, the
// bounce and the sample), its throughput multiplied by the albedo of what it hit, and every ray adds what p3d_trace_rays
// returns for it at max_depth 1 -- find_closest() and the depth >= max_depth return of shade_hit() -- times the throughput.
// A path ends on a miss or after `bounces` rays.  Between bounces a path is a throughput, a running sum, a key and a ray,
// all in registers: no ray queues, no workspace.  The definition, operation by operation: include/p3d_hip.h; the host
// restatement of the steps between two rays: host/indirect_paths_host.cpp.
//   Lane mapping, prologue and the final tree: wf_indirect_kernel's (p3d_pixel_gather.h): a lane is one (pixel, sample),
//   the sum over a pixel's samples is log2 S xor-shuffle steps.  No LDS and no atomics for the sum.
//   Control flow: the walk, the shadow queries and ao_segment()'s ballot loop are wave-wide, so the bounce loop is
//   wave-uniform: a lane whose path ended, or that never had one, stays with alive == false and a harmless ray until no
//   lane of the wave is alive or the last bounce is traced.  `bounces` is a launch argument.
//   One build per scene placement and walk (p3d_kernel_variant.h: Level::IndirectPaths).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p3d_ao_segment.h"
#include "p3d_pixel_gather.h"

namespace p3d {

namespace {

constexpr uint32_t kPathBounceKey = 0x80000000u;        // pk_b = rng_mix(pk_0, kPathBounceKey + b): no sample index reaches it

template <bool LDS, int WALK, int OCC>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void wf_indirect_paths_kernel(const LaunchParams P, const PathIO A) {
    using SV = typename View<LDS>::type;
    const SV sv = View<LDS>::make_shading(P);
    PixelGather g;
    const bool in_row = gather_lane<LDS, false>(A, g);
    if (__ballot(in_row) == 0) return;                           // past the row's end; no barrier follows the scene copy's
    gather_surface(A, in_row, g);
    const bool need = in_row && valid_depth(g.Z);                // 1. an invalid depth: no path, indirect = 0
    V3 r = mk(0.0f, 0.0f, 0.0f);                                 // R, the path's sum
    if (__ballot(need) != 0) {                                   // a wave without a path skips the walks
        gather_origin(A, g);                                     // vertex 0: steps 2 to 6 of p3d_indirect_diffuse
        Ray ray;
        ray.o = g.O;
        const uint32_t pk0 = gather_key(A, g);
        const uint32_t s = g.lane & (g.S - 1u);
        ray.d = ao_segment(g.Ns, pk0, s, 1.0f, need);
        V3 T = mk(1.0f, 1.0f, 1.0f);                             // the throughput; read from bounce 1 on, after it was set
        bool alive = need;
        TravCtx tc = wave_stack<LDS>(P, 0);
        Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
        for (int32_t b = 0;;) {                                  // wave-uniform
            if (!alive) {                                        // lanes without a path stay for the wave-wide walk steps
                ray.o = mk(0.0f, 0.0f, 0.0f); ray.d = mk(1.0f, 0.0f, 0.0f);
            }
            // 2. wf_rays_kernel's steps on Ray(O_b, D_b), at the depth where rayTracing() returns its direct lighting (the
            // host passes max_depth = 1: launch_wf_indirect_paths)
            tc.lane.walk_all = !slab_can_cull(ray);              // its shadow rays too
            const Hit h = find_closest<false, WALK>(P, sv, ray, alive, tc, ctr);
            const NodeOut o = shade_hit<false, WALK, SV, false, false>(P, sv, ray, h, alive, 1, 1.0f, tc, ctr, 0u);
            // 3. R = r_0, then R + T_b * r_b
            if (alive) r = b == 0 ? o.ret : mk(r.x + T.x * o.ret.x, r.y + T.y * o.ret.y, r.z + T.z * o.ret.z);
            b++;
            alive = alive && h.ref != 0xFFFFFFFFu && b < A.bounces;          // a miss, or the last ray, ends the path
            if (__ballot(alive) == 0) break;
            // 4. the next vertex
            V3 Ns = mk(0.0f, 0.0f, 1.0f);
            if (alive) {
                const V3 Pt = mk(ray.o.x + ray.d.x * h.t, ray.o.y + ray.d.y * h.t, ray.o.z + ray.d.z * h.t);
                const V3 N = prim_normal(P, sv, h.ref, ray, Pt);                 // what p3d_trace_rays returns as normal
                const V3 a = load_material(sv, h.mat).diff;
                T = b == 1 ? a : mk(T.x * a.x, T.y * a.y, T.z * a.z);
                const bool away = (N.x * ray.d.x + N.y * ray.d.y) + N.z * ray.d.z > 0.0f;
                Ns = away ? mk(-N.x, -N.y, -N.z) : N;
                ray.o = mk(Pt.x + Ns.x * A.bias, Pt.y + Ns.y * A.bias, Pt.z + Ns.z * A.bias);
            }
            ray.d = ao_segment(Ns, rng_mix(pk0, kPathBounceKey + (uint32_t)b), s, 1.0f, alive);
        }
    }
    // 5. steps 8 and 9 of p3d_indirect_diffuse.  The pixel and S are formed again: they were not kept across the walks.
    PixelGather w;
    gather_lane<LDS, false>(A, w);
    const uint32_t lane = w.lane, S = w.S;
    const size_t pixel = ((size_t)w.f * (size_t)A.res_y + w.y) * (size_t)A.res_x + w.x;
    // the balanced tree in sample order, reached by the whole wave: t[i] = t[2 i] + t[2 i + 1], log2 S times
    for (uint32_t m = 1u; m < S; m <<= 1) {
        const float px = __shfl_xor(r.x, (int)m), py = __shfl_xor(r.y, (int)m), pz = __shfl_xor(r.z, (int)m);
        const bool low = (lane & m) == 0u;                       // (lower + upper in both partners: one sum, the same bits)
        r = mk(low ? r.x + px : px + r.x, low ? r.y + py : py + r.y, low ? r.z + pz : pz + r.z);
    }
    // lane 0 of the pixel's group writes
    if (!in_row || (lane & (S - 1u)) != 0u) return;
    const float inv = fdiv(1.0f, (float)S);                      // a power of two: exact
    const V3 m = mk(r.x * inv, r.y * inv, r.z * inv);            // (a pixel without a path: r = 0, m = 0)
    if (A.indirect) { float* o = A.indirect + 3 * pixel; o[0] = m.x; o[1] = m.y; o[2] = m.z; }
    if (A.rgb) {
        V3 a = mk(1.0f, 1.0f, 1.0f), c = mk(0.0f, 0.0f, 0.0f);
        if (A.albedo) { const float* in = A.albedo + 3 * pixel; a = mk(in[0], in[1], in[2]); }
        if (A.color) { const float* in = A.color + 3 * pixel; c = mk(in[0], in[1], in[2]); }
        V3 out = c;                                              // a pixel without a path: c, or 0 without a colour
        if (need) {
            out = mk(a.x * m.x, a.y * m.y, a.z * m.z);
            if (A.color) out = mk(c.x + out.x, c.y + out.y, c.z + out.z);
        }
        float* o = A.rgb + 3 * pixel;
        o[0] = out.x; o[1] = out.y; o[2] = out.z;
    }
}

// The register budget, in waves per SIMD, chosen from what hipcc reports (profiles/indirect_paths_kernel_regs.txt): a path's
// R, T, key and sample live across the walk next to the ray, and at the 6 waves (80 VGPRs) the one-bounce kernel runs at
// the builds spill 4 (LDS), 16 (HBM, per-lane walk) and 30 (HBM, shared walk) VGPRs inside the bounce loop; at 5 waves (96)
// the LDS build spills none and the HBM builds 2 and 5, one more each than their one-bounce siblings at 6.
constexpr int kPathsOcc = 5;
template <int WALK> constexpr int kPathsOccOf = WALK == WALK_GRID ? 1 : kPathsOcc;
template <bool LDS, int WALK> struct PathsKernel {
    static const void* fn() { return reinterpret_cast<const void*>(&wf_indirect_paths_kernel<LDS, WALK, kPathsOccOf<WALK>>); }
};

}  // namespace

// p3d_indirect_paths: p3d_pixel_gather.h's launch of wf_indirect_paths_kernel.  The launch parameters go with max_depth = 1,
// whatever the caller's: every ray of a path is a ray of depth 1 that returns its direct lighting.
hipError_t launch_wf_indirect_paths(const LaunchParams& P, const PathIO& A, const KernelVariant& v, hipStream_t stream) {
    LaunchParams Pc = P;
    Pc.max_depth = 1;
    return launch_pixel_gather<PathsKernel, Level::IndirectPaths>(Pc, A, v, 64u >> A.log2_samples, stream);
}

}  // namespace p3d
