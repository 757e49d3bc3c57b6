// p3d_scene_view.h -- what every ray kernel does before it walks: the scene view of its launch (the blob where it lies, or
// an LDS copy of it), its wave's traversal stack behind that copy, and the register budget attribute.  Shared by the kernel
// files that walk the scene (p3d_kernels.hip, ao.hip, indirect.hip).
#ifndef P3D_SCENE_VIEW_H
#define P3D_SCENE_VIEW_H

#include "p3d_device_types.h"
#include "p3d_shade.h"

namespace p3d {

__device__ __forceinline__ SceneOffsets scene_offsets(const LaunchParams& P) {
    return SceneOffsets{P.off_nodes, P.off_leaves, P.off_spheres, P.off_sphere_meta, P.off_tris, P.off_tri_normals, P.off_boxes, P.off_mats, P.tri_quads};
}

// Scene view of this launch.  LDS variant: the workgroup first copies the blob into LDS (all
// threads, then one barrier -- the only barrier of the launch; call before any early exit).
template <bool LDS> struct View;
template <> struct View<false> {
    typedef GlobalScene type;
    static __device__ __forceinline__ GlobalScene make(const LaunchParams& P) {
        GlobalScene g; g.q = reinterpret_cast<const float4*>(P.blob);
        g.o = scene_offsets(P);
        g.qn = reinterpret_cast<const uint4*>(P.qnodes);
        for (int a = 0; a < 3; a++) { g.qs[a] = P.q_scale[a]; g.qb[a] = P.q_base[a]; }
        return g;
    }
    static __device__ __forceinline__ GlobalScene make_shading(const LaunchParams& P) { return make(P); }
    static __device__ __forceinline__ uint32_t scene_dwords(const LaunchParams&) { return 0; }
};
template <> struct View<true> {
    typedef LdsScene type;
    static __device__ __forceinline__ LdsScene make(const LaunchParams& P) {
        const float4* src = reinterpret_cast<const float4*>(P.blob);
        float4* dst = reinterpret_cast<float4*>(p3d_lds);
        for (uint32_t i = threadIdx.x; i < P.blob_quads; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
        LdsScene l;
        l.o = scene_offsets(P);
        return l;
    }
    static __device__ __forceinline__ LdsScene make_shading(const LaunchParams& P) { return make(P); }
    static __device__ __forceinline__ uint32_t scene_dwords(const LaunchParams& P) { return P.blob_quads * 4; }
};

// this wave's traversal stack: after the (optional) scene copy, one region per wave
template <bool LDS>
__device__ __forceinline__ TravCtx wave_stack(const LaunchParams& P, uint32_t extra_dwords_per_wave, uint32_t** wave_base = nullptr) {
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t* base = p3d_lds + View<LDS>::scene_dwords(P) + wave * (P.trav_stack_dwords + extra_dwords_per_wave);
    if (wave_base) *wave_base = base;
    TravCtx tc;
    tc.lane.region = base; tc.lane.lane = threadIdx.x & 63; tc.lane.slots = P.trav_stack_entries; tc.lane.walk_all = false;
    tc.wave.base = reinterpret_cast<int32_t*>(base);     // the two walks never run in the same launch
    tc.share = base + P.trav_stack_dwords - kShareDwords; // work-sharing walk: the last kShareDwords of the wave's region (host: p3d_render)
    return tc;
}

// OCC = requested waves per SIMD (amdgpu_waves_per_eu): see wf_primary_kernel of p3d_kernels.hip
#ifndef P3D_OCC_FLOOR
#define P3D_OCC_FLOOR 1          // build-time experiment knob: minimum waves per SIMD of every ray kernel
#endif
#define P3D_OCC(OCC) __attribute__((amdgpu_waves_per_eu(((OCC) > P3D_OCC_FLOOR ? (OCC) : P3D_OCC_FLOOR), 8)))

}  // namespace p3d
#endif
