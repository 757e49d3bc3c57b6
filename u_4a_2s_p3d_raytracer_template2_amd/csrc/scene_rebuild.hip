// scene_rebuild.hip -- p3d_scene_rebuild on the device (the "rebuild" half): a scene handle whose
// primitives have moved gets the device builder's tree (bvh_device.hip) over the records it holds, without a host copy of
// the geometry.  Like every tree here it only has to be CONSERVATIVE; the primitive records travel unchanged.
//
// Steps (all on the scene's stream):
//   1. one thread per scene index: a BuildPrim with the padded bounds the refit computes (scene_bounds.h), planes compacted out
//   2. (bvh_device.hip: Morton sort, leaves of two, Karras hierarchy, boxes, node pairs with leaf codes)
//   3. what type_leaves(direct = true) does on the host: exclusive counts per kind over the sorted list are the new indices;
//      a leaf of one kind (triangles or spheres) is named in its reference, the others get a LeafRec
//   4. every record is copied from the old blob to its new index, and prim_map follows
// Nothing here crosses workgroups except through hipcub's scans.  Built with the ray kernels' flags.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "scene_bounds.h"
#include "scene_rebuild.h"

namespace p3d {

namespace {

constexpr unsigned kThreads = 256;
constexpr uint32_t kLeafPrims = 2;          // bvh_device.hip: leaf j holds the sorted primitives 2 j and 2 j + 1

__global__ void rebuild_flag_kernel(const uint32_t* prim_map, uint32_t n_prims, uint32_t* bounded) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_prims) bounded[i] = (prim_map[i] >> kRefKindShift) != 3u ? 1u : 0u;
}

__global__ void rebuild_prims_kernel(SceneRecords S, const uint32_t* pos, BuildPrim* out, uint32_t n_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n_prims) return;
    const uint32_t ref = S.prim_map[i], kind = ref >> kRefKindShift, k = ref & kRefIndexMask;
    if (kind == 3u) return;                                         // planes are tested outside the tree
    const uint32_t at = pos[i];
    if (at >= n_out) return;
    Box b;
    box_clear(b);
    if (kind == 1u) add_tris(b, S, k, 1u); else if (kind == 0u) add_spheres(b, S, k, 1u); else add_boxes(b, S, k, 1u);
    BuildPrim p;
    for (int a = 0; a < 3; a++) { p.lo[a] = b.lo[a]; p.hi[a] = b.hi[a]; }
    p.ref = ref; p.scene_id = i;
    out[at] = p;
}

__global__ void rebuild_kinds_kernel(const uint32_t* refs, uint32_t n, uint32_t* is_tri, uint32_t* is_sph) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t kind = refs[k] >> kRefKindShift;
    is_tri[k] = kind == 1u ? 1u : 0u; is_sph[k] = kind == 0u ? 1u : 0u;
}

// Leaf `leaf` as type_leaves sees it: its three typed runs, and the reference that names it directly (0: it needs a record).
struct LeafForm { LeafRec rec; uint32_t direct; };
__device__ __forceinline__ LeafForm leaf_form(uint32_t leaf, uint32_t n, const uint32_t* is_tri, const uint32_t* is_sph,
                                              const uint32_t* tri_idx, const uint32_t* sph_idx) {
    const uint32_t first = leaf * kLeafPrims, last = min(first + kLeafPrims, n);
    uint32_t nt = 0, ns = 0, nb = 0;
    for (uint32_t k = first; k < last; k++) {
        if (is_tri[k]) nt++; else if (is_sph[k]) ns++; else nb++;
    }
    LeafForm f;
    f.rec.tri_first = tri_idx[first]; f.rec.sph_first = sph_idx[first]; f.rec.box_first = first - tri_idx[first] - sph_idx[first];
    f.rec.counts = nt | (ns << 8) | (nb << 16);
    f.direct = 0u;
    if (nb == 0u && (nt == 0u) != (ns == 0u)) {                     // one run of one type: the reference names it
        const uint32_t run_first = nt ? f.rec.tri_first : f.rec.sph_first, run = nt ? nt : ns;
        if (run_first <= kLeafFirstMask)
            f.direct = 0x80000000u | ((nt ? kLeafTris : kLeafSpheres) << kLeafKindShift) | ((run - 1u) << kLeafCountShift) | run_first;
    }
    return f;
}

__global__ void rebuild_need_kernel(uint32_t n, uint32_t n_leaves, const uint32_t* is_tri, const uint32_t* is_sph,
                                    const uint32_t* tri_idx, const uint32_t* sph_idx, uint32_t* need) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_leaves) return;
    need[j] = leaf_form(j, n, is_tri, is_sph, tri_idx, sph_idx).direct ? 0u : 1u;
}

// One thread per node pair: each leaf is the child of exactly one.
__global__ void rebuild_leaves_kernel(NodePair* nodes, uint32_t n_nodes, uint32_t n, uint32_t n_leaves, const uint32_t* is_tri,
                                      const uint32_t* is_sph, const uint32_t* tri_idx, const uint32_t* sph_idx,
                                      const uint32_t* rec_idx, uint32_t* blob, uint32_t off_leaves) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    for (int c = 0; c < 2; c++) {
        const int32_t child = c ? nodes[i].child1 : nodes[i].child0;
        if (child >= 0) continue;
        const uint32_t leaf = (~(uint32_t)child >> 3) / kLeafPrims;  // the builder's code: ~(first << 3 | count - 1)
        int32_t ref = ~0;                                           // (never: the builder has no absent child) the empty leaf
        if (leaf < n_leaves) {
            const LeafForm f = leaf_form(leaf, n, is_tri, is_sph, tri_idx, sph_idx);
            if (f.direct) ref = (int32_t)f.direct;
            else {
                const uint32_t r = 1u + rec_idx[leaf];              // leaf 0 stays the empty leaf
                uint32_t* L = blob + 4 * (size_t)(off_leaves + r);
                L[0] = f.rec.tri_first; L[1] = f.rec.sph_first; L[2] = f.rec.box_first; L[3] = f.rec.counts;
                ref = ~(int32_t)r;
            }
        }
        if (c) nodes[i].child1 = ref; else nodes[i].child0 = ref;
    }
}

// One thread per sorted position: the record moves to its new index; scene id and material travel with it.
__global__ void rebuild_gather_kernel(SceneRecords S, uint32_t old_off_sphere_meta, uint32_t n, const uint32_t* refs,
                                      const uint32_t* tri_idx, const uint32_t* sph_idx, uint32_t* blob, BlobSections N,
                                      uint32_t* prim_map) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t ref = refs[k], kind = ref >> kRefKindShift, old = ref & kRefIndexMask;
    uint32_t at, scene_id;
    if (kind == 1u) {
        at = tri_idx[k];
        const uint32_t* src = S.blob + 4 * (size_t)(S.off_tris + S.tri_quads * old);
        uint32_t* dst = blob + 4 * (size_t)(N.off_tris + N.tri_quads * at);
        for (uint32_t w = 0; w < 4u * S.tri_quads; w++) dst[w] = src[w];
        const uint32_t* ns = S.blob + 4 * (size_t)(S.off_tri_normals + old);
        uint32_t* nd = blob + 4 * (size_t)(N.off_tri_normals + at);
        for (int w = 0; w < 4; w++) nd[w] = ns[w];
        scene_id = src[3];
    } else if (kind == 0u) {
        at = sph_idx[k];
        const uint32_t* src = S.blob + 4 * (size_t)(S.off_spheres + old);
        uint32_t* dst = blob + 4 * (size_t)(N.off_spheres + at);
        for (int w = 0; w < 4; w++) dst[w] = src[w];
        const uint32_t* ms = S.blob + 4 * (size_t)old_off_sphere_meta + 2 * (size_t)old;      // PrimMeta: scene id, material
        uint32_t* md = blob + 4 * (size_t)N.off_sphere_meta + 2 * (size_t)at;
        md[0] = ms[0]; md[1] = ms[1];
        scene_id = ms[0];
    } else {
        at = k - tri_idx[k] - sph_idx[k];
        const uint32_t* src = S.blob + 4 * (size_t)(S.off_boxes + 2u * old);
        uint32_t* dst = blob + 4 * (size_t)(N.off_boxes + 2u * at);
        for (int w = 0; w < 8; w++) dst[w] = src[w];
        scene_id = src[3];
    }
    if (scene_id < S.n_prims) prim_map[scene_id] = (kind << kRefKindShift) | at;
}

__device__ __forceinline__ float half_area(const float* lo, const float* hi) {
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return dx * dy + dy * dz + dz * dx;
}
// union of a node pair's two child boxes (an absent child has NaN bounds: fminf / fmaxf return the other operand)
__device__ __forceinline__ float pair_area(const float* f) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = fminf(f[a], f[6 + a]); hi[a] = fmaxf(f[3 + a], f[9 + a]); }
    return lo[0] <= hi[0] ? half_area(lo, hi) : 0.0f;
}
__device__ __forceinline__ uint32_t leaf_held(int32_t child, const uint32_t* blob, uint32_t off_leaves) {
    const uint32_t ref = (uint32_t)child, form = (ref >> kLeafKindShift) & 3u;
    if (form == kLeafIndirect) {
        const uint32_t counts = blob[4 * (size_t)(off_leaves + ~ref) + 3];
        return (counts & 255u) + ((counts >> 8) & 255u) + ((counts >> 16) & 255u);
    }
    return (form == kLeafTris || form == kLeafSpheres) ? ((ref >> kLeafCountShift) & 15u) + 1u : 0u;
}

__global__ void tree_cost_kernel(const NodePair* nodes, uint32_t n_nodes, const uint32_t* blob, uint32_t off_leaves,
                                 float cost_traverse, float cost_intersect, float* sah) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float cost = 0.0f;
    if (i < n_nodes) {
        const float root = fmaxf(pair_area(reinterpret_cast<const float*>(nodes)), 1e-30f);
        const float* f = reinterpret_cast<const float*>(nodes + i);
        cost = cost_traverse * pair_area(f) / root;
        for (int c = 0; c < 2; c++) {
            const int32_t child = c ? nodes[i].child1 : nodes[i].child0;
            const float* lo = f + 6 * c;
            if (child >= 0 || !(lo[0] <= lo[3])) continue;
            cost += cost_intersect * (float)leaf_held(child, blob, off_leaves) * half_area(lo, lo + 3) / root;
        }
    }
    for (int off = 32; off > 0; off >>= 1) cost += __shfl_xor(cost, off);
    if ((threadIdx.x & 63) == 0 && cost != 0.0f) atomicAdd(sah, cost);
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

hipError_t exclusive_sum(const RebuildScratch& W, const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t stream) {
    size_t bytes = W.scan_temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(W.scan_temp, bytes, in, out, (int)n, stream);
}

}  // namespace

hipError_t rebuild_scan_temp_bytes(uint32_t n_items, size_t* bytes, hipStream_t stream) {
    *bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n_items, stream);
    if (e == hipSuccess && *bytes == 0) *bytes = 16;
    return e;
}

hipError_t launch_rebuild_prims(const SceneRecords& S, uint32_t n_bounded, const RebuildScratch& W, hipStream_t stream) {
    if (S.n_prims == 0) return hipSuccess;
    hipLaunchKernelGGL(rebuild_flag_kernel, dim3(blocks_for(S.n_prims)), dim3(kThreads), 0, stream, S.prim_map, S.n_prims, W.bounded);
    hipError_t e = exclusive_sum(W, W.bounded, W.pos, S.n_prims, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rebuild_prims_kernel, dim3(blocks_for(S.n_prims)), dim3(kThreads), 0, stream, S, W.pos, W.prims, n_bounded);
    return hipGetLastError();
}

hipError_t launch_rebuild_type(uint32_t n, const RebuildScratch& W, hipStream_t stream) {
    const uint32_t L = (n + kLeafPrims - 1) / kLeafPrims;
    hipLaunchKernelGGL(rebuild_kinds_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, stream, W.refs, n, W.is_tri, W.is_sph);
    hipError_t e = exclusive_sum(W, W.is_tri, W.tri_idx, n, stream);
    if (e == hipSuccess) e = exclusive_sum(W, W.is_sph, W.sph_idx, n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rebuild_need_kernel, dim3(blocks_for(L)), dim3(kThreads), 0, stream, n, L, W.is_tri, W.is_sph, W.tri_idx, W.sph_idx, W.need);
    if ((e = exclusive_sum(W, W.need, W.rec_idx, L, stream)) != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t launch_rebuild_emit(const SceneRecords& old_scene, uint32_t old_off_sphere_meta, uint32_t n, const RebuildScratch& W,
                               NodePair* nodes, uint32_t* blob, const BlobSections& sec, uint32_t* prim_map, hipStream_t stream) {
    const uint32_t L = (n + kLeafPrims - 1) / kLeafPrims;
    hipLaunchKernelGGL(rebuild_leaves_kernel, dim3(blocks_for(L - 1)), dim3(kThreads), 0, stream, nodes, L - 1, n, L, W.is_tri, W.is_sph,
                       W.tri_idx, W.sph_idx, W.rec_idx, blob, sec.off_leaves);
    hipLaunchKernelGGL(rebuild_gather_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, stream, old_scene, old_off_sphere_meta, n, W.refs,
                       W.tri_idx, W.sph_idx, blob, sec, prim_map);
    return hipGetLastError();
}

hipError_t launch_tree_cost(const NodePair* nodes, uint32_t n_nodes, const uint32_t* blob, uint32_t off_leaves,
                            float cost_traverse, float cost_intersect, float* cost, hipStream_t stream) {
    if (n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(tree_cost_kernel, dim3(blocks_for(n_nodes)), dim3(kThreads), 0, stream, nodes, n_nodes, blob, off_leaves,
                       cost_traverse, cost_intersect, cost);
    return hipGetLastError();
}

}  // namespace p3d
