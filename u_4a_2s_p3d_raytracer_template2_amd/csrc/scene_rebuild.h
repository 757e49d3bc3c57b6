// scene_rebuild.h -- launchers of scene_rebuild.hip: what p3d_scene_rebuild and p3d_scene_tree_cost (p3d_scene_rebuild.cpp)
// enqueue on the scene's stream.  Internal: not installed with include/.
#ifndef P3D_SCENE_REBUILD_H
#define P3D_SCENE_REBUILD_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "bvh_builder.h"
#include "p3d_device_types.h"
#include "scene_update.h"

namespace p3d {

// Section offsets (in quads) of a scene blob, and the stride of its triangle test records.
struct BlobSections {
    uint32_t off_leaves, off_spheres, off_sphere_meta, off_tris, off_tri_normals, off_boxes, off_mats, tri_quads;
};

// Device scratch of one rebuild of n_prims primitives, n of them bounded, in L = (n + 1) / 2 leaves.  The caller allocates
// it (rebuild_scan_temp_bytes() says how much the scans want) and keeps it until the stream has passed.
struct RebuildScratch {
    uint32_t *bounded, *pos;                       // [n_prims] 1 for a bounded primitive; its place among them
    BuildPrim* prims;                              // [n] what the builder sorts, in scene order
    uint32_t* refs;                                // [n] the builder's sorted reference list (kind << 30 | index in the OLD arrays)
    uint32_t *is_tri, *is_sph, *tri_idx, *sph_idx; // [n] per sorted position: kind flags, and the count of that kind in front of it
    uint32_t *need, *rec_idx;                      // [L] 1 for a leaf that gets a LeafRec; the count of such leaves in front of it
    void* scan_temp; size_t scan_temp_bytes;
};
hipError_t rebuild_scan_temp_bytes(uint32_t n_items, size_t* bytes, hipStream_t stream);

// 1. BuildPrims of the bounded primitives in scene order, planes left out: padded bounds of the records as they are now
//    (scene_bounds.h), ref = prim_map's entry, scene_id = the scene index.
hipError_t launch_rebuild_prims(const SceneRecords& S, uint32_t n_bounded, const RebuildScratch& W, hipStream_t stream);
// 3a. after the build: every primitive's index in its kind's leaf-ordered array (exclusive counts over the sorted list) and
//     which leaves need a record.  The count of records (without the empty leaf 0) is rec_idx[L - 1] + need[L - 1].
hipError_t launch_rebuild_type(uint32_t n, const RebuildScratch& W, hipStream_t stream);
// 3b + 4. the builder's leaf codes in `nodes` become the uploaded leaf references (direct runs or ~LeafRec index), the leaf
//     records are written, every primitive record travels from the old blob to its new index and prim_map gets the new
//     references.  `blob` is zeroed, tables and materials copied, by the caller.
hipError_t launch_rebuild_emit(const SceneRecords& old_scene, uint32_t old_off_sphere_meta, uint32_t n, const RebuildScratch& W,
                               NodePair* nodes, uint32_t* blob, const BlobSections& sec, uint32_t* prim_map, hipStream_t stream);

// SAH cost of the tree in `nodes` (f32 pairs with uploaded leaf references), added to *cost, which the caller has cleared:
// cost_traverse * area(node) + cost_intersect * primitives * area(leaf), over the root's area (bvh_device.hip: lbvh_emit_kernel).
hipError_t launch_tree_cost(const NodePair* nodes, uint32_t n_nodes, const uint32_t* blob, uint32_t off_leaves,
                            float cost_traverse, float cost_intersect, float* cost, hipStream_t stream);

}  // namespace p3d
#endif
