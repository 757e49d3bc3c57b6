// scene_update.h -- launchers of scene_update.hip: what p3d_scene_update (p3d_scene_update.cpp) enqueues on the scene's stream.
// Internal: not installed with include/.
#ifndef P3D_SCENE_UPDATE_H
#define P3D_SCENE_UPDATE_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "p3d_device_types.h"

namespace p3d {

// Where the ray kernels read a scene's primitive records, and the map from scene index to them
// (kind << 30 | index in the kind's leaf-ordered array; planes, kind 3, index their own array).
struct SceneRecords {
    uint32_t*       blob;
    uint32_t        off_leaves, off_spheres, off_tris, off_tri_normals, off_boxes, tri_quads;
    PlaneRec*       planes;
    const uint32_t* prim_map;
    uint32_t        n_prims;
};

// words of the status block a refit leaves behind: the root pair's two boxes (lo3, hi3 each), then the count of
// update entries whose index was out of range
constexpr uint32_t kStatusRootFloats = 12, kStatusBadIndex = 12, kStatusWords = 16;

// One thread per entry: primitive index[i] (nullptr: i) gets the record made of prim12[12 i ..], with flatten_scene's float
// operations.  Entries whose index is >= n_prims are skipped and counted in status[kStatusBadIndex].
// grid_bounds (nullptr: the handle has none yet): [n_prims][6] in scene order, the primitive's GRID-mode box
// (grid_builder.h: grid_box_rule) goes to its row.
hipError_t launch_update_records(const SceneRecords& S, uint32_t n, const uint32_t* index, const float* prim12,
                                 uint32_t* status, float* grid_bounds, hipStream_t stream);
// f32 node pairs of a scene that carries quantised ones only (nodes == nullptr: they exist) and every node's parent,
// from the child references of the quantised nodes.  Boxes are left to the refit.
hipError_t launch_refit_prepare(const QNode* qnodes, uint32_t n_nodes, NodePair* nodes, int32_t* parent, hipStream_t stream);
// Every box of the tree from the primitive records: leaf boxes (padded primitive bounds), then bottom-up unions.
// arrived: one word per node, cleared here.  The root pair's boxes are copied to status[0 .. 11].
hipError_t launch_refit(const SceneRecords& S, NodePair* nodes, const int32_t* parent, uint32_t* arrived, uint32_t n_nodes,
                        uint32_t* status, hipStream_t stream);
// quantise_nodes' coding rule for every node under the given grid
struct QuantGrid { float base[3], scale[3]; };
hipError_t launch_requantise(const NodePair* nodes, QNode* qnodes, uint32_t n_nodes, const QuantGrid& grid, hipStream_t stream);

}  // namespace p3d
#endif
