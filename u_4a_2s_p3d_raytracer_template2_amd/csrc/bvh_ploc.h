// bvh_ploc.h -- the clustering rounds of the device builder 2 (bvh_ploc.hip), called by bvh_device.hip between its leaf
// step and its emit step.
#ifndef P3D_BVH_PLOC_H
#define P3D_BVH_PLOC_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace p3d {

struct Box6 { float lo[3], hi[3]; };

constexpr int kPlocRadius = 8;           // R: a cluster looks at the R slots on either side of its own
constexpr int kPlocMaxRounds = 95;       // more rounds than this and the build is abandoned (the caller builds the LBVH)

// Bytes of scratch ploc_cluster() needs for n_leaves leaves.
hipError_t ploc_cluster_scratch_bytes(uint32_t n_leaves, size_t* bytes, hipStream_t stream);

// Clusters the n_leaves >= 2 leaves whose boxes are leaf_box[] (device, sorted order) into a binary tree:
// children[n_leaves - 1] (>= 0 inner node, < 0 leaf ~index; node 0 is the root and every parent has a lower index than its
// children) and node_box[n_leaves - 1], each node's own box.  *d_root_depth (device word) receives the number of inner
// nodes on the longest root-to-leaf path.  Runs on `stream` and WAITS on it once per round (the host reads the number of
// merges back).  *finished == false: more than one cluster was left after kPlocMaxRounds rounds; children / node_box /
// *d_root_depth then hold nothing of use.  `scratch` holds ploc_cluster_scratch_bytes(n_leaves) bytes.
hipError_t ploc_cluster(const Box6* leaf_box, uint32_t n_leaves, int2* children, Box6* node_box, uint32_t* d_root_depth,
                        void* scratch, int* rounds, bool* finished, hipStream_t stream);

}  // namespace p3d
#endif
