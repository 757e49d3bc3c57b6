// p3d_launch.h -- what p3d_kernels.hip, p3d_debug_kernels.hip and bvh_device.hip export to the host side (p3d_capi.cpp).
#ifndef P3D_LAUNCH_H
#define P3D_LAUNCH_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bvh_builder.h"
#include "p3d_device_types.h"
#include "p3d_kernel_variant.h"

namespace p3d {

// ---- p3d_kernels.hip
// the build of level kernel k that serves v (p3d_kernel_variant.h: canonical_level)
KernelVariant level_variant(KernelVariant v, Level k);
size_t tree_kernel_lds_bytes(const LaunchParams& P, bool lds);
size_t wavefront_lds_bytes(const LaunchParams& P, bool lds);
size_t tile_kernel_lds_bytes(const LaunchParams& P, bool lds);
hipError_t launch_tree(const LaunchParams& P, const KernelVariant& v, hipStream_t stream);
hipError_t launch_wf_primary(const LaunchParams& P, const KernelVariant& v, hipStream_t stream);
hipError_t launch_wf_rays(const LaunchParams& P, const RayStreamIO& R, const KernelVariant& v, hipStream_t stream);
hipError_t launch_wf_occlusion(const LaunchParams& P, const OcclusionIO& R, const KernelVariant& v, hipStream_t stream);
hipError_t launch_wf_secondary(const LaunchParams& P, const KernelVariant& v, unsigned waves, hipStream_t stream);
hipError_t launch_wf_tile(const LaunchParams& P, const KernelVariant& v, unsigned blocks, hipStream_t stream);
hipError_t wf_resident_waves(const LaunchParams& P, const KernelVariant& v, unsigned* waves);
hipError_t tile_kernel_resident_blocks(const LaunchParams& P, const KernelVariant& v, int* blocks);
// (ray_stream: the builds whose level-1 nodes return to a ray stream's planes instead of a frame's pixels)
hipError_t launch_wf_resolve(const LaunchParams& P, unsigned blocks, bool ray_stream, hipStream_t stream);
hipError_t launch_wf_resolve_fused(const LaunchParams& P, const ResolveLevels& R, unsigned shards, bool ray_stream, hipStream_t stream);
hipError_t launch_clear_words(uint32_t* p, uint32_t n, hipStream_t stream);
// the pre-pass of a frame with a tile coverage mask (p3d_tile_coverage.h: TileCoverageJob): one workgroup per tile row
struct TileCoverageJob;
hipError_t launch_tile_coverage(const TileCoverageJob& J, hipStream_t stream);
hipError_t launch_frame_cams(FrameCam* dst, const FrameCam* cams, int n, hipStream_t stream);
hipError_t launch_raygen_table(float* fx, float* fy, int res_x, int res_y, hipStream_t stream);
hipError_t launch_sum_samples(const LaunchParams& P, size_t first_px, size_t n_px, hipStream_t stream);
hipError_t launch_deinterleave(const void* gathered, void* frames, int res_x, int res_y, int row_block,
                               int world, size_t rank_stride, int bpp, int n_frames, size_t in_stride,
                               size_t out_stride, hipStream_t stream);
bool kernels_have_stamps();
// a launch of fn with more dynamic LDS than the 64 KiB default says so first (remembered per device and kernel)
hipError_t allow_lds(const void* fn, size_t shmem);

// ---- ao.hip
hipError_t launch_wf_ao(const LaunchParams& P, const AoIO& A, const KernelVariant& v, hipStream_t stream);

// ---- indirect.hip
hipError_t launch_wf_indirect(const LaunchParams& P, const IndirectIO& A, const KernelVariant& v, hipStream_t stream);

// ---- indirect_paths.hip
hipError_t launch_wf_indirect_paths(const LaunchParams& P, const PathIO& A, const KernelVariant& v, hipStream_t stream);

// ---- p3d_debug_kernels.hip: unit probes of the device arithmetic (p3d_debug_* of include/p3d_hip.h)
hipError_t launch_debug_check_rcp(uint32_t first, uint64_t count, unsigned long long* n_bad, uint32_t* first_bad, hipStream_t stream);
hipError_t launch_debug_check_rcp_len(uint32_t first, uint64_t count, unsigned long long* n_bad, uint32_t* first_bad, hipStream_t stream);
hipError_t launch_debug_powf(uint32_t n, const float* x, const float* y, float* out, hipStream_t stream);
hipError_t launch_debug_pow(uint32_t n, const double* x, const double* y, double* out, hipStream_t stream);
hipError_t launch_debug_schlick_kr(uint32_t n, const float* ior_1, const float* new_ior, const float* cos_theta_i, float* out,
                                   hipStream_t stream);
hipError_t launch_debug_intersect(uint32_t n, const uint32_t* type, const float* prim12, const float* origin,
                                  const float* dir, int32_t* hit, float* t, float* normal, hipStream_t stream);

// ---- bvh_device.hip
hipError_t build_lbvh_device(const std::vector<BuildPrim>& prims, const BvhOptions& opt, NodePair* d_nodes,
                             uint32_t* d_refs, BvhStats& stats, hipStream_t stream);
// ... the same build over primitives already on the device, for p3d_scene_rebuild: only enqueued.  `scratch` holds
// lbvh_scratch_bytes(n) bytes and lives until the stream has passed; the two words at *d_result (inside it), read back,
// are what lbvh_stats() turns into the tree's statistics.
hipError_t lbvh_scratch_bytes(uint32_t n, size_t* bytes, hipStream_t stream);
hipError_t lbvh_enqueue(const BuildPrim* d_prims, uint32_t n, const BvhOptions& opt, NodePair* d_nodes, uint32_t* d_refs,
                        void* scratch, uint32_t** d_result, hipStream_t stream);
void lbvh_stats(uint32_t n, const uint32_t result[2], BvhStats& stats);
// ... and builder 2 (bvh_ploc.hip between builder 1's leaves and its emit step): the same split, the same two result words.
// ploc_enqueue WAITS on the stream once per clustering round.  fell_back: the rounds did not finish within their bound and
// the tree is builder 1's.
struct PlocInfo { int32_t rounds = 0, fell_back = 0; };
hipError_t ploc_scratch_bytes(uint32_t n, size_t* bytes, hipStream_t stream);
hipError_t ploc_enqueue(const BuildPrim* d_prims, uint32_t n, const BvhOptions& opt, NodePair* d_nodes, uint32_t* d_refs,
                        void* scratch, uint32_t** d_result, PlocInfo* info, hipStream_t stream);
// builder 1 or 2 over host primitives, synchronous (build_lbvh_device is builder 1)
hipError_t build_bvh_device(uint32_t builder, const std::vector<BuildPrim>& prims, const BvhOptions& opt, NodePair* d_nodes,
                            uint32_t* d_refs, BvhStats& stats, PlocInfo* info, hipStream_t stream);
hipError_t sort_tiles_by_cost(const uint32_t* cost, uint32_t* cost_sorted, uint32_t* iota, uint32_t* order, uint32_t n,
                              void* temp, size_t& temp_bytes, hipStream_t stream);

}  // namespace p3d
#endif
