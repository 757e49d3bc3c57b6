// accumulate.h -- the temporal reprojection of p3d_accumulate (accumulate.hip): what p3d_accumulate (p3d_accumulate.cpp)
// and the p3d_debug_accumulate probe run.  Internal: not installed with include/.
#ifndef P3D_ACCUMULATE_H
#define P3D_ACCUMULATE_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "p3d_hip.h"

namespace p3d {

// Every argument check of p3d_accumulate but the scene's: P3D_OK, or the P3D_ERR_ARG / P3D_ERR_LIMIT of include/p3d_hip.h
// with *why set.  history may be NULL.
int accumulate_check_request(const p3d_accumulate_params* p, const p3d_accumulate_frames* frames,
                             const p3d_accumulate_history* history, const p3d_accumulate_outputs* out, const char** why);

// The checks p3d_accumulate and p3d_accumulate_moving share, given non-NULL params and frames: the three output planes
// (out_prev_xy: p3d_accumulate_moving's, NULL for p3d_accumulate) and the outputs' memory field by value; `moving` chooses
// the wording of the refusals -- p3d_accumulate's are what they were.
int accumulate_check_planes(const p3d_accumulate_params* p, const p3d_accumulate_frames* frames, const p3d_accumulate_history* history,
                            const float* out_rgb32f, const float* out_length, const float* out_prev_xy, int32_t out_memory, bool moving, const char** why);

// Every argument check of p3d_accumulate_moving but the scene's, likewise.
int accumulate_moving_check_request(const p3d_accumulate_params* p, const p3d_accumulate_frames* frames, const p3d_accumulate_history* history,
                                    const p3d_accumulate_motion* motion, const p3d_accumulate_moving_outputs* out, const char** why);

// DEVICE planes of launch_accumulate.  The frames' planes hold n_frames frames back to back, the history's one frame;
// hist_rgb32f == NULL: frame 0 has no history (the other hist_* are then unused).  hit_id and hist_hit_id may be NULL.
// out_rgb32f / out_length: n_frames frames each, or NULL -- then, when n_frames > 1, spare_rgb32f / spare_length must
// hold TWO frames (12 and 4 bytes per pixel): frame f is written to half f & 1, where frame f + 1 reads it.
struct AccumulatePlanes {
    const float *rgb32f, *depth, *normal;
    const int32_t* hit_id;
    const float *hist_rgb32f, *hist_depth, *hist_normal, *hist_length;
    const int32_t* hist_hit_id;
    float *out_rgb32f, *out_length;
    float *spare_rgb32f, *spare_length;
};

// The accumulation of DESIGN "Temporal accumulation" enqueued on `stream`: one launch per frame, in stream order, the
// frame's camera and the camera it looks back at in the launch arguments.  cams: HOST, n_frames of them; hist_cam: HOST,
// read when hist_rgb32f is not NULL.  out_rgb32f == rgb32f is allowed.  The caller has run accumulate_check_request.
hipError_t launch_accumulate(const p3d_accumulate_params& p, const AccumulatePlanes& planes, const p3d_camera* cams,
                             const p3d_camera* hist_cam, hipStream_t stream);

// DEVICE arrays of launch_accumulate_moving beside the planes: the primitives' kinds, the records of every frame
// ([n_frames][n_prims][12]) and of the history's frame ([n_prims][12], read when hist_rgb32f is not NULL), and the optional
// plane of previous positions ([n_frames][res_y][res_x][2]).
struct AccumulateMotion {
    uint32_t n_prims;
    const uint32_t* prim_type;
    const float *prim_data, *hist_prim_data;
    float* out_prev_xy;
};

// p3d_accumulate_moving's launches (accumulate_motion.hip), enqueued as launch_accumulate's are.  planes.hit_id is not NULL.
// The caller has run accumulate_moving_check_request.
hipError_t launch_accumulate_moving(const p3d_accumulate_params& p, const AccumulatePlanes& planes, const AccumulateMotion& motion,
                                    const p3d_camera* cams, const p3d_camera* hist_cam, hipStream_t stream);

}  // namespace p3d
#endif
