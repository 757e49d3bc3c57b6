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

}  // namespace p3d
#endif
