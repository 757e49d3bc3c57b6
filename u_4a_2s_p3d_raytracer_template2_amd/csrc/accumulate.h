// accumulate.h -- the temporal accumulation of accumulate.hip: what p3d_accumulate, p3d_accumulate_moving and
// p3d_accumulate_variance (p3d_accumulate.cpp) and their p3d_debug_accumulate* probes (p3d_debug_planes.cpp) check and run.
// Internal: not installed with include/.
#ifndef P3D_ACCUMULATE_H
#define P3D_ACCUMULATE_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "p3d_hip.h"

namespace p3d {

constexpr int kAccumulateVarianceMaxRadius = 3;

// What one of the three entries (or its probe) was asked, in one shape.  history, history_moments and motion may be NULL;
// variance_params, history_moments, out_moments and out_variance belong to p3d_accumulate_variance, motion and out_prev_xy
// to it and to p3d_accumulate_moving, and are NULL for an entry that has none.  has_out: the entry's outputs struct was not
// NULL (its planes and memory field are here by value).
enum AccumulateEntry { kAccumulate, kAccumulateMoving, kAccumulateVariance };
struct AccumulateRequest {
    AccumulateEntry entry;
    const p3d_accumulate_params* params;
    const p3d_accumulate_variance_params* variance_params;
    const p3d_accumulate_frames* frames;
    const p3d_accumulate_history* history;
    const float* history_moments;
    const p3d_accumulate_motion* motion;
    bool has_out;
    float *out_rgb32f, *out_length, *out_prev_xy, *out_moments, *out_variance;
    int32_t out_memory;
};
inline AccumulateRequest accumulate_request(const p3d_accumulate_params* p, const p3d_accumulate_frames* frames, const p3d_accumulate_history* history,
                                            const p3d_accumulate_outputs* out) {
    return {kAccumulate, p, nullptr, frames, history, nullptr, nullptr, out != nullptr, out ? out->rgb32f : nullptr, out ? out->length : nullptr,
            nullptr, nullptr, nullptr, out ? out->memory : 0};
}
inline AccumulateRequest accumulate_request(const p3d_accumulate_params* p, const p3d_accumulate_frames* frames, const p3d_accumulate_history* history,
                                            const p3d_accumulate_motion* motion, const p3d_accumulate_moving_outputs* out) {
    return {kAccumulateMoving, p, nullptr, frames, history, nullptr, motion, out != nullptr, out ? out->rgb32f : nullptr, out ? out->length : nullptr,
            out ? out->prev_xy : nullptr, nullptr, nullptr, out ? out->memory : 0};
}
inline AccumulateRequest accumulate_request(const p3d_accumulate_params* p, const p3d_accumulate_variance_params* vp, const p3d_accumulate_frames* frames,
                                            const p3d_accumulate_history* history, const float* history_moments, const p3d_accumulate_motion* motion,
                                            const p3d_accumulate_variance_outputs* out) {
    return {kAccumulateVariance, p, vp, frames, history, history_moments, motion, out != nullptr, out ? out->rgb32f : nullptr,
            out ? out->length : nullptr, out ? out->prev_xy : nullptr, out ? out->moments : nullptr, out ? out->variance : nullptr,
            out ? out->memory : 0};
}

// Every argument check of the three entries but the scene's: P3D_OK, or the P3D_ERR_ARG / P3D_ERR_LIMIT of include/p3d_hip.h
// with *why set, in the words of the entry that asks.
int accumulate_check_request(const AccumulateRequest& request, const char** why);

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

// DEVICE arrays of a world that moves, beside the planes: the primitives' kinds, the records of every frame
// ([n_frames][n_prims][12]) and of the history's frame ([n_prims][12], read when hist_rgb32f is not NULL), and the optional
// plane of previous positions ([n_frames][res_y][res_x][2]).
struct AccumulateMotion {
    uint32_t n_prims;
    const uint32_t* prim_type;
    const float *prim_data, *hist_prim_data;
    float* out_prev_xy;
};

// DEVICE planes of the luminance moments, beside AccumulatePlanes: the history's moments (one frame of 2 floats per pixel,
// read when hist_rgb32f is not NULL), the two new outputs (n_frames frames each, or NULL) and, when out_moments is NULL and
// n_frames > 1, TWO frames of moments (8 bytes per pixel) used like spare_rgb32f.
struct AccumulateVariancePlanes {
    const float* hist_moments;
    float *out_moments, *out_variance;
    float* spare_moments;
};
struct AccumulateVariance {
    p3d_accumulate_variance_params params;
    AccumulateVariancePlanes planes;
};

// Whether the spatial launches run: somebody wants the variance, and a history length can lie below min_temporal.
inline bool accumulate_variance_spatial(const p3d_accumulate_variance_params& vp, const float* out_variance) {
    return out_variance && vp.min_temporal > 1.0f;
}
// Whether the colour takes a detour through spare_rgb32f: an in-place call whose spatial launch reads the input colour
// after the temporal launch has blended it.
inline bool accumulate_variance_colour_detour(const p3d_accumulate_variance_params& vp, const float* rgb32f, const float* out_rgb32f,
                                              const float* out_variance) {
    return out_rgb32f == rgb32f && accumulate_variance_spatial(vp, out_variance);
}
// Frames (0, 1 or 2) spare_rgb32f and spare_length must hold when launch_accumulate is given a variance: an output the
// caller does not want is kept for the next frame (two frames when n_frames > 1), and so is the colour of a detour and the
// length the spatial launch reads.
inline int accumulate_variance_spare_colour_frames(const p3d_accumulate_params& p, const float* out_rgb32f, bool detour) {
    return p.n_frames > 1 ? (!out_rgb32f || detour ? 2 : 0) : (detour ? 1 : 0);
}
inline int accumulate_variance_spare_length_frames(const p3d_accumulate_params& p, const p3d_accumulate_variance_params& vp, const float* out_length,
                                                   const float* out_variance) {
    if (out_length) return 0;
    return p.n_frames > 1 ? 2 : (accumulate_variance_spatial(vp, out_variance) ? 1 : 0);
}

// The accumulation of DESIGN "Temporal accumulation" enqueued on `stream`: one temporal launch per frame, in stream order,
// the frame's camera and the camera it looks back at in the launch arguments.  cams: HOST, n_frames of them; hist_cam: HOST,
// read when hist_rgb32f is not NULL.  planes.out_rgb32f == planes.rgb32f is allowed.
//   motion NULL: a static world.  Else the history is looked for where each surface point was one frame ago; planes.hit_id
//   is not NULL.
//   variance NULL: colour and length alone.  Else the moments travel with them and, when accumulate_variance_spatial(), the
//   spatial launch follows each temporal one; the caller has sized the spare planes as the functions above say.
// The caller has run accumulate_check_request.
hipError_t launch_accumulate(const p3d_accumulate_params& p, const AccumulatePlanes& planes, const AccumulateMotion* motion,
                             const AccumulateVariance* variance, const p3d_camera* cams, const p3d_camera* hist_cam, hipStream_t stream);

}  // namespace p3d
#endif
