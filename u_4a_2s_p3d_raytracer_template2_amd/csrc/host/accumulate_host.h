// accumulate_host.h -- the host restatements of p3d_accumulate, p3d_accumulate_moving and p3d_accumulate_variance
// (accumulate_host.cpp): the yardsticks of the device kernels.
#ifndef P3D_ACCUMULATE_HOST_H
#define P3D_ACCUMULATE_HOST_H

#include <stdint.h>

#include "p3d_hip.h"

namespace p3d_host {

// p3d_accumulate on host planes, every bit: p, frames and history as the entry reads them (the caller has checked the
// ranges; the memory fields are not read), history NULL for none.  out_rgb32f and out_length hold n_frames frames and may
// each be NULL; out_rgb32f may be frames.rgb32f, otherwise they must not overlap the inputs.
void accumulate(const p3d_accumulate_params& p, const p3d_accumulate_frames& frames, const p3d_accumulate_history* history,
                float* out_rgb32f, float* out_length);

// p3d_accumulate_moving likewise: motion as the entry reads it (host arrays; the caller has checked it, frames.hit_id is
// not NULL).  out_prev_xy holds n_frames frames of 2 floats per pixel and may be NULL like the other two.
void accumulate_moving(const p3d_accumulate_params& p, const p3d_accumulate_frames& frames, const p3d_accumulate_history* history,
                       const p3d_accumulate_motion& motion, float* out_rgb32f, float* out_length, float* out_prev_xy);

// p3d_accumulate_variance likewise: motion NULL for a static world (then out_prev_xy is not written); history_moments one
// frame of 2 floats per pixel, read when history is not NULL.  out_moments (2 floats per pixel) and out_variance (1) hold
// n_frames frames and may each be NULL like the others.  The spatial estimate reads the frames' colour after the blend has
// been written: here out_rgb32f must NOT be frames.rgb32f.
void accumulate_variance(const p3d_accumulate_params& p, const p3d_accumulate_variance_params& vp, const p3d_accumulate_frames& frames,
                         const p3d_accumulate_history* history, const float* history_moments, const p3d_accumulate_motion* motion,
                         float* out_rgb32f, float* out_length, float* out_moments, float* out_variance, float* out_prev_xy);

}  // namespace p3d_host
#endif
