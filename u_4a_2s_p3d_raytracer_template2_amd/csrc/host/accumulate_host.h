// accumulate_host.h -- the host restatement of p3d_accumulate (accumulate_host.cpp): the yardstick of the device kernel.
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

}  // namespace p3d_host
#endif
