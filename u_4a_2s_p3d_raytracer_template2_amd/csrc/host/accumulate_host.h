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

}  // namespace p3d_host
#endif
