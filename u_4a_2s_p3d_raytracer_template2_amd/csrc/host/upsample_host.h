// upsample_host.h -- the host restatement of p3d_upsample (upsample_host.cpp): the yardstick of the device kernel.
#ifndef P3D_UPSAMPLE_HOST_H
#define P3D_UPSAMPLE_HOST_H

#include <stdint.h>

#include "p3d_hip.h"

namespace p3d_host {

// p3d_upsample on host planes, every bit: p as the entry reads it (the caller has checked the ranges), planes of n_frames
// frames back to back, bottom row first.  out_plane and out_fallback may each be NULL; they must not overlap the inputs.
void upsample(const p3d_upsample_params& p, const float* low, const float* low_depth, const float* low_normal, const float* depth,
              const float* normal, float* out_plane, uint8_t* out_fallback);

}  // namespace p3d_host
#endif
