// denoise_host.h -- the host restatements of p3d_denoise and p3d_denoise_variance (denoise_host.cpp): the yardsticks of the
// device kernels.
#ifndef P3D_DENOISE_HOST_H
#define P3D_DENOISE_HOST_H

#include <stdint.h>

#include "p3d_hip.h"

namespace p3d_host {

// p3d_denoise on host planes, every bit: p as the entry reads it (the caller has checked the ranges), planes of n_frames
// frames back to back, bottom row first.  out_rgb32f and out_rgb8 may each be NULL; they must not overlap the inputs.
void denoise(const p3d_denoise_params& p, const float* rgb32f, const float* depth, const float* normal, const float* albedo,
             float* out_rgb32f, uint8_t* out_rgb8);

// p3d_denoise_variance likewise: variance one float per pixel; out_variance may be NULL too.
void denoise_variance(const p3d_denoise_params& p, const float* rgb32f, const float* depth, const float* normal, const float* albedo,
                      const float* variance, float* out_rgb32f, uint8_t* out_rgb8, float* out_variance);

}  // namespace p3d_host
#endif
