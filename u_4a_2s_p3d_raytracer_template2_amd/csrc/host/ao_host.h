// ao_host.h -- the host restatement of p3d_ambient_occlusion's definition (ao_host.cpp): the yardstick of the device kernel.
#ifndef P3D_AO_HOST_H
#define P3D_AO_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "p3d_hip.h"

namespace p3d_host {

// Steps 1 to 6 of the definition for ONE frame of res_y rows of res_x pixels seen through cam (its res_x / res_y are not
// read), the frame-th of a batch: origin_out and dir_out [res_y][res_x][samples][3] hold O and L of every sample (zeros
// where the pixel has no query), valid_out [res_y][res_x] is 1 where it has one.  The caller has checked the ranges.
void ao_segments(const p3d_ao_params& p, const p3d_camera& cam, int32_t frame, int32_t res_x, int32_t res_y, const float* depth,
                 const float* normal, float* origin_out, float* dir_out, uint8_t* valid_out);

// Step 8 for n_pixels pixels: occluded[i] of the samples of pixel i were occluded (0 where it has no query).  rgb32f_in may be
// NULL; ao_out and rgb32f_out may each be NULL.
void ao_resolve(int32_t samples, size_t n_pixels, const int32_t* occluded, const float* rgb32f_in, float* ao_out, float* rgb32f_out);

}  // namespace p3d_host
#endif
