// indirect_host.h -- the host restatement of steps 8 and 9 of p3d_indirect_diffuse's definition (indirect_host.cpp): the
// yardstick of the device kernel's sum.  The rays (steps 1 to 6) are ao_segments() at radius 1 (ao_host.h).
#ifndef P3D_INDIRECT_HOST_H
#define P3D_INDIRECT_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "p3d_hip.h"

namespace p3d_host {

// Steps 8 and 9 for n_pixels pixels: radiance [n_pixels][samples][3] holds r_s of every sample, valid[i] is 1 where pixel i
// has a query (the radiances of the others are not read).  albedo and rgb32f_in [n_pixels][3] may each be NULL;
// indirect_out and rgb32f_out [n_pixels][3] may each be NULL.  samples is a power of two, 1 .. 64.
void indirect_resolve(int32_t samples, size_t n_pixels, const float* radiance, const uint8_t* valid, const float* albedo,
                      const float* rgb32f_in, float* indirect_out, float* rgb32f_out);

}  // namespace p3d_host
#endif
