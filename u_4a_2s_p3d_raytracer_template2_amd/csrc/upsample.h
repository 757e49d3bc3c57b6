// upsample.h -- the guided upsampler of p3d_upsample (upsample.hip): what p3d_upsample (p3d_upsample.cpp) and the
// p3d_debug_upsample probe run.  Internal: not installed with include/.
#ifndef P3D_UPSAMPLE_H
#define P3D_UPSAMPLE_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "p3d_hip.h"

namespace p3d {

constexpr int kUpsampleMaxFactor = 4;

// Every argument check of p3d_upsample but the scene's: P3D_OK, or the P3D_ERR_ARG / P3D_ERR_LIMIT of include/p3d_hip.h
// with *why set.
int upsample_check_request(const p3d_upsample_params* p, const p3d_upsample_inputs* in, const p3d_upsample_outputs* out, const char** why);

// The filter of DESIGN "Guided upsampling" over DEVICE planes, enqueued on `stream`: one launch, every frame of the batch in
// it.  out_plane and out_fallback may each be NULL (not both).  The caller has run upsample_check_request.
hipError_t launch_upsample(const p3d_upsample_params& p, const float* low, const float* low_depth, const float* low_normal,
                           const float* depth, const float* normal, float* out_plane, uint8_t* out_fallback, hipStream_t stream);

}  // namespace p3d
#endif
