// denoise.h -- the edge-stopping a-trous filter of p3d_denoise (denoise.hip): what p3d_denoise (p3d_denoise.cpp) and the
// p3d_debug_denoise probe run.  Internal: not installed with include/.
#ifndef P3D_DENOISE_H
#define P3D_DENOISE_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "p3d_hip.h"

namespace p3d {

constexpr int kDenoiseMaxIterations = 6;
constexpr int kDenoiseMaxNormalPowerLog2 = 8;

// Every argument check of p3d_denoise but the scene's: P3D_OK, or the P3D_ERR_ARG / P3D_ERR_LIMIT of include/p3d_hip.h
// with *why set.
int denoise_check_request(const p3d_denoise_params* p, const p3d_denoise_inputs* in, const p3d_outputs* out, const char** why);

// Colour scratch buffers (each n_frames * res_x * res_y * 3 floats) launch_denoise needs for `iterations` passes: the
// colour alternates between them and the last pass writes the destination, so a pass never writes what it reads.
// in_place: out_rgb32f == rgb32f, where a single pass would otherwise read its own destination.
inline int denoise_scratch_buffers(int iterations, bool in_place) {
    return iterations >= 3 ? 2 : (iterations == 2 || (iterations == 1 && in_place)) ? 1 : 0;
}

// The filter of DESIGN "Denoising" over DEVICE planes, enqueued on `stream`: one launch per pass, every frame of the
// batch in it; iterations == 0 is one copy-and-quantise launch.  out_rgb32f and out_rgb8 may each be NULL;
// out_rgb32f == rgb32f is allowed.  scratch0 / scratch1: as denoise_scratch_buffers() says (else unused, may be NULL).
// The caller has run denoise_check_request.
hipError_t launch_denoise(const p3d_denoise_params& p, const float* rgb32f, const float* depth, const float* normal,
                          const float* albedo, float* scratch0, float* scratch1, float* out_rgb32f, uint8_t* out_rgb8,
                          hipStream_t stream);

// p3d_denoise_variance (denoise_variance.hip): what p3d_denoise_variance (p3d_denoise.cpp) and the
// p3d_debug_denoise_variance probe run.
// Every argument check of p3d_denoise_variance but the scene's: denoise_check_request's, and the rules of the new planes.
int denoise_variance_check_request(const p3d_denoise_params* p, const p3d_denoise_variance_inputs* in,
                                   const p3d_denoise_variance_outputs* out, const char** why);

// The in_place of denoise_scratch_buffers() for launch_denoise_variance: an output plane is the input plane it filters.
inline bool denoise_variance_in_place(const float* rgb32f, const float* variance, const float* out_rgb32f, const float* out_variance) {
    return out_rgb32f == rgb32f || (out_variance && out_variance == variance);
}

// The variance-guided filter over DEVICE planes, enqueued on `stream`: launch_denoise's launches with the variance plane
// beside the colour.  out_rgb32f, out_rgb8 and out_variance may each be NULL; out_rgb32f == rgb32f and
// out_variance == variance are allowed.  scratch0 / scratch1: as denoise_scratch_buffers() says, each
// n_frames * res_x * res_y * 4 floats (the colour, then the variance).  The caller has run denoise_variance_check_request.
hipError_t launch_denoise_variance(const p3d_denoise_params& p, const float* rgb32f, const float* depth, const float* normal,
                                   const float* albedo, const float* variance, float* scratch0, float* scratch1, float* out_rgb32f,
                                   uint8_t* out_rgb8, float* out_variance, hipStream_t stream);

}  // namespace p3d
#endif
