// p3d_generate_samples.cpp -- p3d_generate_samples of include/p3d_hip.h: the sample array of one frame, made on the
// device (sample_stream.hip) in the bits of the host layer's generate_samples().  Enqueued on the scene's stream; the
// call waits once per pass for the count of completed samples, so it returns with the array complete.
#include "p3d_scene_state.h"
#include "sample_stream.h"

using namespace p3d;

extern "C" int p3d_generate_samples(p3d_scene* s, uint32_t seed, int32_t res_x, int32_t res_y, int32_t spp, float aperture,
                                    float* out, int32_t memory) {
    if (!s || !out) return fail(P3D_ERR_ARG, "scene/out is NULL");
    if (res_x < 1 || res_y < 1 || spp < 1) return fail(P3D_ERR_ARG, "res_x, res_y and spp must be at least 1");
    if (memory != 0 && memory != 1) return fail(P3D_ERR_ARG, "memory must be 0 (host) or 1 (device)");
    // 64-bit products of 31-bit factors: compared step by step so that none of them wraps
    const uint64_t pixels = (uint64_t)res_x * (uint64_t)res_y, per_pixel = (uint64_t)spp * (uint64_t)spp;
    if (pixels > kMaxStackedPixels || per_pixel > kMaxStackedPixels || pixels * per_pixel > kMaxStackedPixels)
        return fail(P3D_ERR_LIMIT, "res_x * res_y * spp * spp does not fit 31 bits");
    HIP_TRY(hipSetDevice(s->device));
    if (stream_capturing(s->stream))
        return fail(P3D_ERR_STATE, "p3d_generate_samples waits on the device for the sample count: not while the stream is being captured");
    const size_t bytes = (size_t)(pixels * per_pixel) * 4 * sizeof(float);
    float* d_out = out;
    if (memory == 0) {       // staged where p3d_render stages a host sample array
        HIP_TRY(s->samples.ensure(bytes));
        d_out = (float*)s->samples.p;
    }
    const size_t held = s->sample_stream.bytes;
    const hipError_t e = generate_sample_stream(s->sample_stream, seed, res_x, res_y, spp, aperture, d_out, 0, nullptr, s->stream);
    s->stats.device_bytes += s->sample_stream.bytes - held;
    HIP_TRY(e);
    if (memory == 0) {
        HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return P3D_OK;
}
