// p3d_denoise.cpp -- p3d_denoise and p3d_denoise_variance of include/p3d_hip.h: the filters of denoise.hip and
// denoise_variance.hip over planes in host or device memory, enqueued on the scene's stream.  What the handle keeps for them
// (p3d_scene::denoise) is scratch and staging only: no frame state is read or written.
#include "denoise.h"
#include "p3d_scene_state.h"

using namespace p3d;

namespace {

// Both entries after their argument checks.  in->variance NULL: p3d_denoise (then out->variance is NULL too); else
// p3d_denoise_variance, whose scratch carries the variance behind the colour.
int denoise_on_scene(p3d_scene* s, const p3d_denoise_params* params, const p3d_denoise_variance_inputs* in, const p3d_denoise_variance_outputs* out) {
    HIP_TRY(hipSetDevice(s->device));
    const bool guided = in->variance != nullptr;
    const size_t pixels = (size_t)params->n_frames * (size_t)params->res_x * (size_t)params->res_y;
    const bool host_in = in->memory == 0, host_out = out->memory == 0;
    const bool in_place = !host_in && !host_out &&
                          (guided ? denoise_variance_in_place(in->rgb32f, in->variance, out->rgb32f, out->variance) : out->rgb32f == in->rgb32f);
    p3d_scene::Denoise& D = s->denoise;

    // everything the call needs of the handle, sized before anything is allocated
    struct Need { RawBuf* buf; size_t bytes; } needs[10];
    int n_needs = 0;
    for (int i = 0; i < denoise_scratch_buffers(params->iterations, in_place); i++) needs[n_needs++] = {&D.scratch[i], pixels * (guided ? 16 : 12)};
    if (host_in) {
        needs[n_needs++] = {&D.in_rgb32f, pixels * 12}; needs[n_needs++] = {&D.in_depth, pixels * 4};
        needs[n_needs++] = {&D.in_normal, pixels * 12}; needs[n_needs++] = {&D.in_albedo, pixels * 12};
        if (guided) needs[n_needs++] = {&D.in_variance, pixels * 4};
    }
    if (host_out && out->rgb32f) needs[n_needs++] = {&D.out_rgb32f, pixels * 12};
    if (host_out && out->rgb8) needs[n_needs++] = {&D.out_rgb8, pixels * 3};
    if (host_out && out->variance) needs[n_needs++] = {&D.out_variance, pixels * 4};
    {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s->stream, &cap);
        if (cap != hipStreamCaptureStatusNone) {
            if (host_in || host_out)
                return fail(P3D_ERR_STATE, guided ? "p3d_denoise_variance copies host planes and waits for them: not while the stream is being captured"
                                                  : "p3d_denoise copies host planes and waits for them: not while the stream is being captured");
            for (int i = 0; i < n_needs; i++)
                if (needs[i].bytes > needs[i].buf->cap)
                    return fail(P3D_ERR_STATE, guided ? "p3d_denoise_variance has to allocate its scratch: make a call of this shape before the capture"
                                                      : "p3d_denoise has to allocate its scratch: make a call of this shape before the capture");
        }
    }
    for (int i = 0; i < n_needs; i++) {
        s->stats.device_bytes -= needs[i].buf->cap;
        const hipError_t e = needs[i].buf->ensure(needs[i].bytes);
        s->stats.device_bytes += needs[i].buf->cap;
        HIP_TRY(e);
    }

    const float *rgb = in->rgb32f, *depth = in->depth, *normal = in->normal, *albedo = in->albedo, *variance = in->variance;
    if (host_in) {
        HIP_TRY(hipMemcpyAsync(D.in_rgb32f.p, in->rgb32f, pixels * 12, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(D.in_depth.p, in->depth, pixels * 4, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(D.in_normal.p, in->normal, pixels * 12, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(D.in_albedo.p, in->albedo, pixels * 12, hipMemcpyHostToDevice, s->stream));
        rgb = (const float*)D.in_rgb32f.p; depth = (const float*)D.in_depth.p;
        normal = (const float*)D.in_normal.p; albedo = (const float*)D.in_albedo.p;
        if (guided) {
            HIP_TRY(hipMemcpyAsync(D.in_variance.p, in->variance, pixels * 4, hipMemcpyHostToDevice, s->stream));
            variance = (const float*)D.in_variance.p;
        }
    }
    float *d_rgb32f = out->rgb32f, *d_variance = out->variance;
    uint8_t* d_rgb8 = out->rgb8;
    if (host_out) {
        if (out->rgb32f) d_rgb32f = (float*)D.out_rgb32f.p;
        if (out->rgb8) d_rgb8 = (uint8_t*)D.out_rgb8.p;
        if (out->variance) d_variance = (float*)D.out_variance.p;
    }
    if (guided)
        HIP_TRY(launch_denoise_variance(*params, rgb, depth, normal, albedo, variance, (float*)D.scratch[0].p, (float*)D.scratch[1].p,
                                        d_rgb32f, d_rgb8, d_variance, s->stream));
    else
        HIP_TRY(launch_denoise(*params, rgb, depth, normal, albedo, (float*)D.scratch[0].p, (float*)D.scratch[1].p, d_rgb32f, d_rgb8, s->stream));
    if (host_out) {
        if (out->rgb32f) HIP_TRY(hipMemcpyAsync(out->rgb32f, d_rgb32f, pixels * 12, hipMemcpyDeviceToHost, s->stream));
        if (out->rgb8) HIP_TRY(hipMemcpyAsync(out->rgb8, d_rgb8, pixels * 3, hipMemcpyDeviceToHost, s->stream));
        if (out->variance) HIP_TRY(hipMemcpyAsync(out->variance, d_variance, pixels * 4, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return P3D_OK;
}

}  // namespace

extern "C" int p3d_denoise(p3d_scene* s, const p3d_denoise_params* params, const p3d_denoise_inputs* in, const p3d_outputs* out) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    const char* why = "";
    if (const int rc = denoise_check_request(params, in, out, &why)) return fail(rc, why);
    const p3d_denoise_variance_inputs planes = {in->rgb32f, in->depth, in->normal, in->albedo, nullptr, in->memory};
    const p3d_denoise_variance_outputs colour = {out->rgb8, out->rgb32f, nullptr, out->memory};
    return denoise_on_scene(s, params, &planes, &colour);
}

extern "C" int p3d_denoise_variance(p3d_scene* s, const p3d_denoise_params* params, const p3d_denoise_variance_inputs* in,
                                    const p3d_denoise_variance_outputs* out) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    const char* why = "";
    if (const int rc = denoise_variance_check_request(params, in, out, &why)) return fail(rc, why);
    return denoise_on_scene(s, params, in, out);
}
