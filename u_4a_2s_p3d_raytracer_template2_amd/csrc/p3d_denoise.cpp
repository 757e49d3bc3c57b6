// p3d_denoise.cpp -- p3d_denoise and p3d_denoise_variance of include/p3d_hip.h: the filters of denoise.hip and
// denoise_variance.hip over planes in host or device memory, enqueued on the scene's stream.  What the handle keeps for them
// (p3d_scene::denoise) is scratch and staging only: no frame state is read or written.
#include "denoise.h"
#include "p3d_plane_stage.h"

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

    PlaneStage st(s, guided ? "p3d_denoise_variance" : "p3d_denoise", "its scratch");
    for (int i = 0; i < denoise_scratch_buffers(params->iterations, in_place); i++) st.scratch(D.scratch[i], pixels * (guided ? 16 : 12));
    const PlaneStage::Plane rgb = st.in(D.in_rgb32f, in->rgb32f, pixels * 12, host_in), depth = st.in(D.in_depth, in->depth, pixels * 4, host_in),
                            normal = st.in(D.in_normal, in->normal, pixels * 12, host_in), albedo = st.in(D.in_albedo, in->albedo, pixels * 12, host_in),
                            variance = st.in(D.in_variance, in->variance, pixels * 4, host_in);
    const PlaneStage::Plane o_rgb32f = st.out(D.out_rgb32f, out->rgb32f, pixels * 12, host_out), o_rgb8 = st.out(D.out_rgb8, out->rgb8, pixels * 3, host_out),
                            o_variance = st.out(D.out_variance, out->variance, pixels * 4, host_out);
    if (const int rc = st.refuse_in_capture()) return rc;
    if (const int rc = st.allocate()) return rc;

    if (const int rc = st.upload()) return rc;
    float *const scratch0 = (float*)D.scratch[0].p, *const scratch1 = (float*)D.scratch[1].p;
    if (guided) HIP_TRY(launch_denoise_variance(*params, rgb, depth, normal, albedo, variance, scratch0, scratch1, o_rgb32f, o_rgb8, o_variance, s->stream));
    else HIP_TRY(launch_denoise(*params, rgb, depth, normal, albedo, scratch0, scratch1, o_rgb32f, o_rgb8, s->stream));
    return st.finish();
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
