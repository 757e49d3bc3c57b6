// p3d_debug_planes.cpp -- the probes of the image-space entries (p3d_debug_denoise*, p3d_debug_upsample,
// p3d_debug_accumulate* of include/p3d_hip.h): the launches of denoise.h, upsample.h and accumulate.h on host planes, on a
// device and without a scene handle.  A plane that is not wanted or not there (or a scratch buffer or spare plane that is not
// needed) is one byte that nothing touches.
#include "accumulate.h"
#include "denoise.h"
#include "p3d_debug_run.h"
#include "upsample.h"

using namespace p3d;

namespace {

// The three accumulate probes: the argument checks, then the 13 planes every request has, the 4 rows of a motion and the 4
// of the moments where the request has them, and launch_accumulate on them.
int debug_accumulate(const char* entry, int device, const AccumulateRequest& r) {
    const char* why = "";
    if (const int rc = accumulate_check_request(r, &why)) return fail(rc, why);
    const p3d_accumulate_params* params = r.params;
    const p3d_accumulate_frames* frames = r.frames;
    const p3d_accumulate_history* history = r.history;
    const p3d_accumulate_motion* motion = r.motion;
    if (frames->memory != 0 || (history && history->memory != 0) || (motion && motion->memory != 0) || r.out_memory != 0)
        return fail(P3D_ERR_ARG, std::string(entry) + " takes host planes: every memory field must be 0");
    const bool var = r.entry == kAccumulateVariance, many = params->n_frames > 1;
    const size_t fr = (size_t)params->res_x * (size_t)params->res_y, px = fr * (size_t)params->n_frames;
    // host planes are staged apart, so no colour is blended in place: no detour
    const size_t spare_c = (size_t)accumulate_variance_spare_colour_frames(*params, r.out_rgb32f, false) * fr * 12;
    const size_t spare_l = (size_t)(var ? accumulate_variance_spare_length_frames(*params, *r.variance_params, r.out_length, r.out_variance)
                                        : many && !r.out_length ? 2 : 0) * fr * 4;
    const p3d_accumulate_history none = {};
    const p3d_accumulate_history& h = history ? *history : none;
    std::vector<DebugArg> a = {{frames->rgb32f, nullptr, px * 12}, {frames->depth, nullptr, px * 4}, {frames->normal, nullptr, px * 12},
                               {frames->hit_id, nullptr, frames->hit_id ? px * 4 : 1},
                               {h.rgb32f, nullptr, history ? fr * 12 : 1}, {h.depth, nullptr, history ? fr * 4 : 1}, {h.normal, nullptr, history ? fr * 12 : 1},
                               {h.length, nullptr, history ? fr * 4 : 1}, {h.hit_id, nullptr, h.hit_id ? fr * 4 : 1},
                               {nullptr, r.out_rgb32f, r.out_rgb32f ? px * 12 : 1}, {nullptr, r.out_length, r.out_length ? px * 4 : 1},
                               {nullptr, nullptr, spare_c ? spare_c : 1}, {nullptr, nullptr, spare_l ? spare_l : 1}};
    const size_t m0 = a.size();
    if (motion) {
        const size_t prims = motion->n_prims;
        a.insert(a.end(), {{motion->prim_type, nullptr, prims * 4}, {motion->prim_data, nullptr, prims * 48 * (size_t)params->n_frames},
                           {history ? motion->history_prim_data : nullptr, nullptr, history ? prims * 48 : 1},
                           {nullptr, r.out_prev_xy, r.out_prev_xy ? px * 8 : 1}});
    }
    const size_t v0 = a.size();
    if (var)
        a.insert(a.end(), {{history ? r.history_moments : nullptr, nullptr, history ? fr * 8 : 1}, {nullptr, r.out_moments, r.out_moments ? px * 8 : 1},
                           {nullptr, r.out_variance, r.out_variance ? px * 4 : 1}, {nullptr, nullptr, many && !r.out_moments ? 2 * fr * 8 : 1}});
    return debug_run(entry, device, a, [&] {
        const AccumulatePlanes P = {a[0].as<float>(), a[1].as<float>(), a[2].as<float>(), frames->hit_id ? a[3].as<int32_t>() : nullptr,
                                    history ? a[4].as<float>() : nullptr, a[5].as<float>(), a[6].as<float>(), a[7].as<float>(),
                                    h.hit_id ? a[8].as<int32_t>() : nullptr,
                                    r.out_rgb32f ? a[9].as<float>() : nullptr, r.out_length ? a[10].as<float>() : nullptr,
                                    a[11].as<float>(), a[12].as<float>()};
        AccumulateMotion M = {};
        if (motion) M = {motion->n_prims, a[m0].as<uint32_t>(), a[m0 + 1].as<float>(), history ? a[m0 + 2].as<float>() : nullptr,
                         r.out_prev_xy ? a[m0 + 3].as<float>() : nullptr};
        AccumulateVariance V = {};
        if (var) V = {*r.variance_params, {history ? a[v0].as<float>() : nullptr, r.out_moments ? a[v0 + 1].as<float>() : nullptr,
                                           r.out_variance ? a[v0 + 2].as<float>() : nullptr, a[v0 + 3].as<float>()}};
        return launch_accumulate(*params, P, motion ? &M : nullptr, var ? &V : nullptr, frames->cams, history ? history->cam : nullptr, nullptr);
    });
}

}  // namespace

extern "C" {

int p3d_debug_denoise(int device, const p3d_denoise_params* params, const p3d_denoise_inputs* in, const p3d_outputs* out) {
    const char* why = "";
    if (const int rc = denoise_check_request(params, in, out, &why)) return fail(rc, why);
    if (in->memory != 0 || out->memory != 0) return fail(P3D_ERR_ARG, "p3d_debug_denoise takes host planes: memory must be 0");
    const size_t px = (size_t)params->n_frames * (size_t)params->res_x * (size_t)params->res_y;
    const int n_scratch = denoise_scratch_buffers(params->iterations, false);
    DebugArg a[8] = {{in->rgb32f, nullptr, px * 12}, {in->depth, nullptr, px * 4}, {in->normal, nullptr, px * 12}, {in->albedo, nullptr, px * 12},
                     {nullptr, nullptr, n_scratch > 0 ? px * 12 : 1}, {nullptr, nullptr, n_scratch > 1 ? px * 12 : 1},
                     {nullptr, out->rgb32f, out->rgb32f ? px * 12 : 1}, {nullptr, out->rgb8, out->rgb8 ? px * 3 : 1}};
    return debug_run("p3d_debug_denoise", device, a, [&] {
        return launch_denoise(*params, a[0].as<float>(), a[1].as<float>(), a[2].as<float>(), a[3].as<float>(), a[4].as<float>(), a[5].as<float>(),
                              out->rgb32f ? a[6].as<float>() : nullptr, out->rgb8 ? a[7].as<uint8_t>() : nullptr, nullptr);
    });
}

int p3d_debug_denoise_variance(int device, const p3d_denoise_params* params, const p3d_denoise_variance_inputs* in,
                               const p3d_denoise_variance_outputs* out) {
    const char* why = "";
    if (const int rc = denoise_variance_check_request(params, in, out, &why)) return fail(rc, why);
    if (in->memory != 0 || out->memory != 0) return fail(P3D_ERR_ARG, "p3d_debug_denoise_variance takes host planes: memory must be 0");
    const size_t px = (size_t)params->n_frames * (size_t)params->res_x * (size_t)params->res_y;
    const int n_scratch = denoise_scratch_buffers(params->iterations, false);
    DebugArg a[10] = {{in->rgb32f, nullptr, px * 12}, {in->depth, nullptr, px * 4}, {in->normal, nullptr, px * 12}, {in->albedo, nullptr, px * 12},
                      {in->variance, nullptr, px * 4},
                      {nullptr, nullptr, n_scratch > 0 ? px * 16 : 1}, {nullptr, nullptr, n_scratch > 1 ? px * 16 : 1},
                      {nullptr, out->rgb32f, out->rgb32f ? px * 12 : 1}, {nullptr, out->rgb8, out->rgb8 ? px * 3 : 1},
                      {nullptr, out->variance, out->variance ? px * 4 : 1}};
    return debug_run("p3d_debug_denoise_variance", device, a, [&] {
        return launch_denoise_variance(*params, a[0].as<float>(), a[1].as<float>(), a[2].as<float>(), a[3].as<float>(), a[4].as<float>(),
                                       a[5].as<float>(), a[6].as<float>(), out->rgb32f ? a[7].as<float>() : nullptr,
                                       out->rgb8 ? a[8].as<uint8_t>() : nullptr, out->variance ? a[9].as<float>() : nullptr, nullptr);
    });
}

int p3d_debug_upsample(int device, const p3d_upsample_params* params, const p3d_upsample_inputs* in, const p3d_upsample_outputs* out) {
    const char* why = "";
    if (const int rc = upsample_check_request(params, in, out, &why)) return fail(rc, why);
    if (in->memory != 0 || out->memory != 0) return fail(P3D_ERR_ARG, "p3d_debug_upsample takes host planes: memory must be 0");
    const size_t low_px = (size_t)params->n_frames * (size_t)params->res_x * (size_t)params->res_y;
    const size_t px = low_px * (size_t)params->factor * (size_t)params->factor, c = (size_t)params->channels;
    DebugArg a[7] = {{in->low, nullptr, low_px * c * 4}, {in->low_depth, nullptr, low_px * 4}, {in->low_normal, nullptr, low_px * 12},
                     {in->depth, nullptr, px * 4}, {in->normal, nullptr, px * 12},
                     {nullptr, out->plane, out->plane ? px * c * 4 : 1}, {nullptr, out->fallback, out->fallback ? px : 1}};
    return debug_run("p3d_debug_upsample", device, a, [&] {
        return launch_upsample(*params, a[0].as<float>(), a[1].as<float>(), a[2].as<float>(), a[3].as<float>(), a[4].as<float>(),
                               out->plane ? a[5].as<float>() : nullptr, out->fallback ? a[6].as<uint8_t>() : nullptr, nullptr);
    });
}

int p3d_debug_accumulate(int device, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                         const p3d_accumulate_history* history, const p3d_accumulate_outputs* out) {
    return debug_accumulate("p3d_debug_accumulate", device, accumulate_request(params, frames, history, out));
}

int p3d_debug_accumulate_moving(int device, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                                const p3d_accumulate_history* history, const p3d_accumulate_motion* motion,
                                const p3d_accumulate_moving_outputs* out) {
    return debug_accumulate("p3d_debug_accumulate_moving", device, accumulate_request(params, frames, history, motion, out));
}

int p3d_debug_accumulate_variance(int device, const p3d_accumulate_params* params, const p3d_accumulate_variance_params* variance_params,
                                  const p3d_accumulate_frames* frames, const p3d_accumulate_history* history, const float* history_moments,
                                  const p3d_accumulate_motion* motion, const p3d_accumulate_variance_outputs* out) {
    return debug_accumulate("p3d_debug_accumulate_variance", device,
                            accumulate_request(params, variance_params, frames, history, history_moments, motion, out));
}

}  // extern "C"
