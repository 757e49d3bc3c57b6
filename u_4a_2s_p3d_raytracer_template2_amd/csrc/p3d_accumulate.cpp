// p3d_accumulate.cpp -- p3d_accumulate, p3d_accumulate_moving and p3d_accumulate_variance of include/p3d_hip.h: the
// reprojection of accumulate.hip (through moved primitives; with luminance moments and their variance) over planes in host
// or device memory, enqueued on the scene's stream.
// What the handle keeps for them (p3d_scene::accumulate) is staging and spare planes only: no history, no geometry of an
// earlier frame, and no frame state is read or written.
#include "accumulate.h"
#include "p3d_plane_stage.h"

using namespace p3d;

namespace {

// The three entries: the argument checks, then the staging and the launches.  r.motion NULL: a static world (then
// r.out_prev_xy is NULL too).
int accumulate_on_scene(p3d_scene* s, const AccumulateRequest& r) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    const char* why = "";
    if (const int rc = accumulate_check_request(r, &why)) return fail(rc, why);
    HIP_TRY(hipSetDevice(s->device));
    const p3d_accumulate_params* params = r.params;
    const p3d_accumulate_frames* frames = r.frames;
    const bool var = r.entry == kAccumulateVariance;
    const size_t frame = (size_t)params->res_x * (size_t)params->res_y, pixels = frame * (size_t)params->n_frames;
    const p3d_accumulate_history no_history = {};
    const p3d_accumulate_history& h = r.history ? *r.history : no_history;
    const p3d_accumulate_motion no_motion = {};
    const p3d_accumulate_motion& m = r.motion ? *r.motion : no_motion;
    const bool host_in = frames->memory == 0, host_hist = r.history && h.memory == 0, host_out = r.out_memory == 0, host_motion = r.motion && m.memory == 0;
    const size_t prims = m.n_prims;
    const bool many = params->n_frames > 1;
    p3d_scene::Accumulate& A = s->accumulate;
    typedef PlaneStage::Plane Plane;

    PlaneStage st(s, var ? "p3d_accumulate_variance" : r.motion ? "p3d_accumulate_moving" : "p3d_accumulate", "its spare planes");
    const Plane rgb32f = st.in(A.in_rgb32f, frames->rgb32f, pixels * 12, host_in), depth = st.in(A.in_depth, frames->depth, pixels * 4, host_in),
                normal = st.in(A.in_normal, frames->normal, pixels * 12, host_in), hit_id = st.in(A.in_hit_id, frames->hit_id, pixels * 4, host_in);
    const Plane h_rgb32f = st.in(A.hist_rgb32f, h.rgb32f, frame * 12, host_hist), h_depth = st.in(A.hist_depth, h.depth, frame * 4, host_hist),
                h_normal = st.in(A.hist_normal, h.normal, frame * 12, host_hist), h_length = st.in(A.hist_length, h.length, frame * 4, host_hist),
                h_hit_id = st.in(A.hist_hit_id, h.hit_id, frame * 4, host_hist);
    const Plane m_type = st.in(A.motion_type, m.prim_type, prims * 4, host_motion),
                m_data = st.in(A.motion_data, m.prim_data, prims * 48 * (size_t)params->n_frames, host_motion),
                m_hist = st.in(A.motion_hist, r.history ? m.history_prim_data : nullptr, prims * 48, host_motion);
    const Plane o_rgb32f = st.out(A.out_rgb32f, r.out_rgb32f, pixels * 12, host_out), o_length = st.out(A.out_length, r.out_length, pixels * 4, host_out),
                o_prev_xy = st.out(A.out_prev_xy, r.out_prev_xy, pixels * 8, host_out);
    Plane h_moments, o_moments, o_variance;
    if (!var) {
        if (many && !r.out_rgb32f) st.scratch(A.spare_rgb32f, 2 * frame * 12);      // the next frame reads what the caller does not want
        if (many && !r.out_length) st.scratch(A.spare_length, 2 * frame * 4);
    } else {
        h_moments = st.in(A.hist_moments, r.history_moments, frame * 8, host_hist);
        o_moments = st.out(A.out_moments, r.out_moments, pixels * 8, host_out);
        o_variance = st.out(A.out_variance, r.out_variance, pixels * 4, host_out);
        // in place is a matter of device planes: host colour in and out are staged apart
        const bool detour = !host_in && !host_out && accumulate_variance_colour_detour(*r.variance_params, frames->rgb32f, r.out_rgb32f, r.out_variance);
        const int spare_c = accumulate_variance_spare_colour_frames(*params, r.out_rgb32f, detour);
        const int spare_l = accumulate_variance_spare_length_frames(*params, *r.variance_params, r.out_length, r.out_variance);
        if (spare_c) st.scratch(A.spare_rgb32f, spare_c * frame * 12);
        if (spare_l) st.scratch(A.spare_length, spare_l * frame * 4);
        if (many && !r.out_moments) st.scratch(A.spare_moments, 2 * frame * 8);
    }
    if (const int rc = st.refuse_in_capture()) return rc;
    if (const int rc = st.allocate()) return rc;

    if (const int rc = st.upload()) return rc;
    const AccumulatePlanes P = {rgb32f, depth, normal, hit_id, h_rgb32f, h_depth, h_normal, h_length, h_hit_id, o_rgb32f, o_length,
                                (float*)A.spare_rgb32f.p, (float*)A.spare_length.p};
    const AccumulateMotion M = {m.n_prims, m_type, m_data, m_hist, o_prev_xy};
    AccumulateVariance V = {};
    if (var) V = {*r.variance_params, {h_moments, o_moments, o_variance, (float*)A.spare_moments.p}};
    HIP_TRY(launch_accumulate(*params, P, r.motion ? &M : nullptr, var ? &V : nullptr, frames->cams, h.cam, s->stream));
    return st.finish();
}

}  // namespace

extern "C" int p3d_accumulate(p3d_scene* s, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                              const p3d_accumulate_history* history, const p3d_accumulate_outputs* out) {
    return accumulate_on_scene(s, accumulate_request(params, frames, history, out));
}

extern "C" int p3d_accumulate_moving(p3d_scene* s, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                                     const p3d_accumulate_history* history, const p3d_accumulate_motion* motion,
                                     const p3d_accumulate_moving_outputs* out) {
    return accumulate_on_scene(s, accumulate_request(params, frames, history, motion, out));
}

extern "C" int p3d_accumulate_variance(p3d_scene* s, const p3d_accumulate_params* params, const p3d_accumulate_variance_params* variance_params,
                                       const p3d_accumulate_frames* frames, const p3d_accumulate_history* history, const float* history_moments,
                                       const p3d_accumulate_motion* motion, const p3d_accumulate_variance_outputs* out) {
    return accumulate_on_scene(s, accumulate_request(params, variance_params, frames, history, history_moments, motion, out));
}
