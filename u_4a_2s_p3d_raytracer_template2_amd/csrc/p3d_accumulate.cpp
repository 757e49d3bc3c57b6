// p3d_accumulate.cpp -- p3d_accumulate, p3d_accumulate_moving and p3d_accumulate_variance of include/p3d_hip.h: the
// reprojection of accumulate.hip (through moved primitives: accumulate_motion.hip; with luminance moments and their
// variance: accumulate_variance.hip) over planes in host or device memory, enqueued on the scene's stream.
// What the handle keeps for them (p3d_scene::accumulate) is staging and spare planes only: no history, no geometry of an
// earlier frame, and no frame state is read or written.
#include "accumulate.h"
#include "p3d_scene_state.h"

using namespace p3d;

namespace {

// What p3d_accumulate_variance adds to a request of its siblings.
struct VarianceRequest {
    const p3d_accumulate_variance_params* params;
    const float* history_moments;
    float *out_moments, *out_variance;
};

// The entries after their argument checks.  motion NULL: a static world (then out_prev_xy is NULL too).  var NULL:
// p3d_accumulate / p3d_accumulate_moving; else p3d_accumulate_variance, named `entry` in its refusals.
int accumulate_on_scene(p3d_scene* s, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                        const p3d_accumulate_history* history, const p3d_accumulate_motion* motion, float* out_rgb32f, float* out_length,
                        float* out_prev_xy, int32_t out_memory, const VarianceRequest* var = nullptr) {
    HIP_TRY(hipSetDevice(s->device));
    const size_t frame = (size_t)params->res_x * (size_t)params->res_y, pixels = frame * (size_t)params->n_frames;
    const bool host_in = frames->memory == 0, host_hist = history && history->memory == 0, host_out = out_memory == 0;
    const bool host_motion = motion && motion->memory == 0;
    const size_t prims = motion ? (size_t)motion->n_prims : 0;
    const bool many = params->n_frames > 1;
    p3d_scene::Accumulate& A = s->accumulate;

    // everything the call needs of the handle, sized before anything is allocated
    struct Need { RawBuf* buf; size_t bytes; } needs[21];
    int n_needs = 0;
    if (host_in) {
        needs[n_needs++] = {&A.in_rgb32f, pixels * 12}; needs[n_needs++] = {&A.in_depth, pixels * 4}; needs[n_needs++] = {&A.in_normal, pixels * 12};
        if (frames->hit_id) needs[n_needs++] = {&A.in_hit_id, pixels * 4};
    }
    if (host_hist) {
        needs[n_needs++] = {&A.hist_rgb32f, frame * 12}; needs[n_needs++] = {&A.hist_depth, frame * 4};
        needs[n_needs++] = {&A.hist_normal, frame * 12}; needs[n_needs++] = {&A.hist_length, frame * 4};
        if (history->hit_id) needs[n_needs++] = {&A.hist_hit_id, frame * 4};
    }
    if (host_motion) {
        needs[n_needs++] = {&A.motion_type, prims * 4}; needs[n_needs++] = {&A.motion_data, prims * 48 * (size_t)params->n_frames};
        if (history) needs[n_needs++] = {&A.motion_hist, prims * 48};
    }
    if (host_out && out_rgb32f) needs[n_needs++] = {&A.out_rgb32f, pixels * 12};
    if (host_out && out_length) needs[n_needs++] = {&A.out_length, pixels * 4};
    if (host_out && out_prev_xy) needs[n_needs++] = {&A.out_prev_xy, pixels * 8};
    if (!var) {
        if (many && !out_rgb32f) needs[n_needs++] = {&A.spare_rgb32f, 2 * frame * 12};      // the next frame reads what the caller does not want
        if (many && !out_length) needs[n_needs++] = {&A.spare_length, 2 * frame * 4};
    } else {
        if (host_hist) needs[n_needs++] = {&A.hist_moments, frame * 8};
        if (host_out && var->out_moments) needs[n_needs++] = {&A.out_moments, pixels * 8};
        if (host_out && var->out_variance) needs[n_needs++] = {&A.out_variance, pixels * 4};
        // in place is a matter of device planes: host colour in and out are staged apart
        const bool detour = !host_in && !host_out && accumulate_variance_colour_detour(*var->params, frames->rgb32f, out_rgb32f, var->out_variance);
        const int spare_c = accumulate_variance_spare_colour_frames(*params, out_rgb32f, detour);
        const int spare_l = accumulate_variance_spare_length_frames(*params, *var->params, out_length, var->out_variance);
        if (spare_c) needs[n_needs++] = {&A.spare_rgb32f, spare_c * frame * 12};
        if (spare_l) needs[n_needs++] = {&A.spare_length, spare_l * frame * 4};
        if (many && !var->out_moments) needs[n_needs++] = {&A.spare_moments, 2 * frame * 8};
    }
    {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s->stream, &cap);
        if (cap != hipStreamCaptureStatusNone) {
            if (host_in || host_hist || host_out || host_motion)
                return fail(P3D_ERR_STATE, var ? "p3d_accumulate_variance copies host planes and waits for them: not while the stream is being captured"
                                           : motion ? "p3d_accumulate_moving copies host planes and waits for them: not while the stream is being captured"
                                                    : "p3d_accumulate copies host planes and waits for them: not while the stream is being captured");
            for (int i = 0; i < n_needs; i++)
                if (needs[i].bytes > needs[i].buf->cap)
                    return fail(P3D_ERR_STATE, var ? "p3d_accumulate_variance has to allocate its spare planes: make a call of this shape before the capture"
                                               : motion ? "p3d_accumulate_moving has to allocate its spare planes: make a call of this shape before the capture"
                                                        : "p3d_accumulate has to allocate its spare planes: make a call of this shape before the capture");
        }
    }
    for (int i = 0; i < n_needs; i++) {
        s->stats.device_bytes -= needs[i].buf->cap;
        const hipError_t e = needs[i].buf->ensure(needs[i].bytes);
        s->stats.device_bytes += needs[i].buf->cap;
        HIP_TRY(e);
    }

    AccumulatePlanes P = {frames->rgb32f, frames->depth, frames->normal, frames->hit_id,
                          nullptr, nullptr, nullptr, nullptr, nullptr, out_rgb32f, out_length,
                          (float*)A.spare_rgb32f.p, (float*)A.spare_length.p};
    auto up = [&](RawBuf& b, const void* src, size_t bytes) { return hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s->stream); };
    if (host_in) {
        HIP_TRY(up(A.in_rgb32f, frames->rgb32f, pixels * 12)); HIP_TRY(up(A.in_depth, frames->depth, pixels * 4));
        HIP_TRY(up(A.in_normal, frames->normal, pixels * 12));
        P.rgb32f = (const float*)A.in_rgb32f.p; P.depth = (const float*)A.in_depth.p; P.normal = (const float*)A.in_normal.p;
        if (frames->hit_id) { HIP_TRY(up(A.in_hit_id, frames->hit_id, pixels * 4)); P.hit_id = (const int32_t*)A.in_hit_id.p; }
    }
    if (history) {
        P.hist_rgb32f = history->rgb32f; P.hist_depth = history->depth; P.hist_normal = history->normal;
        P.hist_length = history->length; P.hist_hit_id = history->hit_id;
    }
    if (host_hist) {
        HIP_TRY(up(A.hist_rgb32f, history->rgb32f, frame * 12)); HIP_TRY(up(A.hist_depth, history->depth, frame * 4));
        HIP_TRY(up(A.hist_normal, history->normal, frame * 12)); HIP_TRY(up(A.hist_length, history->length, frame * 4));
        P.hist_rgb32f = (const float*)A.hist_rgb32f.p; P.hist_depth = (const float*)A.hist_depth.p;
        P.hist_normal = (const float*)A.hist_normal.p; P.hist_length = (const float*)A.hist_length.p;
        if (history->hit_id) { HIP_TRY(up(A.hist_hit_id, history->hit_id, frame * 4)); P.hist_hit_id = (const int32_t*)A.hist_hit_id.p; }
    }
    if (host_out) {
        if (out_rgb32f) P.out_rgb32f = (float*)A.out_rgb32f.p;
        if (out_length) P.out_length = (float*)A.out_length.p;
    }
    float* d_prev_xy = out_prev_xy && host_out ? (float*)A.out_prev_xy.p : out_prev_xy;
    AccumulateVariancePlanes VP = {nullptr, nullptr, nullptr, (float*)A.spare_moments.p};
    if (var) {
        VP.hist_moments = var->history_moments; VP.out_moments = var->out_moments; VP.out_variance = var->out_variance;
        if (host_hist) { HIP_TRY(up(A.hist_moments, var->history_moments, frame * 8)); VP.hist_moments = (const float*)A.hist_moments.p; }
        if (host_out && var->out_moments) VP.out_moments = (float*)A.out_moments.p;
        if (host_out && var->out_variance) VP.out_variance = (float*)A.out_variance.p;
    }
    if (motion) {
        AccumulateMotion M = {motion->n_prims, motion->prim_type, motion->prim_data, history ? motion->history_prim_data : nullptr, d_prev_xy};
        if (host_motion) {
            HIP_TRY(up(A.motion_type, motion->prim_type, prims * 4)); HIP_TRY(up(A.motion_data, motion->prim_data, prims * 48 * (size_t)params->n_frames));
            M.prim_type = (const uint32_t*)A.motion_type.p; M.prim_data = (const float*)A.motion_data.p;
            if (history) { HIP_TRY(up(A.motion_hist, motion->history_prim_data, prims * 48)); M.hist_prim_data = (const float*)A.motion_hist.p; }
        }
        if (var) HIP_TRY(launch_accumulate_variance(*params, *var->params, P, VP, &M, frames->cams, history ? history->cam : nullptr, s->stream));
        else HIP_TRY(launch_accumulate_moving(*params, P, M, frames->cams, history ? history->cam : nullptr, s->stream));
    } else if (var) {
        HIP_TRY(launch_accumulate_variance(*params, *var->params, P, VP, nullptr, frames->cams, history ? history->cam : nullptr, s->stream));
    } else {
        HIP_TRY(launch_accumulate(*params, P, frames->cams, history ? history->cam : nullptr, s->stream));
    }
    if (host_out) {
        if (out_rgb32f) HIP_TRY(hipMemcpyAsync(out_rgb32f, P.out_rgb32f, pixels * 12, hipMemcpyDeviceToHost, s->stream));
        if (out_length) HIP_TRY(hipMemcpyAsync(out_length, P.out_length, pixels * 4, hipMemcpyDeviceToHost, s->stream));
        if (out_prev_xy) HIP_TRY(hipMemcpyAsync(out_prev_xy, d_prev_xy, pixels * 8, hipMemcpyDeviceToHost, s->stream));
        if (var && var->out_moments) HIP_TRY(hipMemcpyAsync(var->out_moments, VP.out_moments, pixels * 8, hipMemcpyDeviceToHost, s->stream));
        if (var && var->out_variance) HIP_TRY(hipMemcpyAsync(var->out_variance, VP.out_variance, pixels * 4, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    } else if (host_in || host_hist || host_motion) {
        HIP_TRY(hipStreamSynchronize(s->stream));        // the caller's host planes have been read when the call returns
    }
    return P3D_OK;
}

}  // namespace

extern "C" int p3d_accumulate(p3d_scene* s, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                              const p3d_accumulate_history* history, const p3d_accumulate_outputs* out) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    const char* why = "";
    if (const int rc = accumulate_check_request(params, frames, history, out, &why)) return fail(rc, why);
    return accumulate_on_scene(s, params, frames, history, nullptr, out->rgb32f, out->length, nullptr, out->memory);
}

extern "C" int p3d_accumulate_moving(p3d_scene* s, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                                     const p3d_accumulate_history* history, const p3d_accumulate_motion* motion,
                                     const p3d_accumulate_moving_outputs* out) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    const char* why = "";
    if (const int rc = accumulate_moving_check_request(params, frames, history, motion, out, &why)) return fail(rc, why);
    return accumulate_on_scene(s, params, frames, history, motion, out->rgb32f, out->length, out->prev_xy, out->memory);
}

extern "C" int p3d_accumulate_variance(p3d_scene* s, const p3d_accumulate_params* params, const p3d_accumulate_variance_params* variance_params,
                                       const p3d_accumulate_frames* frames, const p3d_accumulate_history* history, const float* history_moments,
                                       const p3d_accumulate_motion* motion, const p3d_accumulate_variance_outputs* out) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    const char* why = "";
    if (const int rc = accumulate_variance_check_request(params, variance_params, frames, history, history_moments, motion, out, &why)) return fail(rc, why);
    const VarianceRequest var = {variance_params, history_moments, out->moments, out->variance};
    return accumulate_on_scene(s, params, frames, history, motion, out->rgb32f, out->length, out->prev_xy, out->memory, &var);
}
