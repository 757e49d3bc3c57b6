// p3d_accumulate.cpp -- p3d_accumulate and p3d_accumulate_moving of include/p3d_hip.h: the reprojection of accumulate.hip
// (through moved primitives: accumulate_motion.hip) over planes in host or device memory, enqueued on the scene's stream.
// What the handle keeps for them (p3d_scene::accumulate) is staging and spare planes only: no history, no geometry of an
// earlier frame, and no frame state is read or written.
#include "accumulate.h"
#include "p3d_scene_state.h"

using namespace p3d;

namespace {

// Both entries after their argument checks.  motion NULL: p3d_accumulate (then out_prev_xy is NULL too).
int accumulate_on_scene(p3d_scene* s, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                        const p3d_accumulate_history* history, const p3d_accumulate_motion* motion, float* out_rgb32f, float* out_length,
                        float* out_prev_xy, int32_t out_memory) {
    HIP_TRY(hipSetDevice(s->device));
    const size_t frame = (size_t)params->res_x * (size_t)params->res_y, pixels = frame * (size_t)params->n_frames;
    const bool host_in = frames->memory == 0, host_hist = history && history->memory == 0, host_out = out_memory == 0;
    const bool host_motion = motion && motion->memory == 0;
    const size_t prims = motion ? (size_t)motion->n_prims : 0;
    const bool many = params->n_frames > 1;
    p3d_scene::Accumulate& A = s->accumulate;

    // everything the call needs of the handle, sized before anything is allocated
    struct Need { RawBuf* buf; size_t bytes; } needs[17];
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
    if (many && !out_rgb32f) needs[n_needs++] = {&A.spare_rgb32f, 2 * frame * 12};      // the next frame reads what the caller does not want
    if (many && !out_length) needs[n_needs++] = {&A.spare_length, 2 * frame * 4};
    {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s->stream, &cap);
        if (cap != hipStreamCaptureStatusNone) {
            if (host_in || host_hist || host_out || host_motion)
                return fail(P3D_ERR_STATE, motion ? "p3d_accumulate_moving copies host planes and waits for them: not while the stream is being captured"
                                                 : "p3d_accumulate copies host planes and waits for them: not while the stream is being captured");
            for (int i = 0; i < n_needs; i++)
                if (needs[i].bytes > needs[i].buf->cap)
                    return fail(P3D_ERR_STATE, motion ? "p3d_accumulate_moving has to allocate its spare planes: make a call of this shape before the capture"
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
    if (motion) {
        AccumulateMotion M = {motion->n_prims, motion->prim_type, motion->prim_data, history ? motion->history_prim_data : nullptr, d_prev_xy};
        if (host_motion) {
            HIP_TRY(up(A.motion_type, motion->prim_type, prims * 4)); HIP_TRY(up(A.motion_data, motion->prim_data, prims * 48 * (size_t)params->n_frames));
            M.prim_type = (const uint32_t*)A.motion_type.p; M.prim_data = (const float*)A.motion_data.p;
            if (history) { HIP_TRY(up(A.motion_hist, motion->history_prim_data, prims * 48)); M.hist_prim_data = (const float*)A.motion_hist.p; }
        }
        HIP_TRY(launch_accumulate_moving(*params, P, M, frames->cams, history ? history->cam : nullptr, s->stream));
    } else {
        HIP_TRY(launch_accumulate(*params, P, frames->cams, history ? history->cam : nullptr, s->stream));
    }
    if (host_out) {
        if (out_rgb32f) HIP_TRY(hipMemcpyAsync(out_rgb32f, P.out_rgb32f, pixels * 12, hipMemcpyDeviceToHost, s->stream));
        if (out_length) HIP_TRY(hipMemcpyAsync(out_length, P.out_length, pixels * 4, hipMemcpyDeviceToHost, s->stream));
        if (out_prev_xy) HIP_TRY(hipMemcpyAsync(out_prev_xy, d_prev_xy, pixels * 8, hipMemcpyDeviceToHost, s->stream));
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
