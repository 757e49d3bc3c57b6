// p3d_upsample.cpp -- p3d_upsample of include/p3d_hip.h: its argument checks (upsample_check_request, which the
// p3d_debug_upsample probe shares) and the filter of upsample.hip over planes in host or device memory, enqueued on the
// scene's stream.  What the handle keeps for it (p3d_scene::upsample) is staging only: no frame state is read or written.
#include "upsample.h"

#include <cmath>

#include "denoise.h"
#include "p3d_plane_stage.h"

using namespace p3d;

int p3d::upsample_check_request(const p3d_upsample_params* params, const p3d_upsample_inputs* in, const p3d_upsample_outputs* out, const char** why) {
    *why = "";
    if (!params || !in || !out) { *why = "params / in / out is NULL"; return P3D_ERR_ARG; }
    if (!in->low || !in->low_depth || !in->low_normal || !in->depth || !in->normal) {
        *why = "every input plane is needed: low, low_depth, low_normal, depth, normal"; return P3D_ERR_ARG;
    }
    if (!out->plane && !out->fallback) { *why = "no output plane: plane and fallback are both NULL"; return P3D_ERR_ARG; }
    if (in->memory != 0 && in->memory != 1) { *why = "p3d_upsample_inputs::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (out->memory != 0 && out->memory != 1) { *why = "p3d_upsample_outputs::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    const p3d_upsample_params& p = *params;
    if (p.factor < 1 || p.factor > kUpsampleMaxFactor) { *why = "factor must be 1, 2, 3 or 4"; return P3D_ERR_ARG; }
    if (p.channels != 1 && p.channels != 3) { *why = "channels must be 1 or 3"; return P3D_ERR_ARG; }
    if (p.res_x < 1 || p.res_y < 1 || p.n_frames < 1) { *why = "res_x, res_y and n_frames must be at least 1"; return P3D_ERR_ARG; }
    if (!std::isfinite(p.sigma_depth) || !(p.sigma_depth > 0.0f)) { *why = "sigma_depth must be finite and positive"; return P3D_ERR_ARG; }
    if (p.normal_power_log2 < 0 || p.normal_power_log2 > kDenoiseMaxNormalPowerLog2) { *why = "normal_power_log2 must be in 0..8"; return P3D_ERR_ARG; }
    const void* const ins[5] = {in->low, in->low_depth, in->low_normal, in->depth, in->normal};
    for (const void* q : ins)
        if (q == (const void*)out->plane || q == (const void*)out->fallback) { *why = "an output plane is an input plane"; return P3D_ERR_ARG; }
    // 64-bit products of 31-bit factors, compared step by step so that none of them wraps
    const uint64_t limit = 0x7FFFFFFFull, W = (uint64_t)p.res_x * (uint64_t)p.factor, H = (uint64_t)p.res_y * (uint64_t)p.factor;
    if (W > limit || H > limit || W * H > limit || W * H * (uint64_t)p.n_frames > limit ||
        W * H * (uint64_t)p.n_frames * (uint64_t)p.channels > limit) {
        *why = "n_frames * (res_x * factor) * (res_y * factor) * channels does not fit 31 bits"; return P3D_ERR_LIMIT;
    }
    return P3D_OK;
}

extern "C" int p3d_upsample(p3d_scene* s, const p3d_upsample_params* params, const p3d_upsample_inputs* in, const p3d_upsample_outputs* out) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    const char* why = "";
    if (const int rc = upsample_check_request(params, in, out, &why)) return fail(rc, why);
    HIP_TRY(hipSetDevice(s->device));
    const size_t low_px = (size_t)params->n_frames * (size_t)params->res_x * (size_t)params->res_y;
    const size_t px = low_px * (size_t)params->factor * (size_t)params->factor, c = (size_t)params->channels;
    const bool host_in = in->memory == 0, host_out = out->memory == 0;
    p3d_scene::Upsample& U = s->upsample;

    PlaneStage st(s, "p3d_upsample", "its staging");
    const PlaneStage::Plane low = st.in(U.in_low, in->low, low_px * c * 4, host_in), low_depth = st.in(U.in_low_depth, in->low_depth, low_px * 4, host_in),
                            low_normal = st.in(U.in_low_normal, in->low_normal, low_px * 12, host_in),
                            depth = st.in(U.in_depth, in->depth, px * 4, host_in), normal = st.in(U.in_normal, in->normal, px * 12, host_in);
    const PlaneStage::Plane plane = st.out(U.out_plane, out->plane, px * c * 4, host_out), fallback = st.out(U.out_fallback, out->fallback, px, host_out);
    if (const int rc = st.refuse_in_capture()) return rc;
    if (const int rc = st.allocate()) return rc;

    if (const int rc = st.upload()) return rc;
    HIP_TRY(launch_upsample(*params, low, low_depth, low_normal, depth, normal, plane, fallback, s->stream));
    return st.finish();
}
