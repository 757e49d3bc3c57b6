// accumulate.hip -- p3d_accumulate: temporal reprojection of history over the AOV planes of a sequence.  A pixel's primary
// hit (the pinhole ray through its centre, times its depth) is projected into the previous frame's camera; the four pixels
// around that point which show the same surface (depth, normal, hit id) give the accumulated colour and its history length
// by bilinear weights, and the current colour is blended in with weight 1 / length.  IEEE basic operations only, in one
// fixed order (DESIGN "Temporal accumulation") -- so the device, the host restatement (host/accumulate_host.cpp) and the
// NumPy one (tests/accumulate_reference.py) agree in every bit.  Built with the ray kernels' flags (-ffp-contract=off,
// correctly rounded division and square root).
//   One launch per frame of the sequence, in stream order: frame f reads what the launch of frame f - 1 wrote.  One thread
//   per pixel; a workgroup of 256 threads owns a tile of kTileW x kTileH pixels.  The taps are read where they lie, through
//   L2 (profiles/denoise_cost.txt: staging does not pay once taps scatter); under a smooth camera motion the taps of
//   neighbouring pixels are neighbours.  The tile is 64 x 4: a wave is ONE row of 64 pixels, so its own 12-byte pixels and,
//   mostly, its taps are contiguous runs of 768 bytes.  Compact 2-D footprints were tried and lost: 32 x 8 (a wave 32 x 2)
//   is 1 % slower, 16 x 16 (16 x 4) 8 %, 8 x 32 (8 x 8) 37 % -- their rows are fragments of cache lines, and the four taps of
//   a pixel overlap those of its row neighbours whatever the tile (profiles/accumulate_cost.txt).  Workgroups are numbered
//   so that each XCD (workgroup index mod 8) runs a contiguous range of tiles.
//   Both cameras travel in the launch arguments: no camera buffer exists on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

#include "accumulate.h"
#include "accumulate_device.h"
#include "p3d_device_math.h"
#include "p3d_pinhole.h"

namespace p3d {

namespace {

// One pixel with a frame to look back at: DESIGN "Temporal accumulation", operation by operation.  false: no history.
__device__ __forceinline__ bool reproject(const AccumulateFrame& F, int32_t x, int32_t y, size_t pixel, V3 C, float Z, V3& out, float& len) {
    if (!valid_depth(Z)) return false;
    // 1. the ray of the frame kernels and the point it reaches (p3d_pinhole.h)
    const V3 d = pinhole_dir(F.uw, F.vh, F.vz, x, y, F.res_x, F.res_y);
    const V3 P = pinhole_point(F.eye, d, Z);
    // 2. to 4. its hit seen through the previous camera, the taps and the blend (accumulate_device.h)
    return reproject_point<false>(F, pixel, C, P, out, len, nullptr);
}

template <bool HISTORY>
__global__ void __launch_bounds__(kThreads) accumulate_kernel(AccumulateFrame F) {
    const uint32_t blk = logical_block(), tile_x = blk % (uint32_t)F.tiles_x, tile_y = blk / (uint32_t)F.tiles_x;
    const int64_t x = (int64_t)tile_x * kTileW + (int)threadIdx.x % kTileW, y = (int64_t)tile_y * kTileH + (int)threadIdx.x / kTileW;
    if (x >= F.res_x || y >= F.res_y) return;
    const size_t pixel = (size_t)y * (size_t)F.res_x + (size_t)x;
    const float* cp = F.color + 3 * pixel;
    const V3 C = mk(cp[0], cp[1], cp[2]);            // read before anything is written: out_color may be color
    V3 out = C;
    float len = 1.0f;
    if (HISTORY) {
        V3 o; float l;
        if (reproject(F, (int32_t)x, (int32_t)y, pixel, C, F.depth[pixel], o, l)) { out = o; len = l; }
    }
    if (F.out_color) { float* o = F.out_color + 3 * pixel; o[0] = out.x; o[1] = out.y; o[2] = out.z; }
    if (F.out_length) F.out_length[pixel] = len;
}

}  // namespace

int accumulate_check_request(const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                             const p3d_accumulate_history* history, const p3d_accumulate_outputs* out, const char** why) {
    *why = "";
    if (!params || !frames || !out) { *why = "params / frames / out is NULL"; return P3D_ERR_ARG; }
    return accumulate_check_planes(params, frames, history, out->rgb32f, out->length, nullptr, out->memory, false, why);
}

int accumulate_check_planes(const p3d_accumulate_params* params, const p3d_accumulate_frames* frames, const p3d_accumulate_history* history,
                            const float* out_rgb32f, const float* out_length, const float* out_prev_xy, int32_t out_memory, bool moving, const char** why) {
    if (!frames->rgb32f || !frames->depth || !frames->normal) { *why = "the frames need rgb32f, depth and normal"; return P3D_ERR_ARG; }
    if (!frames->cams) { *why = "p3d_accumulate_frames::cams is NULL: every frame needs its camera"; return P3D_ERR_ARG; }
    if (history && (!history->rgb32f || !history->depth || !history->normal || !history->length)) {
        *why = "a history needs rgb32f, depth, normal and length (pass a NULL history for none)"; return P3D_ERR_ARG;
    }
    if (history && !history->cam) { *why = "p3d_accumulate_history::cam is NULL: the history needs the camera it was seen through"; return P3D_ERR_ARG; }
    if (!out_rgb32f && !out_length && !out_prev_xy) { *why = moving ? "every output plane is NULL" : "both output planes are NULL"; return P3D_ERR_ARG; }
    if (frames->memory != 0 && frames->memory != 1) { *why = "p3d_accumulate_frames::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (history && history->memory != 0 && history->memory != 1) { *why = "p3d_accumulate_history::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (out_memory != 0 && out_memory != 1) { *why = moving ? "p3d_accumulate_moving_outputs::memory must be 0 (host) or 1 (device)" : "p3d_accumulate_outputs::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    const p3d_accumulate_params& p = *params;
    if (p.res_x < 1 || p.res_y < 1 || p.n_frames < 1) { *why = "res_x, res_y and n_frames must be at least 1"; return P3D_ERR_ARG; }
    if (!std::isfinite(p.depth_tolerance) || !(p.depth_tolerance > 0.0f)) { *why = "depth_tolerance must be finite and positive"; return P3D_ERR_ARG; }
    if (!(p.normal_min >= -1.0f && p.normal_min <= 1.0f)) { *why = "normal_min must be in [-1, 1]"; return P3D_ERR_ARG; }
    if (!std::isfinite(p.max_history) || !(p.max_history >= 1.0f)) { *why = "max_history must be finite and at least 1"; return P3D_ERR_ARG; }
    // 64-bit products of 31-bit factors, compared step by step so that none of them wraps
    const uint64_t limit = 0x7FFFFFFFull, pixels = (uint64_t)p.res_x * (uint64_t)p.res_y;
    if (pixels > limit || pixels * (uint64_t)p.n_frames > limit) { *why = "n_frames * res_x * res_y does not fit 31 bits"; return P3D_ERR_LIMIT; }
    for (int f = 0; f < p.n_frames; f++)
        if (frames->cams[f].res_x != p.res_x || frames->cams[f].res_y != p.res_y) { *why = "a camera of the frames has another res_x / res_y than the params"; return P3D_ERR_ARG; }
    if (history && (history->cam->res_x != p.res_x || history->cam->res_y != p.res_y)) { *why = "the history's camera has another res_x / res_y than the params"; return P3D_ERR_ARG; }
    // aliasing: out->rgb32f may be frames->rgb32f (colour onto colour); no other output plane may be anything the launches read
    const void* const outs[3] = {out_rgb32f, out_length, out_prev_xy};
    for (int i = 0; i < 3; i++) {
        const void* o = outs[i];
        if (!o) continue;
        if (o == frames->depth || o == frames->normal || o == frames->hit_id) { *why = "an output plane is the frames' depth, normal or hit_id"; return P3D_ERR_ARG; }
        if (history && (o == history->rgb32f || o == history->depth || o == history->normal || o == history->length || o == history->hit_id)) {
            *why = "an output plane is a plane of the history: the launches read it while they write"; return P3D_ERR_ARG;
        }
        if (i > 0 && o == (const void*)frames->rgb32f) { *why = moving ? "out->length or out->prev_xy is the frames' rgb32f" : "out->length is the frames' rgb32f"; return P3D_ERR_ARG; }
        for (int j = 0; j < i; j++)
            if (o == outs[j]) { *why = moving ? "two output planes are one plane" : "out->rgb32f and out->length are one plane"; return P3D_ERR_ARG; }
    }
    return P3D_OK;
}

hipError_t launch_accumulate(const p3d_accumulate_params& p, const AccumulatePlanes& A, const p3d_camera* cams,
                             const p3d_camera* hist_cam, hipStream_t stream) {
    AccumulateFrame F;
    const uint32_t blocks = first_frame_record(F, p);
    for (size_t f = 0; f < (size_t)p.n_frames; f++) {
        if (next_frame_record(F, p, A, cams, hist_cam, f)) hipLaunchKernelGGL(accumulate_kernel<true>, dim3(blocks), dim3(kThreads), 0, stream, F);
        else hipLaunchKernelGGL(accumulate_kernel<false>, dim3(blocks), dim3(kThreads), 0, stream, F);
    }
    return hipGetLastError();
}

}  // namespace p3d
