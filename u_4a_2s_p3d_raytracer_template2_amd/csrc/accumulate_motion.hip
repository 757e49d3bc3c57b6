// accumulate_motion.hip -- p3d_accumulate_moving: p3d_accumulate's reprojection through primitives that p3d_scene_update
// moved.  The pixel's hit point P on primitive I is mapped to the same surface point of primitive I one frame ago (sphere:
// the same direction from the centre; triangle: the same barycentric coordinates; box: the same fraction of every axis),
// and that point, not P, is projected into the previous camera.  The map is fused into the gather pass: the lane that will
// read the four taps reads its primitive's kind and its two 48-byte records first -- one more dependent load stage, no
// per-pixel motion plane in memory.  Everything from the projected point on is accumulate.hip's code (accumulate_device.h),
// and so are the tile (64 x 4: a wave is one row), the XCD numbering, the launch per frame in stream order and the build
// flags (-ffp-contract=off, correctly rounded division and square root): IEEE basic operations in the order of
// include/p3d_hip.h, which the host restatement (host/accumulate_host.cpp) and tests/accumulate_moving_reference.py repeat.
//   The records are read with three 16-byte loads each.  Pixels of one primitive read the same 100 bytes, so inside a
//   silhouette a wave's lookup is a handful of cache lines; lanes whose depth is not valid (misses) and lanes whose id
//   is outside the primitives read nothing.  profiles/accumulate_moving_cost.txt has the cost against p3d_accumulate.
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

template <bool HISTORY>
__global__ void __launch_bounds__(kThreads) accumulate_moving_kernel(MovingFrame M) {
    const AccumulateFrame& F = M.F;
    const uint32_t blk = logical_block(), tile_x = blk % (uint32_t)F.tiles_x, tile_y = blk / (uint32_t)F.tiles_x;
    const int64_t x = (int64_t)tile_x * kTileW + (int)threadIdx.x % kTileW, y = (int64_t)tile_y * kTileH + (int)threadIdx.x / kTileW;
    if (x >= F.res_x || y >= F.res_y) return;
    const size_t pixel = (size_t)y * (size_t)F.res_x + (size_t)x;
    const float* cp = F.color + 3 * pixel;
    const V3 C = mk(cp[0], cp[1], cp[2]);            // read before anything is written: out_color may be color
    V3 out = C;
    float len = 1.0f;
    float xy[2] = {__uint_as_float(0x7FC00000u), __uint_as_float(0x7FC00000u)};
    if (HISTORY) {
        const float Z = F.depth[pixel];
        if (valid_depth(Z)) {                        // 0.; a miss reads no id and no record
            // 1. the ray of the frame kernels and the point it reaches (p3d_pinhole.h)
            const V3 d = pinhole_dir(F.uw, F.vh, F.vz, (int32_t)x, (int32_t)y, F.res_x, F.res_y);
            const V3 P = pinhole_point(F.eye, d, Z);
            V3 Q, o;
            float l;
            // 2. to 4. from where that surface point was one frame ago
            if (previous_point(M, F.hit[pixel], P, Q) && reproject_point<true>(F, pixel, C, Q, o, l, xy)) { out = o; len = l; }
        }
    }
    if (F.out_color) { float* o = F.out_color + 3 * pixel; o[0] = out.x; o[1] = out.y; o[2] = out.z; }
    if (F.out_length) F.out_length[pixel] = len;
    if (M.out_xy) { Float2A v; v.x = xy[0]; v.y = xy[1]; *(Float2*)(M.out_xy + 2 * pixel) = v; }
}

}  // namespace

int accumulate_moving_check_request(const p3d_accumulate_params* params, const p3d_accumulate_frames* frames, const p3d_accumulate_history* history,
                                    const p3d_accumulate_motion* motion, const p3d_accumulate_moving_outputs* out, const char** why) {
    *why = "";
    if (!params || !frames || !out) { *why = "params / frames / out is NULL"; return P3D_ERR_ARG; }
    if (!motion) { *why = "motion is NULL: p3d_accumulate is the entry for a static world"; return P3D_ERR_ARG; }
    if (!motion->prim_type || !motion->prim_data) { *why = "the motion needs prim_type and prim_data"; return P3D_ERR_ARG; }
    if (motion->n_prims == 0) { *why = "p3d_accumulate_motion::n_prims is 0"; return P3D_ERR_ARG; }
    if (history && !motion->history_prim_data) { *why = "a history needs p3d_accumulate_motion::history_prim_data, the geometry it was rendered with"; return P3D_ERR_ARG; }
    if (motion->memory != 0 && motion->memory != 1) { *why = "p3d_accumulate_motion::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (!frames->hit_id) { *why = "p3d_accumulate_moving needs frames->hit_id: the motion is looked up by it"; return P3D_ERR_ARG; }
    if (const int rc = accumulate_check_planes(params, frames, history, out->rgb32f, out->length, out->prev_xy, out->memory, true, why)) return rc;
    // the first comparison keeps the product of the second (31 bits x 32 bits x 12) inside 64 bits
    if ((uint64_t)params->n_frames * (uint64_t)motion->n_prims > 0x7FFFFFFFull ||
        (uint64_t)params->n_frames * (uint64_t)motion->n_prims * 12 > 0x7FFFFFFFull) {
        *why = "n_frames * n_prims * 12 does not fit 31 bits"; return P3D_ERR_LIMIT;
    }
    if (motion->memory == 0)
        for (uint32_t i = 0; i < motion->n_prims; i++)
            if (motion->prim_type[i] > P3D_PLANE) { *why = "a prim_type is not P3D_SPHERE .. P3D_PLANE"; return P3D_ERR_ARG; }
    const void* const outs[3] = {out->rgb32f, out->length, out->prev_xy};
    for (const void* o : outs)
        if (o && (o == motion->prim_type || o == motion->prim_data || o == motion->history_prim_data)) { *why = "an output plane is an array of the motion"; return P3D_ERR_ARG; }
    return P3D_OK;
}

hipError_t launch_accumulate_moving(const p3d_accumulate_params& p, const AccumulatePlanes& A, const AccumulateMotion& motion,
                                    const p3d_camera* cams, const p3d_camera* hist_cam, hipStream_t stream) {
    const size_t frame = (size_t)p.res_x * (size_t)p.res_y, records = 12 * (size_t)motion.n_prims;
    MovingFrame M;
    memset(&M, 0, sizeof M);
    const uint32_t blocks = first_frame_record(M.F, p);
    M.type = motion.prim_type; M.n_prims = motion.n_prims;
    for (size_t f = 0; f < (size_t)p.n_frames; f++) {
        M.cur = motion.prim_data + f * records;
        M.prev = f > 0 ? motion.prim_data + (f - 1) * records : motion.hist_prim_data;
        M.out_xy = motion.out_prev_xy ? motion.out_prev_xy + 2 * f * frame : nullptr;
        if (next_frame_record(M.F, p, A, cams, hist_cam, f)) hipLaunchKernelGGL(accumulate_moving_kernel<true>, dim3(blocks), dim3(kThreads), 0, stream, M);
        else hipLaunchKernelGGL(accumulate_moving_kernel<false>, dim3(blocks), dim3(kThreads), 0, stream, M);
    }
    return hipGetLastError();
}

}  // namespace p3d
