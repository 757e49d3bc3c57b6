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

// A frame of p3d_accumulate_moving: accumulate.hip's record and the geometry of the two frames.
struct MovingFrame {
    AccumulateFrame F;
    const uint32_t* type;           // [n_prims]
    const float *cur, *prev;        // [n_prims][12]: what the frame was rendered with, and the frame it looks back at (HISTORY only)
    float* out_xy;                  // [res_y][res_x][2] or NULL
    uint32_t n_prims;
};

// 16 bytes of a record as words; the records and the prev_xy plane are only as aligned as their floats
typedef uint32_t Words4A __attribute__((ext_vector_type(4)));
typedef Words4A Words4 __attribute__((aligned(4)));
typedef float Float2A __attribute__((ext_vector_type(2)));
typedef Float2A Float2 __attribute__((aligned(4)));

struct Record { Words4A w[3]; };

__device__ __forceinline__ Record load_record(const float* records, uint32_t i) {
    const Words4* p = (const Words4*)(records + 12 * (size_t)i);
    return {{p[0], p[1], p[2]}};
}
__device__ __forceinline__ float fl(uint32_t w) { return __uint_as_float(w); }
__device__ __forceinline__ float dot3(V3 p, V3 q) { return (p.x * q.x + p.y * q.y) + p.z * q.z; }

// P_prev of include/p3d_hip.h for the hit point P on primitive I.  false: the primitive has changed and its kind gives no point
// one frame ago (a plane): no history.
__device__ __forceinline__ bool previous_point(const MovingFrame& M, int32_t I, V3 P, V3& Q) {
    Q = P;
    if (I < 0 || (uint32_t)I >= M.n_prims) return true;
    const uint32_t k = M.type[I];
    const Record a = load_record(M.cur, (uint32_t)I), b = load_record(M.prev, (uint32_t)I);
    const bool same4 = a.w[0].x == b.w[0].x && a.w[0].y == b.w[0].y && a.w[0].z == b.w[0].z && a.w[0].w == b.w[0].w;
    const bool same6 = same4 && a.w[1].x == b.w[1].x && a.w[1].y == b.w[1].y;
    const bool same9 = same6 && a.w[1].z == b.w[1].z && a.w[1].w == b.w[1].w && a.w[2].x == b.w[2].x;
    if (k == P3D_SPHERE) {
        if (same4) return true;
        const float s = fdiv(fl(b.w[0].w), fl(a.w[0].w));
        Q = mk(fl(b.w[0].x) + (P.x - fl(a.w[0].x)) * s, fl(b.w[0].y) + (P.y - fl(a.w[0].y)) * s, fl(b.w[0].z) + (P.z - fl(a.w[0].z)) * s);
        return true;
    }
    if (k == P3D_TRIANGLE) {
        if (same9) return true;
        const V3 p0 = mk(fl(a.w[0].x), fl(a.w[0].y), fl(a.w[0].z)), p1 = mk(fl(a.w[0].w), fl(a.w[1].x), fl(a.w[1].y));
        const V3 p2 = mk(fl(a.w[1].z), fl(a.w[1].w), fl(a.w[2].x));
        const V3 e1 = mk(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z), e2 = mk(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z);
        const V3 w = mk(P.x - p0.x, P.y - p0.y, P.z - p0.z);
        const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), w1 = dot3(w, e1), w2 = dot3(w, e2);
        const float den = d11 * d22 - d12 * d12;
        const float beta = fdiv(d22 * w1 - d12 * w2, den), gamma = fdiv(d11 * w2 - d12 * w1, den);
        const V3 q0 = mk(fl(b.w[0].x), fl(b.w[0].y), fl(b.w[0].z)), q1 = mk(fl(b.w[0].w), fl(b.w[1].x), fl(b.w[1].y));
        const V3 q2 = mk(fl(b.w[1].z), fl(b.w[1].w), fl(b.w[2].x));
        const V3 f1 = mk(q1.x - q0.x, q1.y - q0.y, q1.z - q0.z), f2 = mk(q2.x - q0.x, q2.y - q0.y, q2.z - q0.z);
        Q = mk((q0.x + f1.x * beta) + f2.x * gamma, (q0.y + f1.y * beta) + f2.y * gamma, (q0.z + f1.z * beta) + f2.z * gamma);
        return true;
    }
    if (k == P3D_BOX) {
        if (same6) return true;
        const float mn[3] = {fl(a.w[0].x), fl(a.w[0].y), fl(a.w[0].z)}, mx[3] = {fl(a.w[0].w), fl(a.w[1].x), fl(a.w[1].y)};
        const float pmn[3] = {fl(b.w[0].x), fl(b.w[0].y), fl(b.w[0].z)}, pmx[3] = {fl(b.w[0].w), fl(b.w[1].x), fl(b.w[1].y)};
        const float p[3] = {P.x, P.y, P.z};
        float r[3];
        for (int c = 0; c < 3; c++) {
            const float e = mx[c] - mn[c];
            const float t = e != 0.0f ? fdiv(p[c] - mn[c], e) : 0.0f;
            r[c] = pmn[c] + (pmx[c] - pmn[c]) * t;
        }
        Q = mk(r[0], r[1], r[2]);
        return true;
    }
    return same4;                    // a plane, or a kind this library does not know: unchanged, or no point to look at
}

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
