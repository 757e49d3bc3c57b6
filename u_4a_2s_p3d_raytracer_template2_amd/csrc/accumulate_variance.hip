// accumulate_variance.hip -- p3d_accumulate_variance: p3d_accumulate (or, with a motion, p3d_accumulate_moving) that also
// carries the first two moments of every pixel's luminance through the same gather, and turns them into the variance that
// steers p3d_denoise_variance (SVGF, Schied et al. 2017).  Colour, length and prev_xy are the siblings' in every bit: the
// kernels here are accumulate_device.h's code with its MOMENTS variant switched on, 8 more bytes per tap and no second
// reprojection.  IEEE basic operations in the order of include/p3d_hip.h, which the host restatement
// (host/accumulate_host.cpp) and tests/accumulate_variance_reference.py repeat; the ray kernels' build flags.
//   Two launches per frame, in stream order:
//   - the temporal one: accumulate.hip's / accumulate_motion.hip's launch (one thread per pixel, 64 x 4 tiles, XCD
//     numbering, cameras by value) writing the moments and the temporal variance max(0, m2 - m1^2) beside colour and length;
//   - the spatial one, for pixels whose history is shorter than min_temporal: the variance of the luminance over the
//     (2 radius + 1)^2 neighbours of the frame's INPUT colour, weighted by p3d_denoise's depth and normal stops.  A
//     workgroup (32 x 8 pixels, denoise.hip's tile) none of whose pixels needs it returns after reading its lengths; the
//     others stage the tile and a halo of `radius` pixels of colour, depth and normal in LDS, in the planes' own layout and
//     in coalesced rows, as denoise.hip does (at radius 3: 38 x 14 pixels of 28 bytes, 14.9 KB), pack the pixels that take
//     the estimate into their first lanes and run the taps from LDS.  It is not launched at all when min_temporal == 1 (no
//     length is below 1) or when nobody wants the variance.
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

// A frame of the temporal launch: accumulate_motion.hip's record (its geometry unused without a motion) and the moments.
struct VarianceFrame {
    MovingFrame M;
    const float* pmoments;          // [res_y][res_x][2]: of the frame looked back at (HISTORY only)
    float* out_moments;             // [res_y][res_x][2] or NULL
    float* out_variance;            // [res_y][res_x] or NULL
};

__device__ __forceinline__ float lum(V3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
__device__ __forceinline__ float max0(float v) { return v > 0.0f ? v : 0.0f; }

template <bool HISTORY, bool MOVING>
__global__ void __launch_bounds__(kThreads) accumulate_variance_kernel(VarianceFrame V) {
    const AccumulateFrame& F = V.M.F;
    const uint32_t blk = logical_block(), tile_x = blk % (uint32_t)F.tiles_x, tile_y = blk / (uint32_t)F.tiles_x;
    const int64_t x = (int64_t)tile_x * kTileW + (int)threadIdx.x % kTileW, y = (int64_t)tile_y * kTileH + (int)threadIdx.x / kTileW;
    if (x >= F.res_x || y >= F.res_y) return;
    const size_t pixel = (size_t)y * (size_t)F.res_x + (size_t)x;
    const float* cp = F.color + 3 * pixel;
    const V3 C = mk(cp[0], cp[1], cp[2]);            // read before anything is written: out_color may be color
    const float l = lum(C), l2 = l * l;
    Moments mo = {V.pmoments, {l, l2}, {0.0f, 0.0f}, {l, l2}};
    V3 out = C;
    float len = 1.0f;
    float xy[2] = {__uint_as_float(0x7FC00000u), __uint_as_float(0x7FC00000u)};
    const float Z = F.depth[pixel];
    if (HISTORY) {
        if (valid_depth(Z)) {                        // 0.; a miss reads no id and no record
            // 1. the ray of the frame kernels and the point it reaches (p3d_pinhole.h)
            const V3 d = pinhole_dir(F.uw, F.vh, F.vz, (int32_t)x, (int32_t)y, F.res_x, F.res_y);
            const V3 P = pinhole_point(F.eye, d, Z);
            V3 Q = P, o;
            float ln;
            // 2. to 4. from where that surface point was one frame ago, the moments with the colour
            if ((!MOVING || previous_point(V.M, F.hit[pixel], P, Q)) && reproject_point<MOVING, true>(F, pixel, C, Q, o, ln, xy, &mo)) {
                out = o; len = ln;
            }
        }
    }
    if (F.out_color) { float* o = F.out_color + 3 * pixel; o[0] = out.x; o[1] = out.y; o[2] = out.z; }
    if (F.out_length) F.out_length[pixel] = len;
    if (MOVING && V.M.out_xy) { Float2A v; v.x = xy[0]; v.y = xy[1]; *(Float2*)(V.M.out_xy + 2 * pixel) = v; }
    if (V.out_moments) { Float2A v; v.x = mo.out[0]; v.y = mo.out[1]; *(Float2*)(V.out_moments + 2 * pixel) = v; }
    if (V.out_variance) V.out_variance[pixel] = valid_depth(Z) ? max0(mo.out[1] - mo.out[0] * mo.out[0]) : 0.0f;
}

// ---------------------------------------------------------------- the spatial estimate
constexpr int kSpatialW = 32, kSpatialH = 8, kSpatialThreads = kSpatialW * kSpatialH;

struct SpatialFrame {
    const float *color, *depth, *normal;     // the frame's INPUT planes
    const float* length;                     // the frame's OUTPUT length
    float* variance;                         // the temporal launch has written it; pixels that take the estimate are overwritten
    int32_t res_x, res_y, tiles_x, tiles_y;
    int32_t npow;
    float min_temporal, sigma_depth;
};

template <int R>
__global__ void __launch_bounds__(kSpatialThreads) spatial_variance_kernel(SpatialFrame S) {
    constexpr int W = kSpatialW + 2 * R, H = kSpatialH + 2 * R;
    __shared__ float sz[W * H], sn[3 * W * H], sc[3 * W * H];
    __shared__ uint16_t list[kSpatialThreads];
    __shared__ int count;
    const uint32_t blk = logical_block(), tile_x = blk % (uint32_t)S.tiles_x, tile_y = blk / (uint32_t)S.tiles_x;
    const int tid = (int)threadIdx.x, lx = tid % kSpatialW, ly = tid / kSpatialW;
    const int64_t x0 = (int64_t)tile_x * kSpatialW, y0 = (int64_t)tile_y * kSpatialH, x = x0 + lx, y = y0 + ly;
    const bool inside = x < S.res_x && y < S.res_y;
    const size_t pixel = inside ? (size_t)y * (size_t)S.res_x + (size_t)x : 0;
    const bool wanted = inside && S.length[pixel] < S.min_temporal;
    if (tid == 0) count = 0;
    if (!__syncthreads_or(wanted)) return;           // every history of the tile is long enough
    const int64_t hx0 = x0 - R, hy0 = y0 - R;        // the halo's corner: may lie outside the frame
    for (int i = tid; i < W * H; i += kSpatialThreads) {
        const int64_t gy = hy0 + i / W, gx = hx0 + i % W;
        const bool in = gy >= 0 && gy < S.res_y && gx >= 0 && gx < S.res_x;
        sz[i] = in ? S.depth[(size_t)gy * (size_t)S.res_x + (size_t)gx] : 0.0f;      // outside the frame: not valid
    }
    for (int i = tid; i < 3 * W * H; i += kSpatialThreads) {       // rows of 3 W floats, as they lie in the planes
        const int64_t gy = hy0 + i / (3 * W), g3 = 3 * hx0 + i % (3 * W);
        const bool in = gy >= 0 && gy < S.res_y && g3 >= 0 && g3 < 3 * (int64_t)S.res_x;
        const size_t at = 3 * ((size_t)gy * (size_t)S.res_x) + (size_t)g3;
        sn[i] = in ? S.normal[at] : 0.0f;
        sc[i] = in ? S.color[at] : 0.0f;
    }
    __syncthreads();
    // The pixels that take the estimate are packed into the first lanes: after a few frames they are the disocclusions, a
    // few per tile, and spread over the waves every one of them would hold a whole wave in the loop below.  (The order in
    // the list is that of the LDS atomic and does not matter: a pixel's estimate depends on the pixel alone.)
    const int own = (ly + R) * W + lx + R;
    if (wanted && valid_depth(sz[own])) list[atomicAdd(&count, 1)] = (uint16_t)tid;      // not valid: the temporal launch wrote 0
    __syncthreads();
    if (tid >= count) return;
    const int px = list[tid] % kSpatialW, py = list[tid] / kSpatialW;
    const int at = (py + R) * W + px + R;
    const float zp = sz[at];
    const V3 np = mk(sn[3 * at], sn[3 * at + 1], sn[3 * at + 2]);
    const float inv_z = 1.0f / (S.sigma_depth * zp);
    float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -R; dy <= R; dy++) {
#pragma unroll
        for (int dx = -R; dx <= R; dx++) {
            const int q = at + dy * W + dx;
            const float zq = sz[q];
            if (!valid_depth(zq)) continue;
            const float tz = max0(1.0f - fabsf(zq - zp) * inv_z), wz = tz * tz;
            const float dn = (np.x * sn[3 * q] + np.y * sn[3 * q + 1]) + np.z * sn[3 * q + 2];
            float wn = max0(dn);
            for (int j = 0; j < S.npow; j++) wn = wn * wn;
            const float w = wz * wn;
            const float lq = lum(mk(sc[3 * q], sc[3 * q + 1], sc[3 * q + 2]));
            s1 = s1 + w * lq;
            s2 = s2 + w * (lq * lq);
            sw = sw + w;
        }
    }
    if (!(sw > 0.0f)) return;                        // the temporal variance stays
    const float a = s1 / sw, b = s2 / sw;
    S.variance[(size_t)(y0 + py) * (size_t)S.res_x + (size_t)(x0 + px)] = max0(b - a * a);
}

void launch_spatial(const SpatialFrame& S, int radius, hipStream_t stream) {
    const dim3 blocks((uint32_t)((uint64_t)S.tiles_x * (uint64_t)S.tiles_y)), threads(kSpatialThreads);     // at most the pixel count
    switch (radius) {
    case 1: hipLaunchKernelGGL(spatial_variance_kernel<1>, blocks, threads, 0, stream, S); break;
    case 2: hipLaunchKernelGGL(spatial_variance_kernel<2>, blocks, threads, 0, stream, S); break;
    default: hipLaunchKernelGGL(spatial_variance_kernel<3>, blocks, threads, 0, stream, S); break;
    }
}

template <bool MOVING>
void launch_temporal(const VarianceFrame& V, bool history, uint32_t blocks, hipStream_t stream) {
    if (history) hipLaunchKernelGGL((accumulate_variance_kernel<true, MOVING>), dim3(blocks), dim3(kThreads), 0, stream, V);
    else hipLaunchKernelGGL((accumulate_variance_kernel<false, MOVING>), dim3(blocks), dim3(kThreads), 0, stream, V);
}

}  // namespace

int accumulate_variance_check_request(const p3d_accumulate_params* params, const p3d_accumulate_variance_params* vparams,
                                      const p3d_accumulate_frames* frames, const p3d_accumulate_history* history, const float* history_moments,
                                      const p3d_accumulate_motion* motion, const p3d_accumulate_variance_outputs* out, const char** why) {
    *why = "";
    if (!params || !vparams || !frames || !out) { *why = "params / variance_params / frames / out is NULL"; return P3D_ERR_ARG; }
    if (out->memory != 0 && out->memory != 1) { *why = "p3d_accumulate_variance_outputs::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (!motion && out->prev_xy) { *why = "out->prev_xy needs a motion: without one the world is static and no previous position is formed"; return P3D_ERR_ARG; }
    if (!out->rgb32f && !out->length && !out->prev_xy && !out->moments && !out->variance) { *why = "every output plane is NULL"; return P3D_ERR_ARG; }
    // the siblings' checks on the planes they know; with only new planes wanted they are given one of those, which is no plane of theirs
    const bool only_new = !out->rgb32f && !out->length && !out->prev_xy;
    const float* const stand_in = only_new ? (out->moments ? out->moments : out->variance) : nullptr;
    if (motion) {
        const p3d_accumulate_moving_outputs o = {out->rgb32f, only_new ? const_cast<float*>(stand_in) : out->length, out->prev_xy, out->memory};
        if (const int rc = accumulate_moving_check_request(params, frames, history, motion, &o, why)) return rc;
    } else {
        if (const int rc = accumulate_check_planes(params, frames, history, out->rgb32f, only_new ? stand_in : out->length, nullptr, out->memory, true, why)) return rc;
    }
    if (history && !history_moments) { *why = "a history needs history_moments, the moments it had accumulated"; return P3D_ERR_ARG; }
    if (!history && history_moments) { *why = "history_moments without a history: pass both or neither"; return P3D_ERR_ARG; }
    const p3d_accumulate_variance_params& v = *vparams;
    if (!std::isfinite(v.min_temporal) || !(v.min_temporal >= 1.0f)) { *why = "min_temporal must be finite and at least 1 (1: no spatial estimate)"; return P3D_ERR_ARG; }
    if (v.radius < 1 || v.radius > kAccumulateVarianceMaxRadius) { *why = "radius must be in 1..3"; return P3D_ERR_ARG; }
    if (!std::isfinite(v.sigma_depth) || !(v.sigma_depth > 0.0f)) { *why = "sigma_depth must be finite and positive"; return P3D_ERR_ARG; }
    if (v.normal_power_log2 < 0 || v.normal_power_log2 > 8) { *why = "normal_power_log2 must be in 0..8"; return P3D_ERR_ARG; }
    // aliasing of the new planes: moments and variance may be nothing the launches read and no other output plane
    const void* const news[2] = {out->moments, out->variance};
    const void* const olds[3] = {out->rgb32f, out->length, out->prev_xy};
    for (int i = 0; i < 2; i++) {
        const void* o = news[i];
        if (!o) continue;
        if (o == frames->rgb32f || o == frames->depth || o == frames->normal || o == frames->hit_id) { *why = "out->moments or out->variance is a plane of the frames"; return P3D_ERR_ARG; }
        if (history && (o == history->rgb32f || o == history->depth || o == history->normal || o == history->length || o == history->hit_id || o == history_moments)) {
            *why = "out->moments or out->variance is a plane of the history: the launches read it while they write"; return P3D_ERR_ARG;
        }
        if (motion && (o == motion->prim_type || o == motion->prim_data || o == motion->history_prim_data)) { *why = "out->moments or out->variance is an array of the motion"; return P3D_ERR_ARG; }
        for (const void* p : olds) if (o == p) { *why = "two output planes are one plane"; return P3D_ERR_ARG; }
        if (i == 1 && o == news[0]) { *why = "two output planes are one plane"; return P3D_ERR_ARG; }
    }
    if (history)
        for (const void* p : olds) if (p && p == history_moments) { *why = "an output plane is history_moments: the launches read it while they write"; return P3D_ERR_ARG; }
    return P3D_OK;
}

hipError_t launch_accumulate_variance(const p3d_accumulate_params& p, const p3d_accumulate_variance_params& vp, const AccumulatePlanes& A,
                                      const AccumulateVariancePlanes& VP, const AccumulateMotion* motion, const p3d_camera* cams,
                                      const p3d_camera* hist_cam, hipStream_t stream) {
    const size_t frame = (size_t)p.res_x * (size_t)p.res_y, records = motion ? 12 * (size_t)motion->n_prims : 0;
    const bool many = p.n_frames > 1, spatial = accumulate_variance_spatial(vp, VP.out_variance);
    const bool detour = accumulate_variance_colour_detour(vp, A.rgb32f, A.out_rgb32f, VP.out_variance);
    // the colour of an in-place call goes through the spare plane: the spatial launch still reads the frame's input colour
    AccumulatePlanes B = A;
    if (detour) B.out_rgb32f = nullptr;
    VarianceFrame V;
    memset(&V, 0, sizeof V);
    const uint32_t blocks = first_frame_record(V.M.F, p);
    if (motion) { V.M.type = motion->prim_type; V.M.n_prims = motion->n_prims; }
    SpatialFrame S;
    memset(&S, 0, sizeof S);
    S.res_x = p.res_x; S.res_y = p.res_y;
    S.tiles_x = (int32_t)(((int64_t)p.res_x + kSpatialW - 1) / kSpatialW); S.tiles_y = (int32_t)(((int64_t)p.res_y + kSpatialH - 1) / kSpatialH);
    S.npow = vp.normal_power_log2; S.min_temporal = vp.min_temporal; S.sigma_depth = vp.sigma_depth;
    for (size_t f = 0; f < (size_t)p.n_frames; f++) {
        if (motion) {
            V.M.cur = motion->prim_data + f * records;
            V.M.prev = f > 0 ? motion->prim_data + (f - 1) * records : motion->hist_prim_data;
            V.M.out_xy = motion->out_prev_xy ? motion->out_prev_xy + 2 * f * frame : nullptr;
        }
        V.pmoments = f > 0 ? V.out_moments : VP.hist_moments;        // what the launch of frame f - 1 wrote
        V.out_moments = VP.out_moments ? VP.out_moments + 2 * f * frame : (many ? VP.spare_moments + 2 * (f & 1) * frame : nullptr);
        V.out_variance = VP.out_variance ? VP.out_variance + f * frame : nullptr;
        const bool history = next_frame_record(V.M.F, p, B, cams, hist_cam, f);
        // a single frame has no next frame to keep a plane for, but the spatial launch reads the length, and a detour needs its plane
        if (!V.M.F.out_color && detour) V.M.F.out_color = A.spare_rgb32f;
        if (!V.M.F.out_length && spatial) V.M.F.out_length = A.spare_length;
        if (motion) launch_temporal<true>(V, history, blocks, stream); else launch_temporal<false>(V, history, blocks, stream);
        if (spatial) {
            S.color = V.M.F.color; S.depth = V.M.F.depth; S.normal = V.M.F.normal;
            S.length = V.M.F.out_length; S.variance = V.out_variance;
            launch_spatial(S, vp.radius, stream);
        }
        if (detour) {
            const hipError_t e = hipMemcpyAsync(A.out_rgb32f + 3 * f * frame, V.M.F.out_color, frame * 12, hipMemcpyDeviceToDevice, stream);
            if (e != hipSuccess) return e;
        }
    }
    return hipGetLastError();
}

}  // namespace p3d
