// denoise.hip -- p3d_denoise: an a-trous edge-avoiding wavelet filter (Dammertz et al. 2010: the 5x5 B3-spline kernel,
// pass i with its taps 2^i pixels apart) over a frame's colour, guided by the AOV planes p3d_render_aov writes.  The
// edge-stopping weights are squares of clamped linear ramps -- compact support, IEEE basic operations only, in one fixed
// order (DESIGN "Denoising") -- so the device, the host restatement (host/denoise_host.cpp) and the NumPy one
// (tests/denoise_reference.py) agree in every bit.  Built with the ray kernels' flags (-ffp-contract=off, correctly rounded
// division).
//   One launch per pass, all frames of a batch in it; a workgroup of 256 threads owns a tile of 32 x 8 pixels.
//   - steps 1 and 2: the tile and its halo of 2 * step pixels are copied into LDS first, every plane in its own layout
//     (depth [H][W], the others [H][W][3]), row by row in coalesced dwords; the 25 taps of a pixel then read LDS.  A wave is
//     two tile rows of 32 pixels: each 32-lane half reads 32 consecutive dwords (depth) or dwords 3 apart (the 3-float
//     planes) -- no two lanes of a half on one bank.  (32 + 4s) x (8 + 4s) pixels of 40 bytes: 17 and 26 KB.
//   - steps 4 to 32: the taps are read where they lie, through L2; the lanes of a tap still read consecutive pixels of a
//     row.  At step 4 the halo is 4.5 times the tile (46 KB, three workgroups per CU) and staging measured twice as slow
//     as not staging; from step 8 on it would be 12 to 60 times the tile.
//   Workgroups are numbered so that each XCD (workgroup index mod 8) runs a contiguous range of tiles: neighbouring tiles
//   share halo rows through one L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "denoise.h"
#include "denoise_device.h"
#include "p3d_device_math.h"

namespace p3d {

namespace {

// One pixel of one pass: DESIGN "Denoising", operation by operation.  The taps run dy outer, dx inner: the sums depend on it.
template <bool COLOR, typename Taps>
__device__ __forceinline__ V3 filter_pixel(const Taps& T, const DenoisePass& P) {
    const V3 cp = T.c(0, 0);
    const float zp = T.z(0, 0);
    if (!valid_depth(zp)) return cp;
    const V3 np = T.n(0, 0), ap = T.a(0, 0);
    const float inv_z = 1.0f / (P.sigma_depth * zp);
    const float lp = COLOR ? lum(cp) : 0.0f;
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    float sw = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float zq = T.z(dx, dy);
            if (!valid_depth(zq)) continue;
            const V3 nq = T.n(dx, dy), aq = T.a(dx, dy), cq = T.c(dx, dy);
            const float h = k1(dx) * k1(dy);
            const float tz = max0(1.0f - fabsf(zq - zp) * inv_z), wz = tz * tz;
            const float dn = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
            float wn = max0(dn);
            for (int j = 0; j < P.npow; j++) wn = wn * wn;
            const float da = (fabsf(aq.x - ap.x) + fabsf(aq.y - ap.y)) + fabsf(aq.z - ap.z);
            const float ta = max0(1.0f - da * P.inv_a), wa = ta * ta;
            float w = ((h * wz) * wn) * wa;
            if (COLOR) {
                const float tc = max0(1.0f - fabsf(lum(cq) - lp) * P.inv_c);
                w = w * (tc * tc);
            }
            sum.x = sum.x + w * cq.x; sum.y = sum.y + w * cq.y; sum.z = sum.z + w * cq.z;
            sw = sw + w;
        }
    }
    if (sw > 0.0f) return mk(sum.x / sw, sum.y / sw, sum.z / sw);
    return cp;
}

template <int S, bool COLOR>
__global__ void __launch_bounds__(kThreads) denoise_staged_kernel(DenoisePass P) {
    constexpr int W = LdsTaps<S>::W, H = LdsTaps<S>::H;
    __shared__ float sz[W * H], sn[3 * W * H], sa[3 * W * H], sc[3 * W * H];
    const Tile t = this_tile(P);
    const int tid = (int)threadIdx.x;
    const int64_t hx0 = t.x0 - 2 * S, hy0 = t.y0 - 2 * S;          // the halo's corner: may lie outside the frame
    for (int i = tid; i < W * H; i += kThreads) {
        const int64_t gy = hy0 + i / W, gx = hx0 + i % W;
        const bool in = gy >= 0 && gy < P.res_y && gx >= 0 && gx < P.res_x;
        sz[i] = in ? P.depth[t.frame + (size_t)gy * (size_t)P.res_x + (size_t)gx] : 0.0f;     // outside the frame: not valid
    }
    for (int i = tid; i < 3 * W * H; i += kThreads) {              // rows of 3 W floats, as they lie in the planes
        const int64_t gy = hy0 + i / (3 * W), g3 = 3 * hx0 + i % (3 * W);
        const bool in = gy >= 0 && gy < P.res_y && g3 >= 0 && g3 < 3 * (int64_t)P.res_x;
        const size_t at = 3 * (t.frame + (size_t)gy * (size_t)P.res_x) + (size_t)g3;
        sn[i] = in ? P.normal[at] : 0.0f;
        sa[i] = in ? P.albedo[at] : 0.0f;
        sc[i] = in ? P.color[at] : 0.0f;
    }
    __syncthreads();
    const int lx = tid % kTileW, ly = tid / kTileW;
    const int64_t x = t.x0 + lx, y = t.y0 + ly;
    if (x >= P.res_x || y >= P.res_y) return;
    const LdsTaps<S> taps = {sz, sn, sa, sc, (ly + 2 * S) * W + lx + 2 * S};
    store_pixel(P, t.frame + (size_t)y * (size_t)P.res_x + (size_t)x, filter_pixel<COLOR>(taps, P));
}

template <bool COLOR>
__global__ void __launch_bounds__(kThreads) denoise_sparse_kernel(DenoisePass P) {
    const Tile t = this_tile(P);
    const int64_t x = t.x0 + (int)threadIdx.x % kTileW, y = t.y0 + (int)threadIdx.x / kTileW;
    if (x >= P.res_x || y >= P.res_y) return;
    const GlobalTaps taps = {P.depth + t.frame, P.normal + 3 * t.frame, P.albedo + 3 * t.frame, P.color + 3 * t.frame,
                             (int32_t)x, (int32_t)y, P.res_x, P.res_y, P.step};
    store_pixel(P, t.frame + (size_t)y * (size_t)P.res_x + (size_t)x, filter_pixel<COLOR>(taps, P));
}

// iterations == 0: the colour as it is (not written where it already lies), and its quantisation
__global__ void __launch_bounds__(256) denoise_copy_kernel(const float* in, size_t n, float* out32, uint8_t* out8) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = in[i];
        if (out32 && out32 != in) out32[i] = v;
        if (out8) out8[i] = (uint8_t)u8fromfloat(clamp01(v));
    }
}

template <bool COLOR>
void launch_pass(const DenoisePass& P, uint32_t blocks, hipStream_t stream) {
    switch (P.step <= P3D_DENOISE_STAGED_MAX_STEP ? P.step : 0) {
    case 1: hipLaunchKernelGGL((denoise_staged_kernel<1, COLOR>), dim3(blocks), dim3(kThreads), 0, stream, P); break;
    case 2: hipLaunchKernelGGL((denoise_staged_kernel<2, COLOR>), dim3(blocks), dim3(kThreads), 0, stream, P); break;
    case 4: hipLaunchKernelGGL((denoise_staged_kernel<4, COLOR>), dim3(blocks), dim3(kThreads), 0, stream, P); break;
    default: hipLaunchKernelGGL((denoise_sparse_kernel<COLOR>), dim3(blocks), dim3(kThreads), 0, stream, P); break;
    }
}

}  // namespace

int denoise_check_request(const p3d_denoise_params* params, const p3d_denoise_inputs* in, const p3d_outputs* out, const char** why) {
    *why = "";
    if (!params || !in || !out) { *why = "params / in / out is NULL"; return P3D_ERR_ARG; }
    if (!in->rgb32f || !in->depth || !in->normal || !in->albedo) { *why = "every input plane is needed: rgb32f, depth, normal, albedo"; return P3D_ERR_ARG; }
    if (out->hit_id) { *why = "p3d_outputs::hit_id must be NULL: a denoised frame has no hit ids"; return P3D_ERR_ARG; }
    if (in->memory != 0 && in->memory != 1) { *why = "p3d_denoise_inputs::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    if (out->memory != 0 && out->memory != 1) { *why = "p3d_outputs::memory must be 0 (host) or 1 (device)"; return P3D_ERR_ARG; }
    const p3d_denoise_params& p = *params;
    if (p.res_x < 1 || p.res_y < 1 || p.n_frames < 1) { *why = "res_x, res_y and n_frames must be at least 1"; return P3D_ERR_ARG; }
    if (p.iterations < 0 || p.iterations > kDenoiseMaxIterations) { *why = "iterations must be in 0..6"; return P3D_ERR_ARG; }
    if (p.normal_power_log2 < 0 || p.normal_power_log2 > kDenoiseMaxNormalPowerLog2) { *why = "normal_power_log2 must be in 0..8"; return P3D_ERR_ARG; }
    if (!std::isfinite(p.sigma_depth) || !(p.sigma_depth > 0.0f)) { *why = "sigma_depth must be finite and positive"; return P3D_ERR_ARG; }
    if (!std::isfinite(p.sigma_albedo) || !(p.sigma_albedo > 0.0f)) { *why = "sigma_albedo must be finite and positive"; return P3D_ERR_ARG; }
    if (!std::isfinite(p.sigma_color) || !(p.sigma_color >= 0.0f)) { *why = "sigma_color must be finite and not negative (0: no colour stop)"; return P3D_ERR_ARG; }
    // 64-bit products of 31-bit factors, compared step by step so that none of them wraps
    const uint64_t limit = 0x7FFFFFFFull, pixels = (uint64_t)p.res_x * (uint64_t)p.res_y;
    if (pixels > limit || pixels * (uint64_t)p.n_frames > limit) { *why = "n_frames * res_x * res_y does not fit 31 bits"; return P3D_ERR_LIMIT; }
    return P3D_OK;
}

hipError_t launch_denoise(const p3d_denoise_params& p, const float* rgb32f, const float* depth, const float* normal,
                          const float* albedo, float* scratch0, float* scratch1, float* out_rgb32f, uint8_t* out_rgb8,
                          hipStream_t stream) {
    const size_t pixels = (size_t)p.n_frames * (size_t)p.res_x * (size_t)p.res_y;
    if (!out_rgb32f && !out_rgb8) return hipSuccess;
    if (p.iterations == 0) {
        if (out_rgb8 || out_rgb32f != rgb32f) {
            const size_t n = 3 * pixels, blocks = (n + 255) / 256;
            hipLaunchKernelGGL(denoise_copy_kernel, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, rgb32f, n, out_rgb32f, out_rgb8);
        }
        return hipGetLastError();
    }
    DenoisePass P;
    const uint32_t blocks = pass_record(P, p, depth, normal, albedo);
    float* const scratch[2] = {scratch0, scratch1};
    const float* src = rgb32f;
    if (p.iterations == 1 && out_rgb32f == rgb32f) {       // in place: the only pass would write what its neighbours still read
        const hipError_t e = hipMemcpyAsync(scratch0, rgb32f, pixels * 12, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
        src = scratch0;
    }
    for (int i = 0; i < p.iterations; i++) {
        const bool last = i == p.iterations - 1;
        P.color = src;
        P.out32 = last ? out_rgb32f : scratch[i & 1];
        P.out8 = last ? out_rgb8 : nullptr;
        P.step = 1 << i;
        const bool color = p.sigma_color > 0.0f;
        P.inv_c = color ? 1.0f / (p.sigma_color * (1.0f / (float)(1 << i))) : 0.0f;      // sigma_color * 2^-i: exact
        if (color) launch_pass<true>(P, blocks, stream); else launch_pass<false>(P, blocks, stream);
        src = P.out32;
    }
    return hipGetLastError();
}

}  // namespace p3d
