// denoise_variance.hip -- p3d_denoise_variance: p3d_denoise's a-trous filter with its colour stop steered by a per-pixel
// variance of the luminance (SVGF, Schied et al. 2017).  Where the variance says a pixel is still noisy the stop is wide,
// where it has converged the stop closes: inv_c = 1 / (sigma_color * sqrt(g) + 2^-20), g the 3 x 3 Gaussian prefilter of
// the variance around the centre.  The variance is filtered along with the colour (weights squared) and handed to the next
// pass.  IEEE basic operations in one fixed order (include/p3d_hip.h, DESIGN "Variance-guided denoising"), so the device,
// the host restatement (host/denoise_host.cpp) and tests/denoise_variance_reference.py agree in every bit.  Built with the
// ray kernels' flags (-ffp-contract=off, correctly rounded division and square root).
//   The launches are denoise.hip's (denoise_device.h has what the two share): one per pass, all frames of a batch in it, a
//   workgroup of 256 threads on a tile of 32 x 8 pixels, staged in LDS up to P3D_DENOISE_STAGED_MAX_STEP and read through
//   L2 beyond.  The variance rides beside the depth: one more [H][W] plane in the staged tile (44 bytes per pixel: 19 and
//   28 KB at steps 1 and 2) and one more float per pixel in the scratch the passes alternate between (colour [n][H][W][3],
//   then variance [n][H][W]: 16 bytes per pixel).  The prefilter reads the stride-1 neighbours of the centre, which the
//   halo of 2 * step >= 2 pixels always holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "denoise.h"
#include "denoise_device.h"
#include "p3d_device_math.h"

namespace p3d {

namespace {

// A pass of p3d_denoise_variance: denoise.hip's record (its inv_c unused) and the variance.
struct VariancePass {
    DenoisePass P;
    const float* var;        // what the pass reads: [frames][res_y][res_x]
    float* out_var;          // what it writes (may be NULL)
    float sigma_color;
};

__device__ __forceinline__ constexpr float k2(int d) { return d == 0 ? 0.5f : 0.25f; }

// The taps of denoise_device.h with the variance plane beside them.  z1 / v1: the neighbour at stride 1, whatever the step.
template <int S>
struct LdsVarianceTaps {
    static constexpr int W = LdsTaps<S>::W;
    LdsTaps<S> t;
    const float* sv;
    __device__ __forceinline__ float z(int dx, int dy) const { return t.z(dx, dy); }
    __device__ __forceinline__ V3 n(int dx, int dy) const { return t.n(dx, dy); }
    __device__ __forceinline__ V3 a(int dx, int dy) const { return t.a(dx, dy); }
    __device__ __forceinline__ V3 c(int dx, int dy) const { return t.c(dx, dy); }
    __device__ __forceinline__ float v(int dx, int dy) const { return sv[t.at + (dy * W + dx) * S]; }
    __device__ __forceinline__ float z1(int dx, int dy) const { return t.sz[t.at + dy * W + dx]; }
    __device__ __forceinline__ float v1(int dx, int dy) const { return sv[t.at + dy * W + dx]; }
};

// v and v1 are read for taps with a valid depth only, which lie inside the frame.
struct GlobalVarianceTaps {
    GlobalTaps t;
    const float* pv;
    __device__ __forceinline__ float z(int dx, int dy) const { return t.z(dx, dy); }
    __device__ __forceinline__ V3 n(int dx, int dy) const { return t.n(dx, dy); }
    __device__ __forceinline__ V3 a(int dx, int dy) const { return t.a(dx, dy); }
    __device__ __forceinline__ V3 c(int dx, int dy) const { return t.c(dx, dy); }
    __device__ __forceinline__ float v(int dx, int dy) const { return pv[t.index(dx, dy)]; }
    __device__ __forceinline__ size_t index1(int dx, int dy) const {
        return (size_t)((int64_t)t.y + dy) * (size_t)t.res_x + (size_t)((int64_t)t.x + dx);
    }
    __device__ __forceinline__ float z1(int dx, int dy) const {
        const int64_t qx = (int64_t)t.x + dx, qy = (int64_t)t.y + dy;
        if (qx < 0 || qx >= t.res_x || qy < 0 || qy >= t.res_y) return 0.0f;
        return t.pz[index1(dx, dy)];
    }
    __device__ __forceinline__ float v1(int dx, int dy) const { return pv[index1(dx, dy)]; }
};

// One pixel of one pass: include/p3d_hip.h (p3d_denoise_variance), operation by operation.  -> the colour; vout: the variance.
template <typename Taps>
__device__ __forceinline__ V3 filter_pixel(const Taps& T, const VariancePass& Q, float& vout) {
    const DenoisePass& P = Q.P;
    const V3 cp = T.c(0, 0);
    const float zp = T.z(0, 0);
    vout = T.v(0, 0);
    if (!valid_depth(zp)) return cp;
    // the prefiltered variance of the centre, and the colour stop it gives
    float sg = 0.0f, sk = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            if (!valid_depth(T.z1(dx, dy))) continue;
            const float k = k2(dx) * k2(dy);
            sg = sg + k * T.v1(dx, dy);
            sk = sk + k;
        }
    }
    const float g = max0(sg / sk);                   // the centre is valid: sk >= 0.25
    const float inv_c = 1.0f / (Q.sigma_color * fsqrt(g) + 0x1p-20f);
    const V3 np = T.n(0, 0), ap = T.a(0, 0);
    const float inv_z = 1.0f / (P.sigma_depth * zp);
    const float lp = lum(cp);
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    float sw = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float zq = T.z(dx, dy);
            if (!valid_depth(zq)) continue;
            const V3 nq = T.n(dx, dy), aq = T.a(dx, dy), cq = T.c(dx, dy);
            const float vq = T.v(dx, dy);
            const float h = k1(dx) * k1(dy);
            const float tz = max0(1.0f - fabsf(zq - zp) * inv_z), wz = tz * tz;
            const float dn = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
            float wn = max0(dn);
            for (int j = 0; j < P.npow; j++) wn = wn * wn;
            const float da = (fabsf(aq.x - ap.x) + fabsf(aq.y - ap.y)) + fabsf(aq.z - ap.z);
            const float ta = max0(1.0f - da * P.inv_a), wa = ta * ta;
            float w = ((h * wz) * wn) * wa;
            const float tc = max0(1.0f - fabsf(lum(cq) - lp) * inv_c);
            w = w * (tc * tc);
            sum.x = sum.x + w * cq.x; sum.y = sum.y + w * cq.y; sum.z = sum.z + w * cq.z;
            sw = sw + w;
            sv = sv + (w * w) * vq;
        }
    }
    if (!(sw > 0.0f)) return cp;
    vout = sv / (sw * sw);
    return mk(sum.x / sw, sum.y / sw, sum.z / sw);
}

template <int S>
__global__ void __launch_bounds__(kThreads) denoise_variance_staged_kernel(VariancePass Q) {
    const DenoisePass& P = Q.P;
    constexpr int W = LdsTaps<S>::W, H = LdsTaps<S>::H;
    __shared__ float sz[W * H], sv[W * H], sn[3 * W * H], sa[3 * W * H], sc[3 * W * H];
    const Tile t = this_tile(P);
    const int tid = (int)threadIdx.x;
    const int64_t hx0 = t.x0 - 2 * S, hy0 = t.y0 - 2 * S;          // the halo's corner: may lie outside the frame
    for (int i = tid; i < W * H; i += kThreads) {
        const int64_t gy = hy0 + i / W, gx = hx0 + i % W;
        const bool in = gy >= 0 && gy < P.res_y && gx >= 0 && gx < P.res_x;
        const size_t at = t.frame + (size_t)gy * (size_t)P.res_x + (size_t)gx;
        sz[i] = in ? P.depth[at] : 0.0f;                           // outside the frame: not valid
        sv[i] = in ? Q.var[at] : 0.0f;
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
    const LdsVarianceTaps<S> taps = {{sz, sn, sa, sc, (ly + 2 * S) * W + lx + 2 * S}, sv};
    const size_t pixel = t.frame + (size_t)y * (size_t)P.res_x + (size_t)x;
    float v;
    store_pixel(P, pixel, filter_pixel(taps, Q, v));
    if (Q.out_var) Q.out_var[pixel] = v;
}

__global__ void __launch_bounds__(kThreads) denoise_variance_sparse_kernel(VariancePass Q) {
    const DenoisePass& P = Q.P;
    const Tile t = this_tile(P);
    const int64_t x = t.x0 + (int)threadIdx.x % kTileW, y = t.y0 + (int)threadIdx.x / kTileW;
    if (x >= P.res_x || y >= P.res_y) return;
    const GlobalVarianceTaps taps = {{P.depth + t.frame, P.normal + 3 * t.frame, P.albedo + 3 * t.frame, P.color + 3 * t.frame,
                                      (int32_t)x, (int32_t)y, P.res_x, P.res_y, P.step}, Q.var + t.frame};
    const size_t pixel = t.frame + (size_t)y * (size_t)P.res_x + (size_t)x;
    float v;
    store_pixel(P, pixel, filter_pixel(taps, Q, v));
    if (Q.out_var) Q.out_var[pixel] = v;
}

// iterations == 0: colour and variance as they are (neither written where it already lies), and the colour's quantisation.
// n: pixels.
__global__ void __launch_bounds__(256) denoise_variance_copy_kernel(const float* in, const float* vin, size_t n, float* out32, uint8_t* out8, float* vout) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < 3 * n; i += (size_t)gridDim.x * 256) {
        const float v = in[i];
        if (out32 && out32 != in) out32[i] = v;
        if (out8) out8[i] = (uint8_t)u8fromfloat(clamp01(v));
        if (i < n && vout && vout != vin) vout[i] = vin[i];
    }
}

void launch_pass(const VariancePass& Q, uint32_t blocks, hipStream_t stream) {
    switch (Q.P.step <= P3D_DENOISE_STAGED_MAX_STEP ? Q.P.step : 0) {
    case 1: hipLaunchKernelGGL((denoise_variance_staged_kernel<1>), dim3(blocks), dim3(kThreads), 0, stream, Q); break;
    case 2: hipLaunchKernelGGL((denoise_variance_staged_kernel<2>), dim3(blocks), dim3(kThreads), 0, stream, Q); break;
    case 4: hipLaunchKernelGGL((denoise_variance_staged_kernel<4>), dim3(blocks), dim3(kThreads), 0, stream, Q); break;
    default: hipLaunchKernelGGL(denoise_variance_sparse_kernel, dim3(blocks), dim3(kThreads), 0, stream, Q); break;
    }
}

}  // namespace

int denoise_variance_check_request(const p3d_denoise_params* params, const p3d_denoise_variance_inputs* in,
                                   const p3d_denoise_variance_outputs* out, const char** why) {
    *why = "";
    if (!params || !in || !out) { *why = "params / in / out is NULL"; return P3D_ERR_ARG; }
    const p3d_denoise_inputs planes = {in->rgb32f, in->depth, in->normal, in->albedo, in->memory};
    const p3d_outputs colour = {out->rgb8, out->rgb32f, nullptr, out->memory};
    if (const int rc = denoise_check_request(params, &planes, &colour, why)) return rc;
    if (!in->variance) { *why = "p3d_denoise_variance_inputs::variance is NULL: the filter is steered by it"; return P3D_ERR_ARG; }
    if (!(params->sigma_color > 0.0f)) { *why = "sigma_color must be positive here: it is the width of the colour stop in standard deviations"; return P3D_ERR_ARG; }
    // aliasing: out->rgb32f may be in->rgb32f and out->variance may be in->variance; no other output plane may be an input plane
    const void* const ins[5] = {in->rgb32f, in->depth, in->normal, in->albedo, in->variance};
    const void* const outs[3] = {out->rgb32f, out->variance, out->rgb8};
    for (int i = 0; i < 3; i++) {
        if (!outs[i]) continue;
        for (int j = 0; j < 5; j++)
            if (outs[i] == ins[j] && !(i == 0 && j == 0) && !(i == 1 && j == 4)) {
                *why = "an output plane is an input plane other than its own (rgb32f onto rgb32f, variance onto variance)"; return P3D_ERR_ARG;
            }
        for (int j = 0; j < i; j++)
            if (outs[i] == outs[j]) { *why = "two output planes are one plane"; return P3D_ERR_ARG; }
    }
    return P3D_OK;
}

hipError_t launch_denoise_variance(const p3d_denoise_params& p, const float* rgb32f, const float* depth, const float* normal,
                                   const float* albedo, const float* variance, float* scratch0, float* scratch1, float* out_rgb32f,
                                   uint8_t* out_rgb8, float* out_variance, hipStream_t stream) {
    const size_t pixels = (size_t)p.n_frames * (size_t)p.res_x * (size_t)p.res_y;
    if (!out_rgb32f && !out_rgb8 && !out_variance) return hipSuccess;
    if (p.iterations == 0) {
        if (out_rgb8 || out_rgb32f != rgb32f || (out_variance && out_variance != variance)) {
            const size_t n = 3 * pixels, blocks = (n + 255) / 256;
            hipLaunchKernelGGL(denoise_variance_copy_kernel, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream,
                               rgb32f, variance, pixels, out_rgb32f, out_rgb8, out_variance);
        }
        return hipGetLastError();
    }
    VariancePass Q;
    const uint32_t blocks = pass_record(Q.P, p, depth, normal, albedo);
    Q.P.inv_c = 0.0f;
    Q.sigma_color = p.sigma_color;
    float* const scratch[2] = {scratch0, scratch1};         // each: the colour, then the variance
    const float *src = rgb32f, *src_var = variance;
    if (p.iterations == 1 && denoise_variance_in_place(rgb32f, variance, out_rgb32f, out_variance)) {
        // in place: the only pass would write what its neighbours still read
        hipError_t e = hipMemcpyAsync(scratch0, rgb32f, pixels * 12, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(scratch0 + 3 * pixels, variance, pixels * 4, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
        src = scratch0; src_var = scratch0 + 3 * pixels;
    }
    for (int i = 0; i < p.iterations; i++) {
        const bool last = i == p.iterations - 1;
        Q.P.color = src; Q.var = src_var;
        Q.P.out32 = last ? out_rgb32f : scratch[i & 1];
        Q.P.out8 = last ? out_rgb8 : nullptr;
        Q.out_var = last ? out_variance : scratch[i & 1] + 3 * pixels;
        Q.P.step = 1 << i;
        launch_pass(Q, blocks, stream);
        src = Q.P.out32; src_var = Q.out_var;
    }
    return hipGetLastError();
}

}  // namespace p3d
