// denoise_host.cpp -- the filters of p3d_denoise and p3d_denoise_variance in plain loops on the host: DESIGN "Denoising" and
// "Variance-guided denoising" read operation by operation, float arithmetic without contraction (HFLAGS: -ffp-contract=off).
// What the device kernels (../denoise.hip, ../denoise_variance.hip) are compared against, bit for bit; it shares no code
// with them.
#include "denoise_host.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace p3d_host {

namespace {

inline bool valid_depth(float z) { return std::isfinite(z) && z > 0.0f; }
inline float max0(float v) { return v > 0.0f ? v : 0.0f; }
inline float lum(const float* c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }
inline float clamp01(float v) { return (v < 0.0f) ? 0.0f : ((v > 1.0f) ? 1.0f : v); }
inline uint8_t u8fromfloat(float x) {                 // RT/maths.h:113-117
    const float s = x * 255.99f;
    return (s >= 255.0f) ? (uint8_t)255 : (uint8_t)(int)s;
}

// one pass over one frame: in -> out, both [res_y][res_x][3]
void denoise_pass(const p3d_denoise_params& p, int pass, const float* in, const float* Z, const float* N, const float* A, float* out) {
    static const float k1[3] = {0.375f, 0.25f, 0.0625f};
    const int W = p.res_x, H = p.res_y, s = 1 << pass;
    const bool color = p.sigma_color > 0.0f;
    const float inv_a = 1.0f / p.sigma_albedo;
    const float inv_c = color ? 1.0f / (p.sigma_color * (1.0f / (float)s)) : 0.0f;
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            const size_t pi = (size_t)y * W + x;
            const float* cp = in + 3 * pi;
            float* o = out + 3 * pi;
            const float zp = Z[pi];
            if (!valid_depth(zp)) { o[0] = cp[0]; o[1] = cp[1]; o[2] = cp[2]; continue; }
            const float inv_z = 1.0f / (p.sigma_depth * zp);
            const float lp = lum(cp);
            const float *np = N + 3 * pi, *ap = A + 3 * pi;
            float sum[3] = {0.0f, 0.0f, 0.0f}, sw = 0.0f;
            for (int dy = -2; dy <= 2; dy++) {
                for (int dx = -2; dx <= 2; dx++) {
                    const long qx = (long)x + (long)dx * s, qy = (long)y + (long)dy * s;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t qi = (size_t)qy * W + (size_t)qx;
                    const float zq = Z[qi];
                    if (!valid_depth(zq)) continue;
                    const float *nq = N + 3 * qi, *aq = A + 3 * qi, *cq = in + 3 * qi;
                    const float h = k1[std::abs(dx)] * k1[std::abs(dy)];
                    const float tz = max0(1.0f - std::fabs(zq - zp) * inv_z);
                    const float wz = tz * tz;
                    const float dn = (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2];
                    float wn = max0(dn);
                    for (int j = 0; j < p.normal_power_log2; j++) wn = wn * wn;
                    const float da = (std::fabs(aq[0] - ap[0]) + std::fabs(aq[1] - ap[1])) + std::fabs(aq[2] - ap[2]);
                    const float ta = max0(1.0f - da * inv_a);
                    const float wa = ta * ta;
                    float w = ((h * wz) * wn) * wa;
                    if (color) {
                        const float tc = max0(1.0f - std::fabs(lum(cq) - lp) * inv_c);
                        const float wc = tc * tc;
                        w = w * wc;
                    }
                    for (int c = 0; c < 3; c++) { const float t = w * cq[c]; sum[c] = sum[c] + t; }
                    sw = sw + w;
                }
            }
            if (sw > 0.0f) { o[0] = sum[0] / sw; o[1] = sum[1] / sw; o[2] = sum[2] / sw; }
            else { o[0] = cp[0]; o[1] = cp[1]; o[2] = cp[2]; }
        }
    }
}

// one pass of p3d_denoise_variance over one frame: (in, vin) -> (out, vout)
void denoise_variance_pass(const p3d_denoise_params& p, int pass, const float* in, const float* vin, const float* Z, const float* N,
                           const float* A, float* out, float* vout) {
    static const float k1[3] = {0.375f, 0.25f, 0.0625f}, k2[2] = {0.5f, 0.25f};
    const int W = p.res_x, H = p.res_y, s = 1 << pass;
    const float inv_a = 1.0f / p.sigma_albedo;
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            const size_t pi = (size_t)y * W + x;
            const float* cp = in + 3 * pi;
            float* o = out + 3 * pi;
            const float zp = Z[pi];
            o[0] = cp[0]; o[1] = cp[1]; o[2] = cp[2];
            vout[pi] = vin[pi];
            if (!valid_depth(zp)) continue;
            float sg = 0.0f, sk = 0.0f;
            for (int dy = -1; dy <= 1; dy++) {
                for (int dx = -1; dx <= 1; dx++) {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t qi = (size_t)qy * W + (size_t)qx;
                    if (!valid_depth(Z[qi])) continue;
                    const float k = k2[std::abs(dx)] * k2[std::abs(dy)];
                    const float t = k * vin[qi];
                    sg = sg + t;
                    sk = sk + k;
                }
            }
            float g = sg / sk;
            g = g > 0.0f ? g : 0.0f;
            const float sd = p.sigma_color * std::sqrt(g);
            const float inv_c = 1.0f / (sd + 0x1p-20f);
            const float inv_z = 1.0f / (p.sigma_depth * zp);
            const float lp = lum(cp);
            const float *np = N + 3 * pi, *ap = A + 3 * pi;
            float sum[3] = {0.0f, 0.0f, 0.0f}, sw = 0.0f, sv = 0.0f;
            for (int dy = -2; dy <= 2; dy++) {
                for (int dx = -2; dx <= 2; dx++) {
                    const long qx = (long)x + (long)dx * s, qy = (long)y + (long)dy * s;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t qi = (size_t)qy * W + (size_t)qx;
                    const float zq = Z[qi];
                    if (!valid_depth(zq)) continue;
                    const float *nq = N + 3 * qi, *aq = A + 3 * qi, *cq = in + 3 * qi;
                    const float h = k1[std::abs(dx)] * k1[std::abs(dy)];
                    const float tz = max0(1.0f - std::fabs(zq - zp) * inv_z);
                    const float wz = tz * tz;
                    const float dn = (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2];
                    float wn = max0(dn);
                    for (int j = 0; j < p.normal_power_log2; j++) wn = wn * wn;
                    const float da = (std::fabs(aq[0] - ap[0]) + std::fabs(aq[1] - ap[1])) + std::fabs(aq[2] - ap[2]);
                    const float ta = max0(1.0f - da * inv_a);
                    const float wa = ta * ta;
                    float w = ((h * wz) * wn) * wa;
                    const float tc = max0(1.0f - std::fabs(lum(cq) - lp) * inv_c);
                    const float wc = tc * tc;
                    w = w * wc;
                    for (int c = 0; c < 3; c++) { const float t = w * cq[c]; sum[c] = sum[c] + t; }
                    sw = sw + w;
                    const float w2 = w * w;
                    const float tv = w2 * vin[qi];
                    sv = sv + tv;
                }
            }
            if (sw > 0.0f) {
                o[0] = sum[0] / sw; o[1] = sum[1] / sw; o[2] = sum[2] / sw;
                const float sw2 = sw * sw;
                vout[pi] = sv / sw2;
            }
        }
    }
}

}  // namespace

void denoise(const p3d_denoise_params& p, const float* rgb32f, const float* depth, const float* normal, const float* albedo,
             float* out_rgb32f, uint8_t* out_rgb8) {
    const size_t frame = (size_t)p.res_x * (size_t)p.res_y, n = frame * (size_t)p.n_frames;
    std::vector<float> cur(rgb32f, rgb32f + 3 * n), next(p.iterations > 0 ? 3 * n : 0);
    for (int i = 0; i < p.iterations; i++) {
        for (int f = 0; f < p.n_frames; f++)
            denoise_pass(p, i, cur.data() + 3 * f * frame, depth + f * frame, normal + 3 * f * frame, albedo + 3 * f * frame,
                         next.data() + 3 * f * frame);
        cur.swap(next);
    }
    if (out_rgb32f) memcpy(out_rgb32f, cur.data(), 3 * n * sizeof(float));
    if (out_rgb8) for (size_t i = 0; i < 3 * n; i++) out_rgb8[i] = u8fromfloat(clamp01(cur[i]));
}

void denoise_variance(const p3d_denoise_params& p, const float* rgb32f, const float* depth, const float* normal, const float* albedo,
                      const float* variance, float* out_rgb32f, uint8_t* out_rgb8, float* out_variance) {
    const size_t frame = (size_t)p.res_x * (size_t)p.res_y, n = frame * (size_t)p.n_frames;
    std::vector<float> cur(rgb32f, rgb32f + 3 * n), next(p.iterations > 0 ? 3 * n : 0);
    std::vector<float> vcur(variance, variance + n), vnext(p.iterations > 0 ? n : 0);
    for (int i = 0; i < p.iterations; i++) {
        for (int f = 0; f < p.n_frames; f++)
            denoise_variance_pass(p, i, cur.data() + 3 * f * frame, vcur.data() + f * frame, depth + f * frame, normal + 3 * f * frame,
                                  albedo + 3 * f * frame, next.data() + 3 * f * frame, vnext.data() + f * frame);
        cur.swap(next);
        vcur.swap(vnext);
    }
    if (out_rgb32f) memcpy(out_rgb32f, cur.data(), 3 * n * sizeof(float));
    if (out_rgb8) for (size_t i = 0; i < 3 * n; i++) out_rgb8[i] = u8fromfloat(clamp01(cur[i]));
    if (out_variance) memcpy(out_variance, vcur.data(), n * sizeof(float));
}

}  // namespace p3d_host
