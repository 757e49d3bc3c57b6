// upsample_host.cpp -- the filter of p3d_upsample in plain loops on the host: DESIGN "Guided upsampling" read operation by
// operation, float arithmetic without contraction (HFLAGS: -ffp-contract=off).  What the device kernel (../upsample.hip) is
// compared against, bit for bit; it shares no code with it.
#include "upsample_host.h"

#include <cmath>

namespace p3d_host {

namespace {

inline bool valid_depth(float z) { return std::isfinite(z) && z > 0.0f; }
inline float max0(float v) { return v > 0.0f ? v : 0.0f; }

// floor(t / d), d > 0
inline long floor_div(long t, long d) { return t >= 0 ? t / d : -((-t + d - 1) / d); }

}  // namespace

void upsample(const p3d_upsample_params& p, const float* low, const float* low_depth, const float* low_normal, const float* depth,
              const float* normal, float* out_plane, uint8_t* out_fallback) {
    const long s = p.factor, lw = p.res_x, lh = p.res_y, W = lw * s, H = lh * s;
    const int c = p.channels;
    for (long f = 0; f < p.n_frames; f++) {
        const float *L = low + (size_t)f * lw * lh * c, *LZ = low_depth + (size_t)f * lw * lh, *LN = low_normal + (size_t)f * lw * lh * 3;
        const float *Z = depth + (size_t)f * W * H, *N = normal + (size_t)f * W * H * 3;
        for (long y = 0; y < H; y++) {
            for (long x = 0; x < W; x++) {
                const size_t pi = (size_t)y * W + x;
                const long tx = 2 * x + 1 - s, ty = 2 * y + 1 - s;
                const long i0 = floor_div(tx, 2 * s), j0 = floor_div(ty, 2 * s);
                const long rx = tx - 2 * s * i0, ry = ty - 2 * s * j0;
                const float fx = (float)rx / (float)(2 * s), fy = (float)ry / (float)(2 * s);
                const float bx[2] = {1.0f - fx, fx}, by[2] = {1.0f - fy, fy};
                const float zp = Z[pi];
                const float* np = N + 3 * pi;
                const bool centre = valid_depth(zp);
                float sum[3] = {0.0f, 0.0f, 0.0f}, sw = 0.0f;
                const float inv_z = centre ? 1.0f / (p.sigma_depth * zp) : 0.0f;
                for (int dy = 0; dy < 2; dy++) {
                    for (int dx = 0; dx < 2; dx++) {
                        const long qx = i0 + dx, qy = j0 + dy;
                        if (qx < 0 || qx >= lw || qy < 0 || qy >= lh) continue;
                        const size_t qi = (size_t)qy * lw + (size_t)qx;
                        const float b = bx[dx] * by[dy];
                        const float zq = LZ[qi];
                        float w;
                        if (centre) {
                            if (!valid_depth(zq)) continue;
                            const float* nq = LN + 3 * qi;
                            const float tz = max0(1.0f - std::fabs(zq - zp) * inv_z);
                            const float wz = tz * tz;
                            const float dn = (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2];
                            float wn = max0(dn);
                            for (int j = 0; j < p.normal_power_log2; j++) wn = wn * wn;
                            const float bz = b * wz;
                            w = bz * wn;
                        } else {
                            if (valid_depth(zq)) continue;
                            w = b;
                        }
                        for (int k = 0; k < c; k++) { const float t = w * L[c * qi + k]; sum[k] = sum[k] + t; }
                        sw = sw + w;
                    }
                }
                uint8_t fell_back = 0;
                if (!(sw > 0.0f)) {                // no low sample explains the pixel: plain bilinear over the taps inside the frame
                    fell_back = 1;
                    sum[0] = sum[1] = sum[2] = 0.0f; sw = 0.0f;
                    for (int dy = 0; dy < 2; dy++) {
                        for (int dx = 0; dx < 2; dx++) {
                            const long qx = i0 + dx, qy = j0 + dy;
                            if (qx < 0 || qx >= lw || qy < 0 || qy >= lh) continue;
                            const size_t qi = (size_t)qy * lw + (size_t)qx;
                            const float b = bx[dx] * by[dy];
                            for (int k = 0; k < c; k++) { const float t = b * L[c * qi + k]; sum[k] = sum[k] + t; }
                            sw = sw + b;
                        }
                    }
                }
                if (out_plane) for (int k = 0; k < c; k++) out_plane[((size_t)f * W * H + pi) * c + k] = sum[k] / sw;
                if (out_fallback) out_fallback[(size_t)f * W * H + pi] = fell_back;
            }
        }
    }
}

}  // namespace p3d_host
