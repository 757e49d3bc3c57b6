// ao_host.cpp -- the segments and the resolve of p3d_ambient_occlusion in plain loops on the host: the definition of
// include/p3d_hip.h read operation by operation, float arithmetic without contraction (HFLAGS: -ffp-contract=off).  What the
// device kernel (../ao.hip) is compared against, bit for bit; it shares no code with it.  The queries themselves (step 7) are
// p3d_occluded's: the host layer has no traversal of its own.
#include "ao_host.h"

#include <cmath>

namespace p3d_host {

namespace {

inline bool valid_depth(float z) { return std::isfinite(z) && z > 0.0f; }

inline uint32_t rng_mix(uint32_t a, uint32_t b) {
    uint32_t h = (a ^ 0x9E3779B9u) * 0x85EBCA6Bu + b;
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return h;
}
inline float rng_u01(uint32_t key, uint32_t k) { return (float)(rng_mix(key, k) >> 8) * (1.0f / 16777216.0f); }

inline void normalize(const float a[3], float out[3]) {
    const float s0 = a[0] * a[0], s1 = a[1] * a[1], s2 = a[2] * a[2];
    const float l = 1.0f / std::sqrt((s0 + s1) + s2);
    for (int k = 0; k < 3; k++) out[k] = a[k] * l;
}

constexpr float kTiny = 9.5367431640625e-07f;     // 2^-20

}  // namespace

void ao_segments(const p3d_ao_params& p, const p3d_camera& cam, int32_t frame, int32_t res_x, int32_t res_y, const float* depth,
                 const float* normal, float* origin_out, float* dir_out, uint8_t* valid_out) {
    const int W = res_x, H = res_y, S = p.samples;
    const float rx = (float)W, ry = (float)H;
    float uw[3], vh[3], vz[3];
    for (int k = 0; k < 3; k++) { uw[k] = cam.u[k] * cam.w; vh[k] = cam.v[k] * cam.h; vz[k] = cam.n[k] * -cam.plane_dist; }
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            const size_t pi = (size_t)y * W + x;
            float* const po = origin_out + 3 * pi * S;
            float* const pd = dir_out + 3 * pi * S;
            const float z = depth[pi];
            // 1. validity
            valid_out[pi] = valid_depth(z) ? 1 : 0;
            if (!valid_out[pi]) {
                for (int i = 0; i < 3 * S; i++) { po[i] = 0.0f; pd[i] = 0.0f; }
                continue;
            }
            // 2. Camera::PrimaryRay((x + 0.5, y + 0.5)), RT/camera.h:91-108, and the hit point
            const float fx = ((float)x + 0.5f) / rx - 0.5f, fy = ((float)y + 0.5f) / ry - 0.5f;
            float D[3], d[3], P[3];
            for (int k = 0; k < 3; k++) { const float vx = uw[k] * fx, vy = vh[k] * fy; const float t = vx + vy; D[k] = t + vz[k]; }
            normalize(D, d);
            for (int k = 0; k < 3; k++) { const float t = d[k] * z; P[k] = cam.eye[k] + t; }
            // 3. face-forward, origin
            const float* N = normal + 3 * pi;
            const float m0 = N[0] * d[0], m1 = N[1] * d[1], m2 = N[2] * d[2];
            const bool away = (m0 + m1) + m2 > 0.0f;
            float Ns[3], O[3];
            for (int k = 0; k < 3; k++) { Ns[k] = away ? -N[k] : N[k]; const float t = Ns[k] * p.bias; O[k] = P[k] + t; }
            // 4. keys
            const uint32_t pk = rng_mix(p.seed + (uint32_t)frame, (uint32_t)y * (uint32_t)W + (uint32_t)x);
            for (int s = 0; s < S; s++) {
                const uint32_t key = rng_mix(pk, (uint32_t)s);
                // 5. a uniform point on the sphere by rejection
                float v[3] = {Ns[0], Ns[1], Ns[2]};
                for (uint32_t j = 0; j < 32u; j++) {
                    float c[3];
                    for (uint32_t i = 0; i < 3u; i++) { const float t = 2.0f * rng_u01(key, 3u * j + i); c[i] = t - 1.0f; }
                    const float q0 = c[0] * c[0], q1 = c[1] * c[1], q2 = c[2] * c[2];
                    const float q = (q0 + q1) + q2;
                    if (q <= 1.0f && q >= kTiny) { normalize(c, v); break; }
                }
                // 6. cosine-weighted direction
                float w[3], wn[3];
                for (int k = 0; k < 3; k++) w[k] = Ns[k] + v[k];
                const float w0 = w[0] * w[0], w1 = w[1] * w[1], w2 = w[2] * w[2];
                if (!((w0 + w1) + w2 >= kTiny)) for (int k = 0; k < 3; k++) w[k] = Ns[k];
                normalize(w, wn);
                for (int k = 0; k < 3; k++) { po[3 * s + k] = O[k]; pd[3 * s + k] = wn[k] * p.radius; }
            }
        }
    }
}

void ao_resolve(int32_t samples, size_t n_pixels, const int32_t* occluded, const float* rgb32f_in, float* ao_out, float* rgb32f_out) {
    for (size_t i = 0; i < n_pixels; i++) {
        const float ao = (float)(samples - occluded[i]) / (float)samples;
        if (ao_out) ao_out[i] = ao;
        if (!rgb32f_out) continue;
        for (int k = 0; k < 3; k++) rgb32f_out[3 * i + k] = rgb32f_in ? ao * rgb32f_in[3 * i + k] : ao;
    }
}

}  // namespace p3d_host
