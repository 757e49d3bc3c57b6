// indirect_paths_host.cpp -- what p3d_indirect_paths does to a path between two of its rays, in plain loops on the host:
// steps 3 and 4 of the definition of include/p3d_hip.h read operation by operation, float arithmetic without contraction
// (HFLAGS: -ffp-contract=off).  What the device kernel (../indirect_paths.hip) is compared against, bit for bit; it shares no
// code with it.  The rays' answers (step 2) are p3d_trace_rays': the host layer has no traversal of its own.
#include "indirect_paths_host.h"

#include <cmath>

namespace p3d_host {

namespace {

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

// steps 5 and 6 of p3d_ambient_occlusion at radius 1 with the key rng_mix(pk, s)
void cosine_direction(const float Ns[3], uint32_t pk, uint32_t s, float out[3]) {
    const uint32_t key = rng_mix(pk, s);
    float v[3] = {Ns[0], Ns[1], Ns[2]};
    for (uint32_t j = 0; j < 32u; j++) {
        float c[3];
        for (uint32_t i = 0; i < 3u; i++) { const float t = 2.0f * rng_u01(key, 3u * j + i); c[i] = t - 1.0f; }
        const float q0 = c[0] * c[0], q1 = c[1] * c[1], q2 = c[2] * c[2];
        const float q = (q0 + q1) + q2;
        if (q <= 1.0f && q >= kTiny) { normalize(c, v); break; }
    }
    float w[3], wn[3];
    for (int k = 0; k < 3; k++) w[k] = Ns[k] + v[k];
    const float w0 = w[0] * w[0], w1 = w[1] * w[1], w2 = w[2] * w[2];
    if (!((w0 + w1) + w2 >= kTiny)) for (int k = 0; k < 3; k++) w[k] = Ns[k];
    normalize(w, wn);
    for (int k = 0; k < 3; k++) out[k] = wn[k] * 1.0f;
}

}  // namespace

void path_next(size_t m, int32_t b, float bias, const float* origin, const float* dir, const float* t, const float* normal, const int32_t* hit_id,
               const uint32_t* prim_material, const float* materials, const uint32_t* pk0, const uint32_t* sample, float* throughput,
               float* origin_out, float* dir_out, uint8_t* alive_out) {
    for (size_t i = 0; i < m; i++) {
        const float *O = origin + 3 * i, *D = dir + 3 * i, *N = normal + 3 * i;
        float *T = throughput + 3 * i, *On = origin_out + 3 * i, *Dn = dir_out + 3 * i;
        alive_out[i] = hit_id[i] >= 0 ? 1 : 0;
        if (!alive_out[i]) {
            for (int k = 0; k < 3; k++) { On[k] = 0.0f; Dn[k] = 0.0f; }
            continue;
        }
        float P[3], Ns[3];
        for (int k = 0; k < 3; k++) { const float p = D[k] * t[i]; P[k] = O[k] + p; }
        const float* a = materials + 12 * (size_t)prim_material[hit_id[i]];
        for (int k = 0; k < 3; k++) T[k] = b == 0 ? a[k] : T[k] * a[k];
        const float m0 = N[0] * D[0], m1 = N[1] * D[1], m2 = N[2] * D[2];
        const bool away = (m0 + m1) + m2 > 0.0f;
        for (int k = 0; k < 3; k++) { Ns[k] = away ? -N[k] : N[k]; const float p = Ns[k] * bias; On[k] = P[k] + p; }
        cosine_direction(Ns, rng_mix(pk0[i], 0x80000000u + (uint32_t)(b + 1)), sample[i], Dn);
    }
}

void path_add(size_t m, int32_t b, const float* throughput, const float* radiance, const uint8_t* alive, float* sum) {
    for (size_t i = 0; i < 3 * m; i++) {
        if (!alive[i / 3]) continue;
        if (b == 0) { sum[i] = radiance[i]; continue; }
        const float p = throughput[i] * radiance[i];
        sum[i] = sum[i] + p;
    }
}

}  // namespace p3d_host
