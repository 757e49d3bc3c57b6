// indirect_host.cpp -- the sum and the outputs of p3d_indirect_diffuse in plain loops on the host: steps 8 and 9 of the
// definition of include/p3d_hip.h read operation by operation, float arithmetic without contraction (HFLAGS:
// -ffp-contract=off).  What the device kernel (../indirect.hip) is compared against, bit for bit; it shares no code with it.
// The rays are ao_segments() at radius 1 (ao_host.cpp) and the radiances (step 7) are p3d_trace_rays': the host layer has
// no traversal of its own.
#include "indirect_host.h"

namespace p3d_host {

void indirect_resolve(int32_t samples, size_t n_pixels, const float* radiance, const uint8_t* valid, const float* albedo,
                      const float* rgb32f_in, float* indirect_out, float* rgb32f_out) {
    const float inv = 1.0f / (float)samples;             // a power of two: exact
    for (size_t i = 0; i < n_pixels; i++) {
        float m[3] = {0.0f, 0.0f, 0.0f};
        const bool query = valid[i] != 0;
        if (query) {
            const float* r = radiance + 3 * i * (size_t)samples;
            for (int k = 0; k < 3; k++) {
                // 8. the balanced tree in sample order
                float t[64];
                for (int s = 0; s < samples; s++) t[s] = r[3 * s + k];
                for (int n = samples; n > 1; n >>= 1)
                    for (int j = 0; j < n / 2; j++) t[j] = t[2 * j] + t[2 * j + 1];
                m[k] = t[0] * inv;
            }
        }
        // 9.
        for (int k = 0; k < 3; k++) {
            if (indirect_out) indirect_out[3 * i + k] = m[k];
            if (!rgb32f_out) continue;
            const float c = rgb32f_in ? rgb32f_in[3 * i + k] : 0.0f;
            float v = c;
            if (query) {
                const float am = (albedo ? albedo[3 * i + k] : 1.0f) * m[k];
                v = rgb32f_in ? c + am : am;
            }
            rgb32f_out[3 * i + k] = v;
        }
    }
}

}  // namespace p3d_host
