// p3d_ao_segment.h -- steps 4 to 6 of p3d_ambient_occlusion's definition (include/p3d_hip.h) in a lane: the cosine-weighted
// segment of one sample of a pixel, from the counter-based random streams of p3d_shade.h.  Said once for the two kernels
// that make their rays in lanes: wf_ao_kernel (ao.hip) and wf_indirect_kernel (indirect.hip), whose ray of sample s is this
// segment at radius 1, and wf_indirect_paths_kernel (indirect_paths.hip), every vertex of whose paths draws one.
#ifndef P3D_AO_SEGMENT_H
#define P3D_AO_SEGMENT_H

#include <stdint.h>

#include "p3d_shade.h"

namespace p3d {

constexpr uint32_t kAoTries = 32u;         // rejection draws of step 5
constexpr float kAoTiny = 0x1p-20f;        // least squared length steps 5 and 6 normalise

// Steps 4 (the sample's key) to 6 for sample s of the pixel with key pk: L, the segment's direction times its length.
// `live`: the lane has a query; the loop ends when no live lane of the wave is still drawing.
__device__ __forceinline__ V3 ao_segment(V3 Ns, uint32_t pk, uint32_t s, float radius, bool live) {
    const uint32_t k = rng_mix(pk, s);
    V3 c = mk(0.0f, 0.0f, 0.0f);
    bool accepted = false;
#pragma nounroll
    for (uint32_t j = 0; j < kAoTries; j++) {
        if (__ballot(live && !accepted) == 0) break;
        const float c0 = 2.0f * rng_u01(k, 3u * j) - 1.0f, c1 = 2.0f * rng_u01(k, 3u * j + 1u) - 1.0f, c2 = 2.0f * rng_u01(k, 3u * j + 2u) - 1.0f;
        const float q = (c0 * c0 + c1 * c1) + c2 * c2;
        const bool take = !accepted && q <= 1.0f && q >= kAoTiny;
        if (take) c = mk(c0, c1, c2);
        accepted = accepted || take;
    }
    V3 v = Ns;
    if (accepted) v = normalized(c);
    V3 w = add(Ns, v);
    if (!((w.x * w.x + w.y * w.y) + w.z * w.z >= kAoTiny)) w = Ns;
    return mul(normalized(w), radius);
}

}  // namespace p3d
#endif
