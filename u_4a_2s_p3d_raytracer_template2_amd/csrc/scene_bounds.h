// scene_bounds.h -- padded bounds of the primitive records as they sit in a scene blob: what the refit of p3d_scene_update
// (scene_update.hip) gives a leaf and what p3d_scene_rebuild (scene_rebuild.hip) gives the device builder.  One statement of
// them, so that a tree rebuilt from the records has the boxes a refit of it would compute.  Device code only; the files that
// include it are built with -ffp-contract=off.  Internal: not installed with include/.
#ifndef P3D_SCENE_BOUNDS_H
#define P3D_SCENE_BOUNDS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scene_update.h"

namespace p3d {

__device__ __forceinline__ float* quad(uint32_t* blob, uint32_t q) { return reinterpret_cast<float*>(blob + 4 * (size_t)q); }
__device__ __forceinline__ const float* quad(const uint32_t* blob, uint32_t q) { return reinterpret_cast<const float*>(blob + 4 * (size_t)q); }

struct Box { float lo[3], hi[3]; };

__device__ __forceinline__ void box_clear(Box& b) {
    for (int a = 0; a < 3; a++) { b.lo[a] = 3.4e38f; b.hi[a] = -3.4e38f; }
}

// scene_flatten.cpp: pad() -- max(1e-3, 1e-5 * |largest coordinate|) on every side -- and the union with b
__device__ __forceinline__ void add_padded(Box& b, const float lo[3], const float hi[3]) {
    float m = 0.0f;
    for (int a = 0; a < 3; a++) m = fmaxf(m, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
    const float p = fmaxf(1e-3f, 1e-5f * m);
    for (int a = 0; a < 3; a++) { b.lo[a] = fminf(b.lo[a], lo[a] - p); b.hi[a] = fmaxf(b.hi[a], hi[a] + p); }
}

__device__ inline void add_tris(Box& b, const SceneRecords& S, uint32_t first, uint32_t n) {
    for (uint32_t k = first; k < first + n; k++) {
        // the triangle the intersector sees is p0, p0 + e1, p0 + e2: the sums round by half an ulp, the pad is 1e-5 of them
        const float* t = quad(S.blob, S.off_tris + S.tri_quads * k);
        float lo[3], hi[3];
        for (int a = 0; a < 3; a++) {
            const float p0 = t[a], p1 = t[a] + t[4 + a], p2 = t[a] + t[8 + a];
            lo[a] = fminf(p0, fminf(p1, p2)); hi[a] = fmaxf(p0, fmaxf(p1, p2));
        }
        add_padded(b, lo, hi);
    }
}
__device__ inline void add_spheres(Box& b, const SceneRecords& S, uint32_t first, uint32_t n) {
    for (uint32_t k = first; k < first + n; k++) {
        const float* s = quad(S.blob, S.off_spheres + k);
        const float r = fabsf(s[3]);
        float lo[3], hi[3];
        for (int a = 0; a < 3; a++) { lo[a] = s[a] - r; hi[a] = s[a] + r; }
        add_padded(b, lo, hi);
    }
}
__device__ inline void add_boxes(Box& b, const SceneRecords& S, uint32_t first, uint32_t n) {
    for (uint32_t k = first; k < first + n; k++) {
        const float* x = quad(S.blob, S.off_boxes + 2u * k);
        float lo[3], hi[3];
        for (int a = 0; a < 3; a++) { lo[a] = fminf(x[a], x[4 + a]); hi[a] = fmaxf(x[a], x[4 + a]); }
        add_padded(b, lo, hi);
    }
}

}  // namespace p3d
#endif
