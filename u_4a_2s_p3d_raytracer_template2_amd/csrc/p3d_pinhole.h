// p3d_pinhole.h -- the pinhole ray through a pixel centre and the point it reaches at a depth, as the entries that read
// AOV planes back form them (p3d_accumulate step 1, p3d_ambient_occlusion step 2): the bits of the spp == 0 frame kernels
// (primary_ray_tab of p3d_shade.h, the table entries formed here).  uw, vh, vz are the float products camera_record()
// of p3d_render.cpp hands to the frame kernels: u * w, v * h, n * -plane_dist.
#ifndef P3D_PINHOLE_H
#define P3D_PINHOLE_H

#include "p3d_device_math.h"

namespace p3d {

__device__ __forceinline__ bool valid_depth(float z) { return z > 0.0f && z <= 3.402823466e+38f; }   // finite and > 0; not NaN

// direction of Camera::PrimaryRay((x + 0.5, y + 0.5)), RT/camera.h:91-108
__device__ __forceinline__ V3 pinhole_dir(const float uw[3], const float vh[3], const float vz[3], int32_t x, int32_t y, int32_t res_x,
                                          int32_t res_y) {
    const float fx = fdiv((float)x + 0.5f, (float)res_x) - 0.5f, fy = fdiv((float)y + 0.5f, (float)res_y) - 0.5f;
    const V3 vX = mul(mk(uw[0], uw[1], uw[2]), fx), vY = mul(mk(vh[0], vh[1], vh[2]), fy);
    return normalized(add(add(vX, vY), mk(vz[0], vz[1], vz[2])));
}
// eye + d * Z, per component a product and then a sum
__device__ __forceinline__ V3 pinhole_point(const float eye[3], V3 d, float Z) {
    return mk(eye[0] + d.x * Z, eye[1] + d.y * Z, eye[2] + d.z * Z);
}

}  // namespace p3d
#endif
