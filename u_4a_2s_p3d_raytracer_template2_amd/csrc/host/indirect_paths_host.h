// indirect_paths_host.h -- the host restatement of steps 3 and 4 of p3d_indirect_paths' definition
// (indirect_paths_host.cpp): what happens to a path between two of its rays.  Vertex 0 (step 1) is ao_segments() at radius 1
// (ao_host.h), the rays' answers (step 2) are p3d_trace_rays', the resolve (step 5) is indirect_resolve() (indirect_host.h).
#ifndef P3D_INDIRECT_PATHS_HOST_H
#define P3D_INDIRECT_PATHS_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "p3d_hip.h"

namespace p3d_host {

// Step 4 for m paths that just traced ray b (0 .. 6): origin, dir [m][3] are Ray(O_b, D_b), t [m], normal [m][3] and hit_id [m]
// (a scene index, -1 = miss) what p3d_trace_rays answered for it; prim_material [n_prims] and materials [n_materials][12] are
// the scene description's; pk0 [m] is the pixel's key and sample [m] the path's sample.  throughput [m][3] holds T_b on
// entry (not read when b == 0) and T_(b+1) on return for the paths that go on.  alive_out [m] is 1 where the path has a
// next vertex (hit_id >= 0); origin_out / dir_out [m][3] are Ray(O_(b+1), D_(b+1)) there and zeros elsewhere, where the
// throughput is left as it was.  The caller knows whether b + 1 < bounces.
void path_next(size_t m, int32_t b, float bias, const float* origin, const float* dir, const float* t, const float* normal, const int32_t* hit_id,
               const uint32_t* prim_material, const float* materials, const uint32_t* pk0, const uint32_t* sample, float* throughput,
               float* origin_out, float* dir_out, uint8_t* alive_out);

// Step 3 for m paths: R = r when b == 0, else R + T * r per channel, a product and then a sum; only where alive [m] is set.
void path_add(size_t m, int32_t b, const float* throughput, const float* radiance, const uint8_t* alive, float* sum);

}  // namespace p3d_host
#endif
