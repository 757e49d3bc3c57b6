// tile_coverage_host.h -- the per-frame tile coverage mask of the level-1 launch (csrc/p3d_tile_coverage.h) on the host: the
// same header's statements over a scene description, for the conservativeness tests that run without a GPU.
#ifndef P3D_TILE_COVERAGE_HOST_H
#define P3D_TILE_COVERAGE_HOST_H

#include <stdint.h>

#include "p3d_hip.h"

namespace p3d_host {

// active_out [tiles_y][tiles_x] = 1 where some primitive may touch the tile, for the tiles of 16 x tile_h pixels that cover
// rank's rows of cam's frame (tiles_x = ceil(res_x / 16), tiles_y = p3d_local_rows(res_y, row_block, world) / tile_h).
// Returns 1 when a primitive asked for every tile (a point of it not in front of the eye, or a plane): all are then active.
int32_t tile_coverage(const p3d_camera& cam, int32_t tile_h, int32_t row_block, int32_t rank, int32_t world, uint32_t n_prims,
                      const uint32_t* prim_type, const float* prim_data, uint8_t* active_out);

}  // namespace p3d_host
#endif
