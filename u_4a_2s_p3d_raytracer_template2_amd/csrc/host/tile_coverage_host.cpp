// tile_coverage_host.cpp -- see tile_coverage_host.h.  The camera products are camera_record()'s of p3d_render.cpp and the
// points are what the pre-pass kernel forms from the device records: a triangle's P0, P0 + (P1 - P0), P0 + (P2 - P0) with
// the differences rounded to float as TriRec holds them, a sphere's centre -+ radius, a box's min and max.
#include "tile_coverage_host.h"

#include <cstring>

#include "../p3d_tile_coverage.h"

namespace p3d_host {

int32_t tile_coverage(const p3d_camera& cam, int32_t tile_h, int32_t row_block, int32_t rank, int32_t world, uint32_t n_prims,
                      const uint32_t* prim_type, const float* prim_data, uint8_t* active_out) {
    using namespace p3d;
    float uw[3], vh[3], vz[3];
    for (int a = 0; a < 3; a++) { uw[a] = cam.u[a] * cam.w; vh[a] = cam.v[a] * cam.h; vz[a] = cam.n[a] * -cam.plane_dist; }
    const CoverCamera c = cover_camera(cam.eye, uw, vh, vz);
    CoverTiles g;
    g.res_x = cam.res_x; g.res_y = cam.res_y; g.tile_h = tile_h;
    const int32_t n_blocks = (cam.res_y + row_block - 1) / row_block;           // p3d_local_rows(), restated: no device library here
    g.tiles_x = (cam.res_x + 15) / 16; g.tiles_y = ((n_blocks + world - 1) / world) * row_block / tile_h;
    g.row_block = row_block; g.rank = rank; g.world = world;
    const size_t n_tiles = (size_t)g.tiles_x * (size_t)g.tiles_y;
    memset(active_out, 0, n_tiles);
    bool all = !c.ok;
    for (int32_t ty = 0; ty < g.tiles_y && !all; ty++) {
        for (uint32_t i = 0; i < n_prims && !all; i++) {
            const float* v = prim_data + 12 * (size_t)i;
            double pts[8][3];
            CoverRow r;
            if (prim_type[i] == P3D_TRIANGLE) {
                float e1[3], e2[3];
                for (int a = 0; a < 3; a++) { e1[a] = v[3 + a] - v[a]; e2[a] = v[6 + a] - v[a]; }
                cover_triangle_points(v, e1, e2, pts);
                r = cover_row<3>(c, g, pts, ty);
            } else if (prim_type[i] == P3D_SPHERE || prim_type[i] == P3D_BOX) {
                double lo[3], hi[3];
                for (int a = 0; a < 3; a++) {
                    lo[a] = prim_type[i] == P3D_SPHERE ? (double)v[a] - (double)v[3] : (double)v[a];
                    hi[a] = prim_type[i] == P3D_SPHERE ? (double)v[a] + (double)v[3] : (double)v[3 + a];
                }
                cover_box_points(lo, hi, pts);
                r = cover_row<8>(c, g, pts, ty);
            } else {
                r.all = true;                       // a plane has no bounds
            }
            if (r.all) { all = true; break; }
            if (r.any)
                for (int32_t tx = r.tx0 < 0 ? 0 : r.tx0; tx <= r.tx1 && tx < g.tiles_x; tx++) active_out[(size_t)ty * g.tiles_x + tx] = 1;
        }
    }
    if (all) memset(active_out, 1, n_tiles);
    return all ? 1 : 0;
}

}  // namespace p3d_host
