// grid_builder.h -- the reference's uniform grid (Grid::Build, RT/grid.cpp:30-98) as flat arrays for the device:
// same bounding box, same cell-count formula, same cell populations in the same (scene) order.  Unlike the
// BVH, whose shape is free because the reference discards its closest-hit result, the grid's
// shape is part of GRID mode's observable behaviour: hits are accepted per cell (RT/grid.cpp:265-309).
#ifndef P3D_GRID_BUILDER_H
#define P3D_GRID_BUILDER_H

#include <cstdint>
#include <vector>

#include "p3d_device_types.h"
#include "p3d_hip.h"

namespace p3d {

constexpr float kGridEps = 0.001f;                                       // EPSILON, RT/macros.h:1

struct GridHost {
    int32_t n[3] = {0, 0, 0};
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    std::vector<uint32_t> cell_start;     // n[0]*n[1]*n[2] + 1 offsets into items
    std::vector<uint32_t> items;          // primitive refs (kind << 30 | index within the kind), scene order per cell
};

// one entry per primitive of the scene, in scene order: the bounding box Object::GetBoundingBox() returns
// (RT/scene.cpp:42-44,180-186,194-196; planes: the default [-1,1]^3 of RT/scene.h:75) and the
// primitive's device reference
struct GridPrim { float lo[3], hi[3]; uint32_t ref; };

// The box rule, stated once: lo / hi of one primitive of kind `type` (P3D_*; anything else: a plane) from its 12 floats, with
// the reference's float arithmetic.  The host (grid_prim_bounds) and the device (update_records_kernel, which keeps the
// handle's grid_bounds current) both call it; min and max are std::min's and std::max's selections written out.
P3D_HD inline void grid_box_rule(uint32_t type, const float* v, float* lo, float* hi) {
    switch (type) {
    case P3D_SPHERE:                                                 // RT/scene.cpp:180-186
        for (int a = 0; a < 3; a++) { lo[a] = v[a] - v[3]; hi[a] = v[a] + v[3]; }
        break;
    case P3D_TRIANGLE:                                               // RT/scene.cpp:26-39: min/max, then -= / += EPSILON
        for (int a = 0; a < 3; a++) {
            float mn = v[3 + a] < v[a] ? v[3 + a] : v[a], mx = v[a] < v[3 + a] ? v[3 + a] : v[a];
            mn = v[6 + a] < mn ? v[6 + a] : mn; mx = mx < v[6 + a] ? v[6 + a] : mx;
            lo[a] = mn - kGridEps; hi[a] = mx + kGridEps;
        }
        break;
    case P3D_BOX:                                                    // RT/scene.cpp:194-196
        for (int a = 0; a < 3; a++) { lo[a] = v[a]; hi[a] = v[3 + a]; }
        break;
    default:                                                         // Plane: Object::GetBoundingBox(), RT/scene.h:75
        for (int a = 0; a < 3; a++) { lo[a] = -1.0f; hi[a] = 1.0f; }
        break;
    }
}
// grid_box_rule into g.lo / g.hi; g.ref is left alone
void grid_prim_bounds(uint32_t type, const float* prim12, GridPrim& g);
// bounding boxes of a scene description in scene order, with the reference's float arithmetic
void grid_prims_from_desc(const p3d_scene_desc& d, std::vector<GridPrim>& out);
// The shape rule (RT/grid.cpp:30-56) from the bounds of all boxes (mn / mx as AABB::extend leaves them: FLT_MAX / -FLT_MAX
// for no primitives) and the primitive count: out.mn / out.mx (the bounds -/+ EPSILON) and out.n.  Shared by build_grid and the
// device build (grid_device.hip), which gets the bounds from a reduction on the device.
enum GridShape {
    kGridShapeCells = 0,      // a grid of out.n cells to fill
    kGridShapeEmpty = 1,      // no primitives, or a count that is no number: ONE empty cell, the box as it stands
    kGridShapeTooLarge = 2    // more than 2^31 - 1 cells: nothing is built
};
GridShape grid_shape(size_t n_prims, const float mn[3], const float mx[3], GridHost& out);
// false: the reference's cell-count formula asks for more than 2^31 cells (nothing is built)
bool build_grid(const std::vector<GridPrim>& prims, GridHost& out);

}  // namespace p3d
#endif
