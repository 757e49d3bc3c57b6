#include "grid_builder.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "p3d_device_types.h"

namespace p3d {

void grid_prim_bounds(uint32_t type, const float* v, GridPrim& g) { grid_box_rule(type, v, g.lo, g.hi); }

void grid_prims_from_desc(const p3d_scene_desc& d, std::vector<GridPrim>& out) {
    out.clear();
    out.reserve(d.n_prims);
    uint32_t n_kind[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < d.n_prims; i++) {
        const uint32_t kind = d.prim_type[i] <= P3D_BOX ? d.prim_type[i] : (uint32_t)P3D_PLANE;
        GridPrim g;
        grid_prim_bounds(kind, d.prim_data + 12 * (size_t)i, g);
        g.ref = (kind << kRefKindShift) | n_kind[kind]++;
        out.push_back(g);
    }
}

static inline double dclamp(double x, double mn, double mx) { return x < mn ? mn : (x > mx ? mx : x); }   // RT/maths.h:50-53

GridShape grid_shape(size_t n_prims, const float lo[3], const float hi[3], GridHost& G) {     // RT/grid.cpp:30-56
    float mn[3], mx[3];
    for (int a = 0; a < 3; a++) { mn[a] = lo[a] - kGridEps; mx[a] = hi[a] + kGridEps; G.mn[a] = mn[a]; G.mx[a] = mx[a]; }
    const double wx = mx[0] - mn[0], wy = mx[1] - mn[1], wz = mx[2] - mn[2];
    const double s = pow((int)n_prims / (wx * wy * wz), 0.3333333);
    const float m = 2.0f;                                                // RT/rayAccelerator.h:29
    const double fx = m * wx * s + 1, fy = m * wy * s + 1, fz = m * wz * s + 1;
    // No primitives (the box is still inverted: widths of -inf, s = 0, NaN counts) or coordinates that are not
    // numbers: the reference's int conversion of such a count is undefined behaviour.  Here: ONE empty cell and the
    // box as it stands -- an inverted box is missed by every ray (grid_init), which is what an empty grid amounts to.
    if (n_prims == 0 || !(fx >= 1.0 && fy >= 1.0 && fz >= 1.0) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(fz)) {
        G.n[0] = G.n[1] = G.n[2] = 1;
        return kGridShapeEmpty;
    }
    if (fx * fy * fz > 2147483647.0) return kGridShapeTooLarge;          // more cells than the device's 32-bit cell index
    G.n[0] = (int)fx; G.n[1] = (int)fy; G.n[2] = (int)fz;
    return kGridShapeCells;
}

bool build_grid(const std::vector<GridPrim>& prims, GridHost& G) {       // RT/grid.cpp:30-98
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (const GridPrim& p : prims)
        for (int a = 0; a < 3; a++) {                                    // AABB::extend, RT/boundingBox.cpp:52-60
            if (mn[a] > p.lo[a]) mn[a] = p.lo[a];
            if (mx[a] < p.hi[a]) mx[a] = p.hi[a];
        }
    const GridShape shape = grid_shape(prims.size(), mn, mx, G);
    if (shape == kGridShapeEmpty) {
        G.cell_start.assign(2, 0u);
        G.items.clear();
        return true;
    }
    if (shape == kGridShapeTooLarge) return false;
    for (int a = 0; a < 3; a++) { mn[a] = G.mn[a]; mx[a] = G.mx[a]; }
    const int nx = G.n[0], ny = G.n[1], nz = G.n[2];
    const size_t cells = (size_t)nx * ny * nz;
    struct Range { int x0, x1, y0, y1, z0, z1; };
    std::vector<Range> rng(prims.size());
    G.cell_start.assign(cells + 1, 0u);
    for (size_t i = 0; i < prims.size(); i++) {
        const GridPrim& p = prims[i];
        Range r;
        r.x0 = dclamp((p.lo[0] - mn[0]) * nx / (mx[0] - mn[0]), 0, nx - 1);
        r.y0 = dclamp((p.lo[1] - mn[1]) * ny / (mx[1] - mn[1]), 0, ny - 1);
        r.z0 = dclamp((p.lo[2] - mn[2]) * nz / (mx[2] - mn[2]), 0, nz - 1);
        r.x1 = dclamp((p.hi[0] - mn[0]) * nx / (mx[0] - mn[0]), 0, nx - 1);
        r.y1 = dclamp((p.hi[1] - mn[1]) * ny / (mx[1] - mn[1]), 0, ny - 1);
        r.z1 = dclamp((p.hi[2] - mn[2]) * nz / (mx[2] - mn[2]), 0, nz - 1);
        rng[i] = r;
        for (int iz = r.z0; iz <= r.z1; iz++)
            for (int iy = r.y0; iy <= r.y1; iy++)
                for (int ix = r.x0; ix <= r.x1; ix++) G.cell_start[(size_t)ix + (size_t)nx * iy + (size_t)nx * ny * iz + 1]++;
    }
    for (size_t c = 0; c < cells; c++) G.cell_start[c + 1] += G.cell_start[c];
    G.items.assign(G.cell_start[cells], 0u);
    std::vector<uint32_t> fill(G.cell_start.begin(), G.cell_start.end() - 1);
    for (size_t i = 0; i < prims.size(); i++) {                          // scene order inside every cell (push_back order)
        const Range& r = rng[i];
        for (int iz = r.z0; iz <= r.z1; iz++)
            for (int iy = r.y0; iy <= r.y1; iy++)
                for (int ix = r.x0; ix <= r.x1; ix++) G.items[fill[(size_t)ix + (size_t)nx * iy + (size_t)nx * ny * iz]++] = prims[i].ref;
    }
    return true;
}

}  // namespace p3d
