// p3d_scene_build_grid.cpp -- p3d_scene_build_grid of include/p3d_hip.h: GRID mode's uniform grid of a live scene handle is
// built on the device (grid_device.hip) from the boxes the handle keeps there, with no host copy of the geometry.  The two
// arrays are allocated inside the build, after its limit checks, and installed after its last wait: a call that fails leaves
// the handle's grid state as it was.
#include <cstring>

#include "grid_device.h"
#include "p3d_scene_state.h"

using namespace p3d;

int p3d::ensure_grid_bounds(p3d_scene* s) {
    if (s->grid_bounds.p) return P3D_OK;
    // every update so far came from host memory and refreshed grid_src: it is current
    std::vector<float> rows(6 * s->grid_src.size());
    for (size_t i = 0; i < s->grid_src.size(); i++) {
        memcpy(&rows[6 * i], s->grid_src[i].lo, 12); memcpy(&rows[6 * i + 3], s->grid_src[i].hi, 12);
    }
    DevBuf<float> b;
    HIP_TRY(b.upload(rows));
    s->grid_bounds = std::move(b);
    s->stats.device_bytes += s->grid_bounds.bytes();
    return P3D_OK;
}

extern "C" int p3d_scene_build_grid(p3d_scene* s, p3d_grid_info* info) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    if (s->cull_never_hit)
        return fail(P3D_ERR_STATE, "scene was built with cull_never_hit: GRID mode walks the reference's grid over ALL primitives; use accel BVH");
    HIP_TRY(hipSetDevice(s->device));
    if (stream_capturing(s->stream))
        return fail(P3D_ERR_STATE, "p3d_scene_build_grid allocates and waits on the device: not while the stream is being captured");
    auto report = [&](uint32_t built) {
        if (!info) return;
        info->built = built;
        for (int a = 0; a < 3; a++) { info->n[a] = s->grid_info.n[a]; info->mn[a] = s->grid_info.mn[a]; info->mx[a] = s->grid_info.mx[a]; }
        info->n_cells = s->grid_cells.n - 1; info->n_items = s->grid_items.n;
    };
    if (s->grid_ready) { report(0u); return P3D_OK; }
    int rc = ensure_grid_bounds(s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));       // after everything already enqueued (an update's records, a rebuild's map)
    GridDeviceOut G;
    GridDeviceLimit limit = kGridFits;
    HIP_TRY(build_grid_device(s->grid_bounds.p, s->prim_map.p, (uint32_t)s->prim_map.n, false, s->stream, G, &limit));
    if (limit == kGridTooManyCells) return fail(P3D_ERR_LIMIT, "the reference's grid formula asks for more than 2^31 cells");
    if (limit == kGridTooManyItems) return fail(P3D_ERR_LIMIT, "the grid's cells hold more than 2^32 - 1 primitive references");
    // ---- install: from here on nothing fails
    s->grid_cells.release(); s->grid_items.release();
    s->grid_cells.p = G.cell_start; s->grid_cells.n = (size_t)G.n_cells + 1;
    s->grid_items.p = G.items; s->grid_items.n = (size_t)G.n_items;
    for (int a = 0; a < 3; a++) { s->grid_info.n[a] = G.n[a]; s->grid_info.mn[a] = G.mn[a]; s->grid_info.mx[a] = G.mx[a]; }
    s->stats.device_bytes += s->grid_cells.bytes() + s->grid_items.bytes();
    s->grid_ready = true;
    report(1u);
    return P3D_OK;
}
