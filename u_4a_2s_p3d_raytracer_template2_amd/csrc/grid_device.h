// grid_device.h -- the reference's uniform grid (grid_builder.h: build_grid) built on the device (grid_device.hip): what
// p3d_scene_build_grid (p3d_scene_build_grid.cpp) and the probe p3d_debug_grid_build run.  Internal: not installed with include/.
#ifndef P3D_GRID_DEVICE_H
#define P3D_GRID_DEVICE_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct p3d_scene;

namespace p3d {

// What the device build made: build_grid()'s dims and box, and its two arrays in device memory.
struct GridDeviceOut {
    int32_t   n[3] = {1, 1, 1};
    float     mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    uint64_t  n_cells = 1, n_items = 0;
    uint32_t* cell_start = nullptr;     // [n_cells + 1], hipMalloc'ed here: the caller's to free (nullptr: sizes only)
    uint32_t* items = nullptr;          // [max(n_items, 1)], likewise
};
enum GridDeviceLimit { kGridFits = 0, kGridTooManyCells = 1, kGridTooManyItems = 2 };

// build_grid() over n boxes in device memory: bounds6 [n][6] (lo xyz, hi xyz, scene order) and ref [n], the reference each
// box's primitive is listed under.  out.cell_start and out.items are, word for word, the GridHost arrays build_grid() makes of
// the same boxes and refs.  Synchronous: enqueued on `stream`, with waits for the bounds (six floats), for the item total, and
// for the finished arrays.  All scratch is freed before return.  sizes_only: dims, box and totals, no arrays.
// *limit != kGridFits: the grid is not built (more than 2^31 - 1 cells, the host rule; or an item total beyond 32 bits), found
// before either array is allocated.  On an error nothing is left allocated.
hipError_t build_grid_device(const float* bounds6, const uint32_t* ref, uint32_t n, bool sizes_only, hipStream_t stream,
                             GridDeviceOut& out, GridDeviceLimit* limit);

// The handle's grid_bounds array ([n_prims][6], scene order), made of grid_src on first need: by the first update from
// device memory, before its kernel runs, or by the first p3d_scene_build_grid.  Counted in device_bytes.  A P3D_* code.
int ensure_grid_bounds(p3d_scene* s);

}  // namespace p3d
#endif
