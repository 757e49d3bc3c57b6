// grid_device.hip -- Grid::Build (RT/grid.cpp:30-98; grid_builder.cpp: build_grid) on the device.  The grid's shape is
// observable (hits are accepted per cell), so this is not "a" grid over the boxes but the host's arrays, word for word:
//   1. bounds of all boxes: wave reduction, one combine per workgroup (min and max are exact in any order); six floats come
//      back and the host applies the shape rule (grid_builder.cpp: grid_shape, shared with build_grid)
//   2. per primitive the six cell indices with the host's float expression, and the number of cells it covers
//   3. exclusive scan of those counts (64-bit: the total is checked against 32 bits before anything is allocated for it)
//   4. every (cell, scene index) pair, written at the primitive's offset: pairs leave in scene order
//   5. STABLE radix sort by cell over the bits a cell index uses: scene order inside every cell, as push_back gives it
//   6. cell_start[c] = first pair of a cell >= c (binary search: empty runs cost nothing extra); items = ref[scene index]
// A primitive that covers many cells (a ground box, a plane's [-1,1]^3 in a fine grid) is walked by all 64 lanes of its wave.
// Built with the ray kernels' flags: -ffp-contract=off and correctly rounded divide, which step 2 depends on.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <cfloat>
#include <cstring>

#include "grid_builder.h"
#include "grid_device.h"

namespace p3d {

namespace {

constexpr unsigned kThreads = 256, kWaves = kThreads / 64;
constexpr unsigned kBoundsBlocks = 1024;      // step 1 strides: at most this many combines per word
constexpr uint32_t kLaneCells = 64;           // a primitive covering more cells than this is walked by its whole wave

struct GridDims { int32_t n[3]; float mn[3], mx[3]; };
struct CellRange { int32_t lo[3], hi[3]; };

// floats as unsigned words of the same order (atomicMin / atomicMax on them)
__device__ __forceinline__ uint32_t ordered(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
float unordered(uint32_t e) {
    const uint32_t u = (e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e;
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// out[0..2]: ordered() minima of lo, out[3..5]: ordered() maxima of hi; preset to all ones / all zeros
__global__ void grid_bounds_kernel(const float* __restrict__ bounds6, uint32_t n, uint32_t* out) {
    __shared__ float part[kWaves][6];
    float v[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const float* b = bounds6 + 6 * i;
        for (int a = 0; a < 3; a++) { v[a] = fminf(v[a], b[a]); v[3 + a] = fmaxf(v[3 + a], b[3 + a]); }
    }
    for (int off = 32; off >= 1; off >>= 1)
        for (int a = 0; a < 3; a++) { v[a] = fminf(v[a], __shfl_xor(v[a], off)); v[3 + a] = fmaxf(v[3 + a], __shfl_xor(v[3 + a], off)); }
    if ((threadIdx.x & 63u) == 0u)
        for (int a = 0; a < 6; a++) part[threadIdx.x >> 6][a] = v[a];
    __syncthreads();
    if (threadIdx.x < 6u) {
        float r = part[0][threadIdx.x];
        for (unsigned w = 1; w < kWaves; w++) r = threadIdx.x < 3u ? fminf(r, part[w][threadIdx.x]) : fmaxf(r, part[w][threadIdx.x]);
        if (threadIdx.x < 3u) atomicMin(out + threadIdx.x, ordered(r)); else atomicMax(out + threadIdx.x, ordered(r));
    }
}

// grid_builder.cpp:80-85 -- the float expression (v - mn) * nx / (mx - mn) with nx converted to float, widened, clamped to
// [0, nx - 1] (dclamp, RT/maths.h:50-53) and truncated
__device__ __forceinline__ int32_t cell_index(float v, float mn, float mx, int32_t n) {
    const double x = (double)((v - mn) * (float)n / (mx - mn));
    const double top = (double)(n - 1);
    return (int32_t)(x < 0.0 ? 0.0 : (x > top ? top : x));
}
__device__ __forceinline__ CellRange cell_range(const float* b, const GridDims& G) {
    CellRange r;
    for (int a = 0; a < 3; a++) {
        r.lo[a] = cell_index(b[a], G.mn[a], G.mx[a], G.n[a]);
        r.hi[a] = cell_index(b[3 + a], G.mn[a], G.mx[a], G.n[a]);
    }
    return r;
}
// cells the host's three loops visit: none when a range is inverted (a box given with min > max)
__device__ __forceinline__ uint32_t cells_covered(const CellRange& r) {
    uint32_t c = 1u;             // at most nx * ny * nz < 2^31
    for (int a = 0; a < 3; a++) c *= r.hi[a] >= r.lo[a] ? (uint32_t)(r.hi[a] - r.lo[a] + 1) : 0u;
    return c;
}

__global__ void grid_count_kernel(const float* __restrict__ bounds6, uint32_t n, GridDims G, uint64_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    count[i] = cells_covered(cell_range(bounds6 + 6 * (size_t)i, G));
}

// pair j of a primitive whose range is r: x fastest, as the host's loops run (the order inside a primitive does not matter
// to a stable sort by cell: a primitive is in a cell once)
__device__ __forceinline__ uint32_t cell_of(const CellRange& r, uint32_t j, const GridDims& G) {
    const uint32_t dx = (uint32_t)(r.hi[0] - r.lo[0] + 1), dy = (uint32_t)(r.hi[1] - r.lo[1] + 1);
    const uint32_t t = j / dx;
    const uint32_t ix = (uint32_t)r.lo[0] + (j - t * dx), iy = (uint32_t)r.lo[1] + t % dy, iz = (uint32_t)r.lo[2] + t / dy;
    return ix + (uint32_t)G.n[0] * (iy + (uint32_t)G.n[1] * iz);
}

// One thread per primitive.  Primitives of up to kLaneCells cells are written by their own lane; the others one after the
// other by the whole wave: ballot, the owner's range and offset through readlane, 64 pairs per step.  No lane leaves early.
__global__ void grid_emit_kernel(const float* __restrict__ bounds6, uint32_t n, GridDims G, const uint64_t* __restrict__ offset,
                                 uint32_t* __restrict__ cell, uint32_t* __restrict__ prim) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63u;
    CellRange r = {{0, 0, 0}, {0, 0, 0}};
    uint32_t cnt = 0u;
    uint64_t at = 0u;
    if (i < n) {
        r = cell_range(bounds6 + 6 * (size_t)i, G);
        cnt = cells_covered(r);
        at = offset[i];
    }
    const bool heavy = cnt > kLaneCells;
    if (!heavy)
        for (uint32_t j = 0; j < cnt; j++) { cell[at + j] = cell_of(r, j, G); prim[at + j] = i; }
    for (uint64_t todo = __ballot(heavy); todo != 0ull; todo &= todo - 1ull) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
        CellRange o;
        for (int a = 0; a < 3; a++) { o.lo[a] = __builtin_amdgcn_readlane(r.lo[a], src); o.hi[a] = __builtin_amdgcn_readlane(r.hi[a], src); }
        const uint32_t o_cnt = (uint32_t)__builtin_amdgcn_readlane((int)cnt, src), o_prim = (uint32_t)__builtin_amdgcn_readlane((int)i, src);
        const uint64_t o_at = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)at, src) |
                              ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(at >> 32), src) << 32);
        for (uint32_t j = lane; j < o_cnt; j += 64u) { cell[o_at + j] = cell_of(o, j, G); prim[o_at + j] = o_prim; }
    }
}

// cell_start[c], c = 0 .. n_cells: the first sorted pair whose cell is >= c
__global__ void grid_cell_start_kernel(const uint32_t* __restrict__ cell_sorted, uint32_t n_items, uint64_t n_cells,
                                       uint32_t* __restrict__ cell_start) {
    const uint64_t c = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c > n_cells) return;
    uint32_t lo = 0u, hi = n_items;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((uint64_t)cell_sorted[mid] < c) lo = mid + 1u; else hi = mid;
    }
    cell_start[c] = lo;
}

__global__ void grid_items_kernel(const uint32_t* __restrict__ prim_sorted, uint32_t n_items, const uint32_t* __restrict__ ref,
                                  uint32_t* __restrict__ items) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j < n_items) items[j] = ref[prim_sorted[j]];
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

struct Scratch {           // device memory freed on every path
    void* p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
};

#define GRID_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

// the one empty cell of an empty or degenerate scene: cell_start = {0, 0}, no items
hipError_t empty_grid(bool sizes_only, hipStream_t stream, GridDeviceOut& out) {
    out.n_cells = 1; out.n_items = 0;
    if (sizes_only) return hipSuccess;
    Scratch cells, items;
    GRID_TRY(hipMalloc(&cells.p, 2 * sizeof(uint32_t)));
    GRID_TRY(hipMalloc(&items.p, sizeof(uint32_t)));
    GRID_TRY(hipMemsetAsync(cells.p, 0, 2 * sizeof(uint32_t), stream));
    GRID_TRY(hipStreamSynchronize(stream));
    out.cell_start = (uint32_t*)cells.p; out.items = (uint32_t*)items.p;
    cells.p = items.p = nullptr;
    return hipSuccess;
}

}  // namespace

hipError_t build_grid_device(const float* bounds6, const uint32_t* ref, uint32_t n, bool sizes_only, hipStream_t stream,
                             GridDeviceOut& out, GridDeviceLimit* limit) {
    out = GridDeviceOut();
    *limit = kGridFits;
    // ---- 1. the bounds, and the host's shape rule
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    Scratch per_prim;        // ordered bounds (8 words) | counts [n] | offsets [n] | scan temporaries
    size_t scan_bytes = 0;
    uint64_t *count = nullptr, *offset = nullptr;
    if (n > 0) {
        GRID_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n, stream));
        const size_t head = 256, arr = ((size_t)n * sizeof(uint64_t) + 255) & ~(size_t)255;
        GRID_TRY(hipMalloc(&per_prim.p, head + 2 * arr + scan_bytes));
        uint32_t* enc = (uint32_t*)per_prim.p;
        count = (uint64_t*)((char*)per_prim.p + head); offset = (uint64_t*)((char*)per_prim.p + head + arr);
        GRID_TRY(hipMemsetAsync(enc, 0xFF, 3 * sizeof(uint32_t), stream));
        GRID_TRY(hipMemsetAsync(enc + 3, 0, 3 * sizeof(uint32_t), stream));
        hipLaunchKernelGGL(grid_bounds_kernel, dim3(std::min(blocks_for(n), kBoundsBlocks)), dim3(kThreads), 0, stream, bounds6, n, enc);
        GRID_TRY(hipGetLastError());
        uint32_t back[6];
        GRID_TRY(hipMemcpyAsync(back, enc, sizeof back, hipMemcpyDeviceToHost, stream));
        GRID_TRY(hipStreamSynchronize(stream));
        for (int a = 0; a < 3; a++) { mn[a] = unordered(back[a]); mx[a] = unordered(back[3 + a]); }
    }
    GridHost shape;
    const GridShape kind = grid_shape(n, mn, mx, shape);
    for (int a = 0; a < 3; a++) { out.n[a] = shape.n[a]; out.mn[a] = shape.mn[a]; out.mx[a] = shape.mx[a]; }
    if (kind == kGridShapeTooLarge) { *limit = kGridTooManyCells; return hipSuccess; }
    if (kind == kGridShapeEmpty) return empty_grid(sizes_only, stream, out);
    GridDims G;
    for (int a = 0; a < 3; a++) { G.n[a] = shape.n[a]; G.mn[a] = shape.mn[a]; G.mx[a] = shape.mx[a]; }
    const uint64_t n_cells = (uint64_t)G.n[0] * (uint64_t)G.n[1] * (uint64_t)G.n[2];     // <= 2^31 - 1
    out.n_cells = n_cells;

    // ---- 2, 3. ranges, counts, offsets, and the total
    hipLaunchKernelGGL(grid_count_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, stream, bounds6, n, G, count);
    GRID_TRY(hipGetLastError());
    void* scan_temp = (char*)offset + (((size_t)n * sizeof(uint64_t) + 255) & ~(size_t)255);
    GRID_TRY(hipcub::DeviceScan::ExclusiveSum(scan_temp, scan_bytes, count, offset, (int)n, stream));
    uint64_t last[2] = {0, 0};
    GRID_TRY(hipMemcpyAsync(&last[0], offset + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    GRID_TRY(hipMemcpyAsync(&last[1], count + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    GRID_TRY(hipStreamSynchronize(stream));
    const uint64_t n_items = last[0] + last[1];
    out.n_items = n_items;
    if (n_items > 0xFFFFFFFFull) { *limit = kGridTooManyItems; return hipSuccess; }
    if (sizes_only) return hipSuccess;

    // ---- the two arrays, then 4 - 6
    Scratch cells, items, pairs;
    GRID_TRY(hipMalloc(&cells.p, (size_t)(n_cells + 1) * sizeof(uint32_t)));
    GRID_TRY(hipMalloc(&items.p, (size_t)std::max<uint64_t>(n_items, 1) * sizeof(uint32_t)));
    uint32_t* cell_sorted = nullptr;
    if (n_items > 0) {
        int cell_bits = 1;
        while (cell_bits < 32 && (n_cells - 1) >> cell_bits) cell_bits++;
        size_t sort_bytes = 0;
        GRID_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                                    (uint32_t*)nullptr, (size_t)n_items, 0, cell_bits, stream));
        const size_t arr = ((size_t)n_items * sizeof(uint32_t) + 255) & ~(size_t)255;
        GRID_TRY(hipMalloc(&pairs.p, 4 * arr + sort_bytes));
        uint32_t* cell = (uint32_t*)pairs.p; uint32_t* prim = (uint32_t*)((char*)pairs.p + arr);
        cell_sorted = (uint32_t*)((char*)pairs.p + 2 * arr);
        uint32_t* prim_sorted = (uint32_t*)((char*)pairs.p + 3 * arr);
        hipLaunchKernelGGL(grid_emit_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, stream, bounds6, n, G, offset, cell, prim);
        GRID_TRY(hipGetLastError());
        GRID_TRY(hipcub::DeviceRadixSort::SortPairs((char*)pairs.p + 4 * arr, sort_bytes, cell, cell_sorted, prim, prim_sorted, (size_t)n_items, 0,
                                                    cell_bits, stream));
        hipLaunchKernelGGL(grid_items_kernel, dim3(blocks_for(n_items)), dim3(kThreads), 0, stream, prim_sorted, (uint32_t)n_items, ref,
                           (uint32_t*)items.p);
        GRID_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(grid_cell_start_kernel, dim3(blocks_for(n_cells + 1)), dim3(kThreads), 0, stream, cell_sorted, (uint32_t)n_items, n_cells,
                       (uint32_t*)cells.p);
    GRID_TRY(hipGetLastError());
    GRID_TRY(hipStreamSynchronize(stream));
    out.cell_start = (uint32_t*)cells.p; out.items = (uint32_t*)items.p;
    cells.p = items.p = nullptr;
    return hipSuccess;
}

}  // namespace p3d
