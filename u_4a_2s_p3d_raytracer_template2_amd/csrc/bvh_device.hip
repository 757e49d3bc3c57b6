// bvh_device.hip -- BVH construction on the GPU: a linear BVH over
// Morton-sorted primitives, written straight into the scene blob in the NodePair / leaf-reference
// format the traversal kernels walk.  Replaces BVH::Build (RT/bvh.cpp:28-158) for the "load another
// scene" loop (RT/main.cpp:963-976) and for scenes whose host SAH build takes seconds (1e6 primitives:
// 1.6 s on the host).  Like the host builder's tree it only has to be CONSERVATIVE: the reference
// discards its own BVH's closest hit, so any tree over the padded primitive bounds gives
// the same image.  Its quality is below binned SAH (measured: 1e6 random primitives build in 0.08 s
// instead of 1.5 s incl. flattening and upload, and trace at 6.9 ms instead of 4.3 ms per 1080p frame);
// p3d_build_opts::builder selects it.
//
// Steps (one launch each, all on the caller's stream):
//   1. bounds of the primitive centroids                         (float min/max as ordered ints)
//   2. 63-bit Morton key per primitive, 21 bits per axis
//   3. radix sort of (key, primitive) pairs                      (hipcub::DeviceRadixSort)
//   4. leaves = runs of kLeafPrims consecutive sorted primitives: leaf reference list, leaf boxes
//   5. Karras' parallel hierarchy over the leaf keys              (HPG 2012; ties broken by index)
//   6. bottom-up box refit with one atomic counter per inner node (second arriver continues)
//   7. NodePair records (a node holds its CHILDREN's boxes), tree depth, SAH cost
// Builder 2 (p3d_build_opts::builder == 2) shares steps 1-4 and 7 and puts the clustering rounds of bvh_ploc.hip in the place
// of 5-6; when those rounds do not finish within their bound, 5-6 run after all and the tree is builder 1's.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bvh_builder.h"
#include "bvh_ploc.h"
#include "p3d_device_types.h"
#include "p3d_launch.h"

namespace p3d {

namespace {

constexpr uint32_t kLeafPrims = 2;

__device__ __forceinline__ uint32_t ordered(float f) {          // monotone float -> uint map
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

__global__ void lbvh_bounds_kernel(const BuildPrim* prims, uint32_t n, uint32_t* bounds /* lo3, hi3 as ordered */) {
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const BuildPrim p = prims[i];
        for (int a = 0; a < 3; a++) {
            const float c = 0.5f * (p.lo[a] + p.hi[a]);
            lo[a] = fminf(lo[a], c); hi[a] = fmaxf(hi[a], c);
        }
    }
    for (int a = 0; a < 3; a++) {
        for (int off = 32; off > 0; off >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; a++) {
            atomicMin(bounds + a, ordered(lo[a]));
            atomicMax(bounds + 3 + a, ordered(hi[a]));
        }
    }
}

__device__ __forceinline__ uint64_t spread21(uint32_t v) {      // 21 bits -> every third bit
    uint64_t x = v & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x1F00000000FFFFull;
    x = (x | (x << 16)) & 0x1F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

__global__ void lbvh_morton_kernel(const BuildPrim* prims, uint32_t n, const uint32_t* bounds, uint64_t* keys,
                                   uint32_t* vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BuildPrim p = prims[i];
    uint64_t key = 0;
    for (int a = 0; a < 3; a++) {
        const float lo = unordered(bounds[a]), hi = unordered(bounds[3 + a]);
        const float ext = fmaxf(hi - lo, 1e-30f);
        const float c = 0.5f * (p.lo[a] + p.hi[a]);
        float f = (c - lo) / ext * 2097152.0f;
        f = fminf(fmaxf(f, 0.0f), 2097151.0f);
        key |= spread21((uint32_t)f) << (2 - a);
    }
    keys[i] = key; vals[i] = i;
}

__global__ void lbvh_leaves_kernel(const BuildPrim* prims, uint32_t n, uint32_t n_leaves, const uint64_t* keys,
                                   const uint32_t* order, uint32_t* refs, uint64_t* leaf_keys, Box6* leaf_box) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_leaves) return;
    const uint32_t first = j * kLeafPrims, last = min(first + kLeafPrims, n);
    Box6 b;
    for (int a = 0; a < 3; a++) { b.lo[a] = 3.4e38f; b.hi[a] = -3.4e38f; }
    for (uint32_t k = first; k < last; k++) {
        const BuildPrim p = prims[order[k]];
        refs[k] = p.ref;
        for (int a = 0; a < 3; a++) { b.lo[a] = fminf(b.lo[a], p.lo[a]); b.hi[a] = fmaxf(b.hi[a], p.hi[a]); }
    }
    leaf_keys[j] = keys[first];
    leaf_box[j] = b;
}

// common-prefix length of leaf keys i and j (ties broken by the index, so all keys are distinct)
__device__ __forceinline__ int delta(const uint64_t* k, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t x = k[i] ^ k[j];
    if (x == 0) return 64 + __clz((unsigned)(i ^ j));
    return __clzll((long long)x);
}

// children: >= 0 inner node, < 0 leaf ~index.  parent_* give each node its parent inner node.
__global__ void lbvh_hierarchy_kernel(const uint64_t* k, int n_leaves, int2* children, int* parent_inner, int* parent_leaf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_leaves - 1) return;
    const int d = (delta(k, n_leaves, i, i + 1) - delta(k, n_leaves, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = delta(k, n_leaves, i, i - d);
    int lmax = 2;
    while (delta(k, n_leaves, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (delta(k, n_leaves, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(k, n_leaves, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (delta(k, n_leaves, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + min(d, 0);
    const int lo = min(i, j), hi = max(i, j);
    int2 c;
    if (lo == gamma) { c.x = ~gamma; parent_leaf[gamma] = i; } else { c.x = gamma; parent_inner[gamma] = i; }
    if (hi == gamma + 1) { c.y = ~(gamma + 1); parent_leaf[gamma + 1] = i; } else { c.y = gamma + 1; parent_inner[gamma + 1] = i; }
    children[i] = c;
    if (i == 0) parent_inner[0] = -1;
}

__device__ __forceinline__ Box6 child_box(int c, const Box6* leaf_box, const Box6* node_box) {
    return c < 0 ? leaf_box[~c] : node_box[c];
}
// the same while the refit is running: an inner node's box was written by another workgroup a moment
// ago, so it is read past this CU's L1 (a cached line may predate the write)
__device__ __forceinline__ Box6 child_box_fresh(int c, const Box6* leaf_box, const Box6* node_box) {
    if (c < 0) return leaf_box[~c];
    Box6 b;
    const float* src = reinterpret_cast<const float*>(node_box + c);
    for (int x = 0; x < 3; x++) {
        b.lo[x] = __hip_atomic_load(src + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b.hi[x] = __hip_atomic_load(src + 3 + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return b;
}

__global__ void lbvh_refit_kernel(int n_leaves, const int2* children, const int* parent_inner, const int* parent_leaf,
                                  const Box6* leaf_box, Box6* node_box, uint32_t* arrived, uint32_t* max_depth) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_leaves) return;
    int node = parent_leaf[j];
    uint32_t depth = 1;                      // levels of inner nodes above this leaf
    // boxes: the second thread to reach a node finds both children complete
    bool fitting = true;
    while (node >= 0) {
        if (fitting) {
            __threadfence();
            if (atomicAdd(arrived + node, 1u) == 0u) fitting = false;
            else {
                const int2 c = children[node];
                const Box6 a = child_box_fresh(c.x, leaf_box, node_box), b = child_box_fresh(c.y, leaf_box, node_box);
                Box6 u;
                for (int x = 0; x < 3; x++) { u.lo[x] = fminf(a.lo[x], b.lo[x]); u.hi[x] = fmaxf(a.hi[x], b.hi[x]); }
                node_box[node] = u;
            }
        }
        node = parent_inner[node];
        if (node >= 0) depth++;
    }
    atomicMax(max_depth, depth);
}

__device__ __forceinline__ float half_area(const Box6& b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx * dy + dy * dz + dz * dx;
}

__global__ void lbvh_emit_kernel(int n_leaves, uint32_t n_prims, const int2* children, const Box6* leaf_box,
                                 const Box6* node_box, NodePair* nodes, float cost_traverse, float cost_intersect,
                                 float* sah) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float cost = 0.0f;
    if (i < n_leaves - 1) {
        const int2 c = children[i];
        const Box6 a = child_box(c.x, leaf_box, node_box), b = child_box(c.y, leaf_box, node_box);
        auto leaf_code = [&](int leaf) {
            const uint32_t first = (uint32_t)leaf * kLeafPrims;
            const uint32_t cnt = min(kLeafPrims, n_prims - first);
            return (int32_t)~((first << 3) | (cnt - 1u));
        };
        NodePair nd;
        nd.lo0[0] = a.lo[0]; nd.lo0[1] = a.lo[1]; nd.lo0[2] = a.lo[2]; nd.hi0x = a.hi[0];
        nd.hi0yz[0] = a.hi[1]; nd.hi0yz[1] = a.hi[2]; nd.lo1xy[0] = b.lo[0]; nd.lo1xy[1] = b.lo[1];
        nd.lo1z = b.lo[2]; nd.hi1[0] = b.hi[0]; nd.hi1[1] = b.hi[1]; nd.hi1[2] = b.hi[2];
        nd.child0 = c.x < 0 ? leaf_code(~c.x) : c.x;
        nd.child1 = c.y < 0 ? leaf_code(~c.y) : c.y;
        nd.pad0 = 0; nd.pad1 = 0;
        nodes[i] = nd;
        // SAH cost in the host builder's units: node visits + primitive tests, area-weighted
        const float root = fmaxf(half_area(node_box[0]), 1e-30f);
        cost = cost_traverse * half_area(node_box[i]) / root;
        if (c.x < 0) cost += cost_intersect * (float)((~nd.child0 & 7) + 1) * half_area(a) / root;
        if (c.y < 0) cost += cost_intersect * (float)((~nd.child1 & 7) + 1) * half_area(b) / root;
    }
    for (int off = 32; off > 0; off >>= 1) cost += __shfl_xor(cost, off);
    if ((threadIdx.x & 63) == 0 && cost != 0.0f) atomicAdd(sah, cost);
}

}  // namespace

// The scratch a build of n primitives carves out of one allocation (after the caller's own `head` bytes).
struct LbvhLayout {
    size_t keys, keys2, vals, vals2, lkeys, lbox, nbox, child, pin, pleaf, arr, misc, sort, sort_bytes, total;
};
static hipError_t lbvh_layout(uint32_t n, size_t head, LbvhLayout& Y, hipStream_t stream) {
    const uint32_t L = (n + kLeafPrims - 1) / kLeafPrims;
    size_t off = head;
    auto carve = [&](size_t bytes) { size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return at; };
    Y.keys = carve((size_t)n * 8); Y.keys2 = carve((size_t)n * 8);
    Y.vals = carve((size_t)n * 4); Y.vals2 = carve((size_t)n * 4);
    Y.lkeys = carve((size_t)L * 8); Y.lbox = carve((size_t)L * sizeof(Box6)); Y.nbox = carve((size_t)L * sizeof(Box6));
    Y.child = carve((size_t)L * 8); Y.pin = carve((size_t)L * 4); Y.pleaf = carve((size_t)L * 4);
    Y.arr = carve((size_t)L * 4); Y.misc = carve(64);
    Y.sort_bytes = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, Y.sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                      (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 63, stream);
    if (e != hipSuccess) return e;
    Y.sort = carve(Y.sort_bytes);
    Y.total = off;
    return hipSuccess;
}

hipError_t lbvh_scratch_bytes(uint32_t n, size_t* bytes, hipStream_t stream) {
    LbvhLayout Y;
    hipError_t e = lbvh_layout(n, 0, Y, stream);
    if (e == hipSuccess) *bytes = Y.total;
    return e;
}

// The build itself over `d_prims` (device array, padded bounds), enqueued on `stream`: nodes[n_leaves - 1], refs[n].
// `pool` is the allocation Y was laid out for; it must live until the stream has passed.  The tree's depth (levels of
// inner nodes) and SAH cost are left in the two words at *d_result.
struct LbvhArrays {
    uint64_t *keys, *keys2, *lkeys;
    uint32_t *vals, *vals2, *arrived, *misc;              // misc: bounds[6], depth, sah
    Box6 *lbox, *nbox;
    int2* child;
    int *pin, *pleaf;
    LbvhArrays(char* pool, const LbvhLayout& Y)
        : keys((uint64_t*)(pool + Y.keys)), keys2((uint64_t*)(pool + Y.keys2)), lkeys((uint64_t*)(pool + Y.lkeys)),
          vals((uint32_t*)(pool + Y.vals)), vals2((uint32_t*)(pool + Y.vals2)), arrived((uint32_t*)(pool + Y.arr)),
          misc((uint32_t*)(pool + Y.misc)), lbox((Box6*)(pool + Y.lbox)), nbox((Box6*)(pool + Y.nbox)), child((int2*)(pool + Y.child)),
          pin((int*)(pool + Y.pin)), pleaf((int*)(pool + Y.pleaf)) {}
};
constexpr unsigned T = 256;

// steps 1-4: sorted references in d_refs, leaf keys and leaf boxes in the scratch
static hipError_t lbvh_enqueue_leaves(const BuildPrim* d_prims, uint32_t n, uint32_t* d_refs, char* pool, const LbvhLayout& Y, hipStream_t stream) {
    const uint32_t L = (n + kLeafPrims - 1) / kLeafPrims;
    const LbvhArrays A(pool, Y);
    hipError_t e;
    const uint32_t init[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u};
    if ((e = hipMemcpyAsync(A.misc, init, sizeof init, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(A.arrived, 0, (size_t)L * 4, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(lbvh_bounds_kernel, dim3(std::min<unsigned>((n + T - 1) / T, 2048)), dim3(T), 0, stream, d_prims, n, A.misc);
    hipLaunchKernelGGL(lbvh_morton_kernel, dim3((n + T - 1) / T), dim3(T), 0, stream, d_prims, n, A.misc, A.keys, A.vals);
    size_t sort_bytes = Y.sort_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(pool + Y.sort, sort_bytes, A.keys, A.keys2, A.vals, A.vals2, (int)n, 0, 63, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lbvh_leaves_kernel, dim3((L + T - 1) / T), dim3(T), 0, stream, d_prims, n, L, A.keys2, A.vals2, d_refs, A.lkeys, A.lbox);
    return hipGetLastError();
}
// steps 5-6: Karras' hierarchy and the refit
static hipError_t lbvh_enqueue_hierarchy(uint32_t n, char* pool, const LbvhLayout& Y, hipStream_t stream) {
    const uint32_t L = (n + kLeafPrims - 1) / kLeafPrims;
    const LbvhArrays A(pool, Y);
    hipLaunchKernelGGL(lbvh_hierarchy_kernel, dim3((L + T - 1) / T), dim3(T), 0, stream, A.lkeys, (int)L, A.child, A.pin, A.pleaf);
    hipLaunchKernelGGL(lbvh_refit_kernel, dim3((L + T - 1) / T), dim3(T), 0, stream, (int)L, A.child, A.pin, A.pleaf, A.lbox, A.nbox, A.arrived, A.misc + 6);
    return hipGetLastError();
}
// step 7
static hipError_t lbvh_enqueue_emit(uint32_t n, const BvhOptions& opt, NodePair* d_nodes, char* pool, const LbvhLayout& Y,
                                    uint32_t** d_result, hipStream_t stream) {
    const uint32_t L = (n + kLeafPrims - 1) / kLeafPrims;
    const LbvhArrays A(pool, Y);
    hipLaunchKernelGGL(lbvh_emit_kernel, dim3((L + T - 1) / T), dim3(T), 0, stream, (int)L, n, A.child, A.lbox, A.nbox, d_nodes,
                       opt.cost_traverse, opt.cost_intersect, (float*)(A.misc + 7));
    *d_result = A.misc + 6;
    return hipGetLastError();
}

// The build itself over `d_prims` (device array, padded bounds), enqueued on `stream`: nodes[n_leaves - 1], refs[n].
// `pool` is the allocation Y was laid out for; it must live until the stream has passed.  The tree's depth (levels of
// inner nodes) and SAH cost are left in the two words at *d_result.
static hipError_t lbvh_enqueue_at(const BuildPrim* d_prims, uint32_t n, const BvhOptions& opt, NodePair* d_nodes, uint32_t* d_refs,
                                  char* pool, const LbvhLayout& Y, uint32_t** d_result, hipStream_t stream) {
    hipError_t e;
    if ((e = lbvh_enqueue_leaves(d_prims, n, d_refs, pool, Y, stream)) != hipSuccess) return e;
    if ((e = lbvh_enqueue_hierarchy(n, pool, Y, stream)) != hipSuccess) return e;
    return lbvh_enqueue_emit(n, opt, d_nodes, pool, Y, d_result, stream);
}
// Builder 2: the clustered hierarchy between the same leaves and the same emit step.  Waits on the stream once per round
// (bvh_ploc.h).  `ploc_pool` holds ploc_cluster_scratch_bytes(n_leaves) bytes.  info = {rounds, fell_back}.
static hipError_t ploc_enqueue_at(const BuildPrim* d_prims, uint32_t n, const BvhOptions& opt, NodePair* d_nodes, uint32_t* d_refs,
                                  char* pool, const LbvhLayout& Y, char* ploc_pool, uint32_t** d_result, PlocInfo* info, hipStream_t stream) {
    const uint32_t L = (n + kLeafPrims - 1) / kLeafPrims;
    const LbvhArrays A(pool, Y);
    hipError_t e;
    if ((e = lbvh_enqueue_leaves(d_prims, n, d_refs, pool, Y, stream)) != hipSuccess) return e;
    int rounds = 0;
    bool finished = false;
    if ((e = ploc_cluster(A.lbox, L, A.child, A.nbox, A.misc + 6, ploc_pool, &rounds, &finished, stream)) != hipSuccess) return e;
    if (!finished && (e = lbvh_enqueue_hierarchy(n, pool, Y, stream)) != hipSuccess) return e;
    if (info) { info->rounds = rounds; info->fell_back = finished ? 0 : 1; }
    return lbvh_enqueue_emit(n, opt, d_nodes, pool, Y, d_result, stream);
}

hipError_t lbvh_enqueue(const BuildPrim* d_prims, uint32_t n, const BvhOptions& opt, NodePair* d_nodes, uint32_t* d_refs,
                        void* scratch, uint32_t** d_result, hipStream_t stream) {
    LbvhLayout Y;
    hipError_t e = lbvh_layout(n, 0, Y, stream);
    if (e != hipSuccess) return e;
    return lbvh_enqueue_at(d_prims, n, opt, d_nodes, d_refs, (char*)scratch, Y, d_result, stream);
}

// the two halves of builder 2's scratch: builder 1's layout, then that of the clustering rounds
static hipError_t ploc_layout_both(uint32_t n, size_t head, LbvhLayout& Y, size_t* ploc_at, size_t* total, hipStream_t stream) {
    hipError_t e = lbvh_layout(n, head, Y, stream);
    if (e != hipSuccess) return e;
    size_t bytes = 0;
    if ((e = ploc_cluster_scratch_bytes((n + kLeafPrims - 1) / kLeafPrims, &bytes, stream)) != hipSuccess) return e;
    *ploc_at = Y.total;
    *total = Y.total + bytes;
    return hipSuccess;
}

hipError_t ploc_scratch_bytes(uint32_t n, size_t* bytes, hipStream_t stream) {
    LbvhLayout Y;
    size_t at = 0;
    return ploc_layout_both(n, 0, Y, &at, bytes, stream);
}

hipError_t ploc_enqueue(const BuildPrim* d_prims, uint32_t n, const BvhOptions& opt, NodePair* d_nodes, uint32_t* d_refs,
                        void* scratch, uint32_t** d_result, PlocInfo* info, hipStream_t stream) {
    LbvhLayout Y;
    size_t at = 0, total = 0;
    hipError_t e = ploc_layout_both(n, 0, Y, &at, &total, stream);
    if (e != hipSuccess) return e;
    return ploc_enqueue_at(d_prims, n, opt, d_nodes, d_refs, (char*)scratch, Y, (char*)scratch + at, d_result, info, stream);
}

void lbvh_stats(uint32_t n, const uint32_t result[2], BvhStats& stats) {
    const uint32_t L = (n + kLeafPrims - 1) / kLeafPrims;
    stats = BvhStats();
    stats.n_nodes = L - 1; stats.n_leaves = L; stats.n_leaf_refs = n;
    stats.max_depth = result[0] + 1;          // + the leaf level, like the host builder's count
    memcpy(&stats.sah_cost, &result[1], 4);
}

// Builds the tree of `prims` (host array, padded bounds) into device memory: nodes[n_leaves - 1],
// refs[n].  n >= 2 * kLeafPrims.  Synchronous (returns when the tree is complete).  builder 1: the LBVH; 2: the clustered
// tree, *info telling how many rounds it took and whether the LBVH was made after all.
hipError_t build_bvh_device(uint32_t builder, const std::vector<BuildPrim>& prims, const BvhOptions& opt, NodePair* d_nodes,
                            uint32_t* d_refs, BvhStats& stats, PlocInfo* info, hipStream_t stream) {
    const uint32_t n = (uint32_t)prims.size();
    hipError_t e;
    char* pool = nullptr;
    // one scratch allocation, carved up: the uploaded primitives lead it
    LbvhLayout Y;
    const size_t head = ((size_t)n * sizeof(BuildPrim) + 255) & ~(size_t)255;
    size_t ploc_at = 0, total = 0;
    if (builder == 2) e = ploc_layout_both(n, head, Y, &ploc_at, &total, stream);
    else { e = lbvh_layout(n, head, Y, stream); total = Y.total; }
    if (e != hipSuccess) return e;
    if ((e = hipMalloc((void**)&pool, total)) != hipSuccess) return e;
    auto done = [&](hipError_t rc) { (void)hipFree(pool); return rc; };
    BuildPrim* d_prims = (BuildPrim*)pool;
    if ((e = hipMemcpyAsync(d_prims, prims.data(), (size_t)n * sizeof(BuildPrim), hipMemcpyHostToDevice, stream)) != hipSuccess) return done(e);
    uint32_t* d_result = nullptr;
    if (info) *info = PlocInfo();
    if (builder == 2) e = ploc_enqueue_at(d_prims, n, opt, d_nodes, d_refs, pool, Y, pool + ploc_at, &d_result, info, stream);
    else e = lbvh_enqueue_at(d_prims, n, opt, d_nodes, d_refs, pool, Y, &d_result, stream);
    if (e != hipSuccess) return done(e);
    uint32_t back[2];
    if ((e = hipMemcpyAsync(back, d_result, sizeof back, hipMemcpyDeviceToHost, stream)) != hipSuccess) return done(e);
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return done(e);
    lbvh_stats(n, back, stats);
    return done(hipSuccess);
}

hipError_t build_lbvh_device(const std::vector<BuildPrim>& prims, const BvhOptions& opt, NodePair* d_nodes,
                             uint32_t* d_refs, BvhStats& stats, hipStream_t stream) {
    return build_bvh_device(1, prims, opt, d_nodes, d_refs, stats, nullptr, stream);
}

// ------------------------------------------------------------------ tile order of the persistent tile schedule
// "Heaviest first": tiles sorted by the duration the previous frames measured for them (p3d_kernels.hip: wf_tile_kernel
// writes LaunchParams::tile_cost).  Persistent workgroups that draw tiles in that order finish together; drawn row by row,
// the expensive tiles of a frame are started late and the launch ends with a few workgroups still on them (dragon: 1.29 ms
// against 0.76 for the same tile durations list-scheduled heaviest first, profiles/r03_tile_timeline.txt).
__global__ void iota_kernel(uint32_t* v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}
// temp_bytes == 0: only reports the temporary storage the sort needs
hipError_t sort_tiles_by_cost(const uint32_t* cost, uint32_t* cost_sorted, uint32_t* iota, uint32_t* order, uint32_t n,
                              void* temp, size_t& temp_bytes, hipStream_t stream) {
    if (temp == nullptr)
        return hipcub::DeviceRadixSort::SortPairsDescending(nullptr, temp_bytes, cost, cost_sorted, iota, order, (int)n, 0, 32, stream);
    hipLaunchKernelGGL(iota_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, iota, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortPairsDescending(temp, temp_bytes, cost, cost_sorted, iota, order, (int)n, 0, 32, stream);
}

}  // namespace p3d
