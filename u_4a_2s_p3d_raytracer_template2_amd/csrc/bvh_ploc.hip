// bvh_ploc.hip -- the hierarchy of device builder 2 (p3d_build_opts::builder == 2): parallel locally-ordered clustering
// (Meister & Bittner, "Parallel Locally-Ordered Clustering for Bounding Volume Hierarchy Construction", TVCG 2017) over
// the Morton-sorted leaves bvh_device.hip makes for builder 1.  It replaces Karras' hierarchy and the refit (steps 5-6
// there); the leaves before it and the emit step after it are builder 1's.
//
// The live clusters sit in slots 0 .. m-1 of an array, at first the L leaves in sorted order.  A cluster is its box, its
// child code (~leaf, or the node index of a merged cluster) and its inner depth (inner nodes on the longest path below it;
// a leaf has 0).  One round:
//   1. nearest neighbour   nn[i] = the j in [i - R, i + R] (inside the array, j != i) whose union with i has the least
//                          half_area(), the lowest such j on ties.  The union is fminf / fmaxf, so d(i, j) and d(j, i)
//                          are the same bits.
//   2. merge               slots with nn[nn[i]] == i and i < nn[i]: a new node with child0 = slot i's cluster and child1 =
//                          slot nn[i]'s; its box is their union, its depth the larger of theirs + 1.  It stays in slot i,
//                          slot nn[i] dies.
//   3. numbering           downwards, so that the root is node 0: `next` starts at L - 1; a round of k merges gives the
//                          merge of rank r (in slot order) the index next - k + r, and next -= k.
//   4. compaction          of the live slots, order kept.
// The lowest slot of a pair at the least distance always finds its partner pointing back, so every round merges.  Launches
// per round: neighbours, flags, one exclusive scan of (live, merges) packed into 64 bits, merge + compaction; the host reads
// k back (4 bytes) and waits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "bvh_ploc.h"

namespace p3d {

namespace {

constexpr int R = kPlocRadius;
constexpr int kBlock = 256;
constexpr uint64_t kLive = 1ull << 32;          // a slot's flags: live in the high word, merges in the low one

__global__ void ploc_init_kernel(const Box6* leaf_box, int n_leaves, Box6* box, int* code, int* depth) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_leaves) return;
    box[i] = leaf_box[i]; code[i] = ~i; depth[i] = 0;
}

// One thread per slot.  The workgroup's 256 + 2R boxes are staged in LDS component by component ((256 + 2R) * 24 B =
// 6.4 KiB; consecutive lanes read consecutive dwords), the halo clamped at the array's ends.
__global__ __launch_bounds__(kBlock) void ploc_nn_kernel(const Box6* box, int m, int* nn) {
    __shared__ float tile[6][kBlock + 2 * R];
    const int base = (int)blockIdx.x * kBlock - R;
    for (int t = threadIdx.x; t < kBlock + 2 * R; t += kBlock) {
        const Box6 b = box[min(max(base + t, 0), m - 1)];
        for (int a = 0; a < 3; a++) { tile[a][t] = b.lo[a]; tile[3 + a][t] = b.hi[a]; }
    }
    __syncthreads();
    const int i = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (i >= m) return;
    const int li = (int)threadIdx.x + R;
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = tile[a][li]; hi[a] = tile[3 + a][li]; }
    float best = 0.0f;
    int best_j = -1;
#pragma unroll
    for (int off = -R; off <= R; off++) {            // ascending j and a strict comparison: the lowest j wins a tie
        if (off == 0) continue;
        const int j = i + off;
        if (j < 0 || j >= m) continue;
        const float dx = fmaxf(hi[0], tile[3][li + off]) - fminf(lo[0], tile[0][li + off]);
        const float dy = fmaxf(hi[1], tile[4][li + off]) - fminf(lo[1], tile[1][li + off]);
        const float dz = fmaxf(hi[2], tile[5][li + off]) - fminf(lo[2], tile[2][li + off]);
        const float d = dx * dy + dy * dz + dz * dx;
        if (best_j < 0 || d < best) { best = d; best_j = j; }
    }
    nn[i] = best_j;
}

__global__ void ploc_flags_kernel(const int* nn, int m, uint64_t* flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int j = nn[i];
    const bool paired = nn[j] == i;
    flags[i] = (paired && j < i) ? 0ull : (kLive | (paired ? 1ull : 0ull));
}

// scan[i] = (live slots before i) << 32 | merges before i.  The merged or kept cluster of live slot i goes to the slot of
// its rank.  The thread of the last slot leaves k, the number of merges of the round, in *k_out.
__global__ void ploc_merge_kernel(int m, int next, const int* nn, const uint64_t* flags, const uint64_t* scan, const Box6* box,
                                  const int* code, const int* depth, Box6* box_out, int* code_out, int* depth_out, int2* children,
                                  Box6* node_box, uint32_t* k_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int k = (int)(uint32_t)(scan[m - 1] + flags[m - 1]);
    if (i == m - 1) *k_out = (uint32_t)k;
    const uint64_t f = flags[i], s = scan[i];
    if (!(f & kLive)) return;
    const int pos = (int)(s >> 32);
    if (f & 1ull) {
        const int j = nn[i], node = next - k + (int)(uint32_t)s;
        const Box6 a = box[i], b = box[j];
        Box6 u;
        for (int x = 0; x < 3; x++) { u.lo[x] = fminf(a.lo[x], b.lo[x]); u.hi[x] = fmaxf(a.hi[x], b.hi[x]); }
        children[node] = make_int2(code[i], code[j]);
        node_box[node] = u;
        box_out[pos] = u; code_out[pos] = node; depth_out[pos] = max(depth[i], depth[j]) + 1;
    } else {
        box_out[pos] = box[i]; code_out[pos] = code[i]; depth_out[pos] = depth[i];
    }
}

struct PlocLayout { size_t box[2], code[2], depth[2], nn, flags, scan, word, temp, temp_bytes, total; };

hipError_t ploc_layout(uint32_t L, PlocLayout& Y, hipStream_t stream) {
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return at; };
    for (int s = 0; s < 2; s++) { Y.box[s] = carve((size_t)L * sizeof(Box6)); Y.code[s] = carve((size_t)L * 4); Y.depth[s] = carve((size_t)L * 4); }
    Y.nn = carve((size_t)L * 4); Y.flags = carve((size_t)L * 8); Y.scan = carve((size_t)L * 8); Y.word = carve(64);
    Y.temp_bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, Y.temp_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)L, stream);
    if (e != hipSuccess) return e;
    Y.temp = carve(Y.temp_bytes);
    Y.total = off;
    return hipSuccess;
}

}  // namespace

hipError_t ploc_cluster_scratch_bytes(uint32_t n_leaves, size_t* bytes, hipStream_t stream) {
    PlocLayout Y;
    hipError_t e = ploc_layout(n_leaves, Y, stream);
    if (e == hipSuccess) *bytes = Y.total;
    return e;
}

hipError_t ploc_cluster(const Box6* leaf_box, uint32_t n_leaves, int2* children, Box6* node_box, uint32_t* d_root_depth,
                        void* scratch, int* rounds, bool* finished, hipStream_t stream) {
    PlocLayout Y;
    hipError_t e = ploc_layout(n_leaves, Y, stream);
    if (e != hipSuccess) return e;
    char* pool = (char*)scratch;
    Box6* box[2] = {(Box6*)(pool + Y.box[0]), (Box6*)(pool + Y.box[1])};
    int* code[2] = {(int*)(pool + Y.code[0]), (int*)(pool + Y.code[1])};
    int* depth[2] = {(int*)(pool + Y.depth[0]), (int*)(pool + Y.depth[1])};
    int* nn = (int*)(pool + Y.nn);
    uint64_t *flags = (uint64_t*)(pool + Y.flags), *scan = (uint64_t*)(pool + Y.scan);
    uint32_t* k_word = (uint32_t*)(pool + Y.word);
    auto blocks = [](int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); };
    int m = (int)n_leaves, next = (int)n_leaves - 1, cur = 0;
    *rounds = 0; *finished = false;
    hipLaunchKernelGGL(ploc_init_kernel, blocks(m), dim3(kBlock), 0, stream, leaf_box, m, box[0], code[0], depth[0]);
    while (m > 1 && *rounds < kPlocMaxRounds) {
        hipLaunchKernelGGL(ploc_nn_kernel, blocks(m), dim3(kBlock), 0, stream, box[cur], m, nn);
        hipLaunchKernelGGL(ploc_flags_kernel, blocks(m), dim3(kBlock), 0, stream, nn, m, flags);
        size_t temp_bytes = Y.temp_bytes;
        if ((e = hipcub::DeviceScan::ExclusiveSum(pool + Y.temp, temp_bytes, flags, scan, m, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(ploc_merge_kernel, blocks(m), dim3(kBlock), 0, stream, m, next, nn, flags, scan, box[cur], code[cur], depth[cur],
                           box[cur ^ 1], code[cur ^ 1], depth[cur ^ 1], children, node_box, k_word);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        uint32_t k = 0;
        if ((e = hipMemcpyAsync(&k, k_word, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        if (k == 0 || k > (uint32_t)next) return hipErrorUnknown;         // (never: see the head of this file)
        next -= (int)k; m -= (int)k; cur ^= 1;
        ++*rounds;
    }
    if (m > 1) return hipSuccess;
    *finished = true;
    return hipMemcpyAsync(d_root_depth, depth[cur], 4, hipMemcpyDeviceToDevice, stream);
}

}  // namespace p3d
