// scene_update.hip -- p3d_scene_update on the device (the "refit" half): primitives of a scene
// handle move, the tree keeps its topology and gets new boxes.  Like every tree here it only has to be CONSERVATIVE -- a
// closest hit is "nearest, lowest scene index on ties" whatever the tree -- while the primitive RECORDS have to
// be, bit for bit, what p3d_scene_create makes of the same description (scene_flatten.cpp: flatten_scene).
//
// Steps (all on the scene's stream):
//   1. one thread per updated primitive writes its record where the ray kernels read it
//   2. refit: one thread per leaf child computes the leaf's box from the records (padded primitive bounds) and climbs, one
//      arrival counter per node pair: the second arriver finds both boxes of the pair complete and carries their union up
//   3. (host: quantisation grid from the root pair's boxes) every 32-byte node pair is coded again
// Built with the ray kernels' flags: -ffp-contract=off and correctly rounded divide / sqrt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grid_builder.h"
#include "scene_bounds.h"
#include "scene_update.h"

namespace p3d {

namespace {

constexpr unsigned kThreads = 256;

__global__ void update_records_kernel(SceneRecords S, uint32_t n, const uint32_t* index, const float* prim12, uint32_t* status,
                                      float* grid_bounds) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t prim = index ? index[i] : i;
    if (prim >= S.n_prims) { atomicAdd(status + kStatusBadIndex, 1u); return; }
    const float* v = prim12 + 12 * (size_t)i;
    const uint32_t ref = S.prim_map[prim], kind = ref >> kRefKindShift, k = ref & kRefIndexMask;
    if (kind == 0u) {                                              // SphereRec
        float* r = quad(S.blob, S.off_spheres + k);
        r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3];
    } else if (kind == 1u) {                                       // triangle: p0, e1, e2 and the twice-normalised normal
        float* t = quad(S.blob, S.off_tris + S.tri_quads * k);
        float e1[3], e2[3];
        for (int a = 0; a < 3; a++) { e1[a] = v[3 + a] - v[a]; e2[a] = v[6 + a] - v[a]; }
        for (int a = 0; a < 3; a++) { t[a] = v[a]; t[4 + a] = e1[a]; t[8 + a] = e2[a]; }
        float nr[3] = {(e1[1] * e2[2]) - (e1[2] * e2[1]), (e1[2] * e2[0]) - (e1[0] * e2[2]), (e1[0] * e2[1]) - (e1[1] * e2[0])};
        for (int pass = 0; pass < 2; pass++) {
            const float l = 1.0f / sqrtf(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
            nr[0] *= l; nr[1] *= l; nr[2] *= l;
        }
        float* nq = quad(S.blob, S.off_tri_normals + k);
        nq[0] = nr[0]; nq[1] = nr[1]; nq[2] = nr[2];
    } else if (kind == 2u) {                                       // BoxRec: mn, id, mx, material
        float* b = quad(S.blob, S.off_boxes + 2u * k);
        for (int a = 0; a < 3; a++) { b[a] = v[a]; b[4 + a] = v[3 + a]; }
    } else {
        S.planes[k] = PlaneRec{v[0], v[1], v[2], v[3]};
    }
    if (grid_bounds) {                                             // GRID mode's box of the primitive (grid_builder.h), scene order
        float* g = grid_bounds + 6 * (size_t)prim;
        grid_box_rule(kind, v, g, g + 3);
    }
}

__global__ void refit_prepare_kernel(const QNode* qnodes, uint32_t n_nodes, NodePair* nodes, int32_t* parent) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const int32_t c0 = qnodes[i].child0, c1 = qnodes[i].child1;
    if (nodes) { nodes[i].child0 = c0; nodes[i].child1 = c1; nodes[i].pad0 = 0u; nodes[i].pad1 = 0u; }
    if (c0 >= 0) parent[c0] = (int32_t)i;
    if (c1 >= 0) parent[c1] = (int32_t)i;
    if (i == 0) parent[0] = -1;
}

// (padded bounds of the records: scene_bounds.h, shared with the rebuild)

// Child slot c of a node pair is six consecutive floats: lo xyz, hi xyz (p3d_device_types.h: NodePair).
__device__ __forceinline__ float* slot(NodePair* nd, int c) { return reinterpret_cast<float*>(nd) + 6 * c; }

// One thread per child slot.  Slots that hold a leaf are filled here; slots that hold an inner node by the thread that
// completes that node.  Boxes another workgroup wrote a moment ago are read past this CU's L1 (agent-scope loads) behind
// the arrival atomic; the writer fenced in front of it.  Nobody waits: the first arriver leaves.
__global__ void refit_kernel(SceneRecords S, NodePair* nodes, const int32_t* parent, uint32_t* arrived, uint32_t n_nodes, uint32_t* status) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2u * n_nodes) return;
    uint32_t cur = t >> 1;
    const int c = (int)(t & 1u);
    const int32_t child = c ? nodes[cur].child1 : nodes[cur].child0;
    if (child >= 0) return;
    Box b;
    for (int a = 0; a < 3; a++) { b.lo[a] = 3.4e38f; b.hi[a] = -3.4e38f; }
    const uint32_t ref = (uint32_t)child, form = (ref >> kLeafKindShift) & 3u;
    uint32_t held = 0;
    if (form == kLeafIndirect) {
        const uint32_t* L = S.blob + 4 * (size_t)(S.off_leaves + ~ref);          // LeafRec: tri_first, sph_first, box_first, counts
        const uint32_t nt = L[3] & 255u, ns = (L[3] >> 8) & 255u, nb = (L[3] >> 16) & 255u;
        add_tris(b, S, L[0], nt); add_spheres(b, S, L[1], ns); add_boxes(b, S, L[2], nb);
        held = nt + ns + nb;
    } else {
        const uint32_t first = ref & kLeafFirstMask, n = ((ref >> kLeafCountShift) & 15u) + 1u;
        if (form == kLeafTris) add_tris(b, S, first, n); else if (form == kLeafSpheres) add_spheres(b, S, first, n);
        held = (form == kLeafTris || form == kLeafSpheres) ? n : 0u;
    }
    if (held == 0u) {                                                // the empty leaf: an absent child keeps a NaN box
        const float nan = __uint_as_float(0x7FC00000u);
        for (int a = 0; a < 3; a++) { b.lo[a] = nan; b.hi[a] = nan; }
    }
    float* dst = slot(nodes + cur, c);
    for (int a = 0; a < 3; a++) { dst[a] = b.lo[a]; dst[3 + a] = b.hi[a]; }
    for (;;) {
        __threadfence();
        if (atomicAdd(arrived + cur, 1u) == 0u) return;              // the pair's other box is still to come
        const float* src = reinterpret_cast<const float*>(nodes + cur);
        float f[12];
        for (int x = 0; x < 12; x++) f[x] = __hip_atomic_load(src + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0u) {                                             // the root pair is complete: the tree is
            for (int x = 0; x < 12; x++) status[x] = __float_as_uint(f[x]);
            return;
        }
        const uint32_t up = (uint32_t)parent[cur];
        float* d = slot(nodes + up, nodes[up].child0 == (int32_t)cur ? 0 : 1);
        for (int a = 0; a < 3; a++) { d[a] = fminf(f[a], f[6 + a]); d[3 + a] = fmaxf(f[3 + a], f[9 + a]); }   // (NaN: the other operand)
        cur = up;
    }
}

// scene_flatten.cpp: quantise_nodes -- lo at floor - 1, hi at ceil + 1, in double against the f32 base and scale the ray
// kernels decode with; an absent child at code 0.
__global__ void requantise_kernel(const NodePair* nodes, QNode* qnodes, uint32_t n_nodes, QuantGrid G) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const float* f = reinterpret_cast<const float*>(nodes + i);
    uint32_t code[2][3];
    for (int c = 0; c < 2; c++) {
        const float* lo = f + 6 * c; const float* hi = lo + 3;
        for (int a = 0; a < 3; a++) {
            if (!(lo[0] <= hi[0])) { code[c][a] = 0u; continue; }
            const double b = G.base[a], sc = G.scale[a];
            double ql = floor(((double)lo[a] - b) / sc) - 1.0, qh = ceil(((double)hi[a] - b) / sc) + 1.0;
            ql = fmin(fmax(ql, 0.0), 65535.0); qh = fmin(fmax(qh, 0.0), 65535.0);
            code[c][a] = (uint32_t)ql | ((uint32_t)qh << 16);
        }
    }
    QNode q;
    q.x0 = code[0][0]; q.y0 = code[0][1]; q.z0 = code[0][2]; q.child0 = nodes[i].child0;
    q.x1 = code[1][0]; q.y1 = code[1][1]; q.z1 = code[1][2]; q.child1 = nodes[i].child1;
    qnodes[i] = q;
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

hipError_t launch_update_records(const SceneRecords& S, uint32_t n, const uint32_t* index, const float* prim12,
                                 uint32_t* status, float* grid_bounds, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(update_records_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, stream, S, n, index, prim12, status, grid_bounds);
    return hipGetLastError();
}

hipError_t launch_refit_prepare(const QNode* qnodes, uint32_t n_nodes, NodePair* nodes, int32_t* parent, hipStream_t stream) {
    if (n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(refit_prepare_kernel, dim3(blocks_for(n_nodes)), dim3(kThreads), 0, stream, qnodes, n_nodes, nodes, parent);
    return hipGetLastError();
}

hipError_t launch_refit(const SceneRecords& S, NodePair* nodes, const int32_t* parent, uint32_t* arrived, uint32_t n_nodes,
                        uint32_t* status, hipStream_t stream) {
    if (n_nodes == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(arrived, 0, (size_t)n_nodes * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(refit_kernel, dim3(blocks_for(2ull * n_nodes)), dim3(kThreads), 0, stream, S, nodes, parent, arrived, n_nodes, status);
    return hipGetLastError();
}

hipError_t launch_requantise(const NodePair* nodes, QNode* qnodes, uint32_t n_nodes, const QuantGrid& grid, hipStream_t stream) {
    if (n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(requantise_kernel, dim3(blocks_for(n_nodes)), dim3(kThreads), 0, stream, nodes, qnodes, n_nodes, grid);
    return hipGetLastError();
}

}  // namespace p3d
