// p3d_kernels.hip -- gfx950 (MI355X / CDNA4) kernels of the Whitted hot path.
//
// Two schedules of the same per-node code (p3d_shade.h), bit-identical results:
//
//  * WAVEFRONT (default).  The reference's recursion rayTracing() (RT/main.cpp:530-721) is
//    unrolled by tree level: one launch per level traces one ray per lane; nodes that spawn
//    children are parked as 48-byte NodeRec, their child rays are compacted into the next
//    level's queue with wave ballot + mbcnt prefix sums (one atomic per wave), and resolve
//    launches walk the levels back up combining children into parents in the reference's
//    post-order arithmetic (the last level combines sibling pairs with their parent itself:
//    combine_pair).  Every launch is short and uniform: no lane waits for a
//    neighbour's deeper tree, there is no per-lane recursion stack, and the only LDS use is the
//    BVH traversal stack.
//  * TREE (P3D_FLAG_TREE_KERNEL, and the fallback when the worst-case queues would not fit):
//    one launch, each lane walks its pixel's whole tree with an explicit post-order frame
//    stack in LDS.
//
// A wave owns a 16x4 pixel tile; the blockIdx -> tile map hands chunks of tiles to XCDs.
// Numerics: compiled with -ffp-contract=off, no fast-math; see p3d_device_math.h.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "p3d_device_types.h"
#include "p3d_launch.h"
#include "p3d_shade.h"
#include "p3d_scene_view.h"
#include "p3d_tile_coverage.h"

namespace p3d {

// ------------------------------------------------------------------ common helpers
__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {          // # set bits below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// the scene id a frame's hit_id plane records for a primary hit (-1: the ray left the scene)
__device__ __forceinline__ int32_t hit_id_of(const Hit& h) { return (h.ref == 0xFFFFFFFFu) ? -1 : (int32_t)h.sid; }
// "color / (4 * 4)" of the anti-aliased path (RT/main.cpp:800)
__device__ __forceinline__ V3 div16(V3 c) { return mk(fdiv(c.x, 16.0f), fdiv(c.y, 16.0f), fdiv(c.z, 16.0f)); }

// The AOV planes of compact pixel p (p3d_render_aov: LaunchParams::aov_*), written where hit_id is, from the primary ray and
// its closest hit.  Only the AOV = true builds of the kernels call it (p3d_kernel_variant.h: has_aov): a frame without planes
// runs the builds without, which hold none of this.  Each plane is one wave-uniform test of its pointer.  The normal is
// computed for lanes with a hit only, by the helper a ray stream's level 1 uses (wf_rays_kernel), so the two entries agree in
// every bit; the albedo is the diffuse rgb of the hit's material record as the scene description gave it.  Per lane one
// 4-byte and two 12-byte stores: the 16 lanes of a tile row write 64 / 192 consecutive bytes per plane.  No atomics, no LDS.
template <class SV>
__device__ __forceinline__ void write_aov(const LaunchParams& P, const SV& sv, size_t p, bool valid, const Ray& ray, const Hit& h) {
    const bool hit = valid && h.ref != 0xFFFFFFFFu;
    if (valid && P.aov_depth) P.aov_depth[p] = hit ? h.t : __builtin_inff();
    if (P.aov_normal) {                                      // getNormal(hit point).normalize(), RT/main.cpp:587-589
        V3 n = mk(0.0f, 0.0f, 0.0f);
        if (hit) n = prim_normal(P, sv, h.ref, ray, add(ray.o, mul(ray.d, h.t)));
        if (valid) { float* pn = P.aov_normal + 3 * p; pn[0] = n.x; pn[1] = n.y; pn[2] = n.z; }
    }
    if (P.aov_albedo) {                                      // Material::GetDiffColor(), RT/scene.h:23-55: not multiplied by Kd
        V3 a = mk(0.0f, 0.0f, 0.0f);
        if (hit) a = load_material(sv, h.mat).diff;
        if (valid) { float* pa = P.aov_albedo + 3 * p; pa[0] = a.x; pa[1] = a.y; pa[2] = a.z; }
    }
}

template <bool COUNT>
__device__ __forceinline__ void flush_counters(const LaunchParams& P, const Ctr& ctr, uint32_t pixels) {
    if (COUNT) {
        DeviceCounters* c = P.counters;
        atomicAdd(&c->closest_queries, (unsigned long long)ctr.closest);
        atomicAdd(&c->shadow_queries, (unsigned long long)ctr.shadow);
        atomicAdd(&c->box_tests, (unsigned long long)ctr.box);
        atomicAdd(&c->sphere_tests, (unsigned long long)ctr.sph);
        atomicAdd(&c->tri_tests, (unsigned long long)ctr.tri);
        atomicAdd(&c->aabox_tests, (unsigned long long)ctr.aab);
        atomicAdd(&c->plane_tests, (unsigned long long)ctr.pln);
        atomicAdd(&c->pixels, (unsigned long long)pixels);
    }
}

// img_Data / colors of RT/main.cpp:803-815 for compact pixel p
__device__ __forceinline__ void write_pixel(const LaunchParams& P, size_t p, V3 color) {
    if (P.rgb8) {
        P.rgb8[3 * p] = (uint8_t)u8fromfloat(color.x);
        P.rgb8[3 * p + 1] = (uint8_t)u8fromfloat(color.y);
        P.rgb8[3 * p + 2] = (uint8_t)u8fromfloat(color.z);
    }
    if (P.rgb32f) { P.rgb32f[3 * p] = color.x; P.rgb32f[3 * p + 1] = color.y; P.rgb32f[3 * p + 2] = color.z; }
}

// One finished primary-ray tree: "rayTracing(...).clamp()", summed over samples and divided
// by 4*4 in the anti-aliased path (RT/main.cpp:774,797-800).
// In the anti-aliased path every sample pass writes its clamped colours to its own plane (so that the
// passes of a frame can run concurrently) and sum_samples_kernel adds the planes in sample order.
__device__ __forceinline__ void sink_sample(const LaunchParams& P, size_t p, V3 ret) {
    V3 c = clampc(ret);
    if (P.wf_nsamples <= 1 && P.spp == 0) { write_pixel(P, p, c); return; }
    float* a = P.wf_planes + (size_t)P.wf_sample * P.wf_plane_stride + 3 * p;
    a[0] = c.x; a[1] = c.y; a[2] = c.z;
}

// One finished ray of a ray stream (p3d_trace_rays): what rayTracing(ray, 1, 1.0) returns, as it is -- no clamp, no image.
__device__ __forceinline__ void sink_ray(const LaunchParams& P, size_t i, V3 ret) {
    if (P.rgb32f) { P.rgb32f[3 * i] = ret.x; P.rgb32f[3 * i + 1] = ret.y; P.rgb32f[3 * i + 2] = ret.z; }
}

// row of the compact local buffer -> image row (this rank's row blocks are every world-th one)
__device__ __forceinline__ int image_row(const LaunchParams& P, int row) {
    const int blk = P.row_block_shift >= 0 ? (row >> P.row_block_shift) : row / P.row_block;
    return (blk * P.world + P.rank) * P.row_block + (row - blk * P.row_block);
}

// "color += rayTracing(...).clamp()" over the samples in order, then "color / (4 * 4)"
// (RT/main.cpp:797-800), for the rows [row0, row0 + rows) of the compact buffer
template <bool BATCH>
__global__ __launch_bounds__(256) void sum_samples_kernel(const LaunchParams P, size_t first_px, size_t n_px) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_px; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = first_px + i;
        // rows past the image (the compact buffer is padded to whole row blocks) are never written:
        // a caller's device plane only holds res_y rows when world == 1 (include/p3d_hip.h)
        int row = (int)(p / (size_t)P.res_x);
        if (BATCH) row %= P.out_rows;                    // (a batch: p counts out_rows rows per frame)
        if (image_row(P, row) >= P.res_y) continue;
        V3 acc = mk(0.0f, 0.0f, 0.0f);
        for (int smp = 0; smp < P.wf_nsamples; smp++) {
            const float* a = P.wf_planes + (size_t)smp * P.wf_plane_stride + 3 * p;
            acc = add(acc, mk(a[0], a[1], a[2]));
        }
        write_pixel(P, p, div16(acc));
    }
}

// Frame batches (LaunchParams::n_frames) are compiled into their own kernel instantiations (BATCH = true); BATCH = false
// is the one-frame code unchanged.
// Frame of a batch that the tile row starting at stacked compact row `row0` belongs to (0 for one frame).  row0 is
// wave-uniform: the division runs once per wave, on the scalar unit.
template <bool BATCH>
__device__ __forceinline__ int batch_frame(const LaunchParams& P, int row0) {
    return BATCH ? __builtin_amdgcn_readfirstlane(row0 / P.frame_rows) : 0;
}
// stacked compact row of frame f -> row of the caller's planes (frame f starts out_rows rows in)
template <bool BATCH>
__device__ __forceinline__ int out_row(const LaunchParams& P, int f, int row) {
    return BATCH ? row + f * (P.out_rows - P.frame_rows) : row;
}

// tile -> pixel.  Returns false for lanes outside the image.  row = the stacked compact row; f = the batch frame;
// y = the image row inside frame f.
template <bool ORDERED = false, bool BATCH = false>
__device__ __forceinline__ bool tile_pixel(const LaunchParams& P, int& x, int& y, int& row, int& f, int* tile_out = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = 0; y = 0; row = 0; f = 0;
    int tx, ty, tile;
    if (!ORDERED && gridDim.y > 1) {
        // 2-D launch (identity tile map, xcd_chunk == 1): blockIdx.x / .y ARE the tile's column and row -- no division by
        // launch parameters on the scalar unit (three of them cost this kernel ~60 of its ~350 scalar instructions per wave)
        tx = blockIdx.x; ty = blockIdx.y;
        tile = ty * P.tiles_x + tx;
        if (tile_out) *tile_out = tile;
        ty += P.wf_tile_row0;
    } else {
        // XCD-aware tile map.  Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8
        // share one, each XCD has its own L2), so XCD k is given CHUNKS of xcd_chunk consecutive
        // tiles: chunk c goes to XCD c % 8.  xcd_chunk = 1 is the identity map (best load balance),
        // larger chunks trade balance for L2 locality on scenes whose BVH does not fit one L2.
        const int bid = blockIdx.x;
        const int j = bid >> 3;
        tile = P.xcd_chunk == 1 ? bid : ((j / P.xcd_chunk) * 8 + (bid & 7)) * P.xcd_chunk + (j % P.xcd_chunk);
        if (tile_out) *tile_out = tile;
        if (tile >= P.n_tiles) return false;
        if (ORDERED && P.tile_order) {            // heaviest first (scenes read from HBM, once a frame has measured the tiles)
            tile = (int)P.tile_order[tile];
            if (tile_out) *tile_out = tile;
        }
        tx = tile % P.tiles_x; ty = P.wf_tile_row0 + tile / P.tiles_x;
    }
    x = tx * 16 + (lane & 15);
    const int row0 = ty * (P.wg_waves * 4);
    row = row0 + (lane >> 4) + wave * 4;                          // row in the compact local buffer
    f = batch_frame<BATCH>(P, row0);
    y = image_row(P, BATCH ? row - f * P.frame_rows : row);
    return x < P.res_x && y < P.res_y;
}
// The 2-D launch's branch of tile_pixel() for a tile the caller names: column tx, row ty of the band (one frame, LDS scenes).
__device__ __forceinline__ bool tile_pixel_at(const LaunchParams& P, int tx, int ty, int& x, int& y, int& row) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = tx * 16 + (lane & 15);
    row = (ty + P.wf_tile_row0) * (P.wg_waves * 4) + (lane >> 4) + wave * 4;
    y = image_row(P, row);
    return x < P.res_x && y < P.res_y;
}

// camera ray of pixel (x, y) of batch frame f: frame f's camera and sample array (wave-uniform branch and loads)
template <bool BATCH = false>
__device__ __forceinline__ Ray camera_ray(const LaunchParams& P, int x, int y, int sample, int f) {
    const int ns = P.spp * P.spp;                                                     // RT/main.cpp:776-795
    if (BATCH) {
        const FrameCam& C = P.frame_cams[f];
        if (P.spp == 0) return primary_ray_tab(P, C, x, y);
        const float4 sm = reinterpret_cast<const float4*>(P.samples)[(((size_t)f * P.res_y + y) * P.res_x + x) * ns + sample];
        return primary_ray_lens(P, C, sm.z, sm.w, sm.x, sm.y);
    }
    if (P.spp == 0) return primary_ray_tab(P, P, x, y);                               // RT/main.cpp:756-772
    const float4 sm = reinterpret_cast<const float4*>(P.samples)[((size_t)y * P.res_x + x) * ns + sample];
    return primary_ray_lens(P, P, sm.z, sm.w, sm.x, sm.y);
}

// ------------------------------------------------------------------ workspace records
// RayRec and NodeRec (p3d_device_types.h) move as 16-byte quads: {o | ior} {d | link} and {color | KR} {refl_ret | mat}
// {refr_ret | link}.  The five statements below are the only code that knows which quad and lane holds what; every
// schedule parks, queues, returns and resolves through them.
static_assert(offsetof(RayRec, ior) == 12 && offsetof(RayRec, link) == 28 && offsetof(NodeRec, KR) == 12 && offsetof(NodeRec, mat) == 28 &&
              offsetof(NodeRec, link) == 44, "the quad view below follows the records' layout");

// Write a child ray.  present = false (pair mode only) leaves the marker of a sibling pair's unused half instead.
__device__ __forceinline__ void store_ray(RayRec* r, bool present, const Ray& ray, float ior, uint32_t link) {
    float4* rq = reinterpret_cast<float4*>(r);
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kPairEmpty));
    rq[0] = present ? make_float4(ray.o.x, ray.o.y, ray.o.z, ior) : z;
    rq[1] = present ? make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(link)) : z;
}
// Read a queued ray.
__device__ __forceinline__ void load_ray(const RayRec* r, Ray& ray, float& ior_1, uint32_t& link) {
    const float4* rq = reinterpret_cast<const float4*>(r);
    const float4 a = rq[0], b = rq[1];
    ray.o = mk(a.x, a.y, a.z); ray.d = mk(b.x, b.y, b.z);
    ior_1 = a.w; link = __float_as_uint(b.w);
}
// Write a parked node: both return slots start as zero, which is what the reference adds for a child it never traced.
__device__ __forceinline__ void park_node(NodeRec* n, const NodeOut& o, uint32_t link) {
    float4* nd = reinterpret_cast<float4*>(n);
    nd[0] = make_float4(o.color.x, o.color.y, o.color.z, o.KR);
    nd[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(o.mat));
    nd[2] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(link));
}
// Store a child's return value into the slot of its parent (nodes = the parent's level) that the child's link names.
__device__ __forceinline__ void store_return(NodeRec* nodes, uint32_t link, V3 ret) {
    NodeRec* parent = nodes + (link & ~kLinkRefr);
    float* dst = (link & kLinkRefr) ? parent->refr_ret : parent->refl_ret;
    dst[0] = ret.x; dst[1] = ret.y; dst[2] = ret.z;
}
// Read a parked node and resolve it: color + (refl_ret*KR*spec + refr_ret*(1-KR)), RT/main.cpp:719; link = whom the
// result goes to.  STORED: the children's returns are the record's own slots; else (pair mode, where they never went
// through memory) the caller's.
template <bool STORED = true, class SV>
__device__ __forceinline__ V3 resolve_node(const SV& sv, const NodeRec* n, uint32_t& link, V3 refl_ret = V3(), V3 refr_ret = V3()) {
    const float4* nd = reinterpret_cast<const float4*>(n);
    const float4 a = nd[0], b = nd[1], c = nd[2];
    if (STORED) { refl_ret = mk(b.x, b.y, b.z); refr_ret = mk(c.x, c.y, c.z); }
    const Mtl M = load_material(sv, __float_as_uint(b.w));
    link = __float_as_uint(c.w);
    return combine_node(mk(a.x, a.y, a.z), a.w, M.spec, refl_ret, refr_ret);
}

// ------------------------------------------------------------------ WAVEFRONT schedule
// One shard's slice of the level queues (see LaunchParams::wf_shards).
struct Shard {
    const RayRec* rays_in; uint32_t count_in;
    RayRec* rays_out; uint32_t* count_out;
    NodeRec* nodes_parent; NodeRec* nodes_self; uint32_t* ncount_self;
    NodeRec* nodes_grand;                          // level wf_level - 2 (pair mode)
    const uint32_t* rng_in; uint32_t* rng_out;     // random-stream keys of the queued rays, or nullptr
};
// the counter arrays of this launch under pass parity `par` (see LaunchParams::wf_alt)
__device__ __forceinline__ const uint32_t* count_in_array(const LaunchParams& P, uint32_t par) {
    return P.wf_level == 2 ? P.wf_alt + (size_t)(par * 2u) * kWfShards : P.wf_count_in;
}
__device__ __forceinline__ uint32_t* count_out_array(const LaunchParams& P, uint32_t par) {
    return P.wf_level == 1 ? P.wf_alt + (size_t)(par * 2u) * kWfShards : P.wf_count_out;
}
__device__ __forceinline__ uint32_t* ncount_self_array(const LaunchParams& P, uint32_t par) {
    return P.wf_level == 1 ? P.wf_alt + (size_t)(par * 2u + 1u) * kWfShards : P.wf_ncount_self;
}
__device__ __forceinline__ Shard shard_of(const LaunchParams& P, uint32_t s, uint32_t par) {
    Shard h;
    h.rays_in = P.wf_rays_in ? P.wf_rays_in + (size_t)s * P.wf_cap_in : nullptr;
    h.count_in = P.wf_rays_in ? count_in_array(P, par)[s] : 0u;
    h.rays_out = P.wf_rays_out ? P.wf_rays_out + (size_t)s * P.wf_cap_out : nullptr;
    h.count_out = count_out_array(P, par) + s;
    h.nodes_parent = P.wf_nodes_parent ? P.wf_nodes_parent + (size_t)s * P.wf_ncap_parent : nullptr;
    h.nodes_self = P.wf_nodes_self ? P.wf_nodes_self + (size_t)s * P.wf_ncap_self : nullptr;
    h.nodes_grand = P.wf_nodes_grand ? P.wf_nodes_grand + (size_t)s * P.wf_ncap_grand : nullptr;
    h.ncount_self = ncount_self_array(P, par) + s;
    h.rng_in = P.wf_rng_in ? P.wf_rng_in + (size_t)s * P.wf_cap_in : nullptr;
    h.rng_out = P.wf_rng_out ? P.wf_rng_out + (size_t)s * P.wf_cap_out : nullptr;
    return h;
}

// Hand a finished node's return value to whoever waits for it.
// (parents = this shard's nodes of level - 1; level 1 returns to the pixel, or -- STREAM: the launches of a ray stream
//  that can hold a level-1 node, wf_rays_kernel and the resolve launches -- to the ray's entry of the caller's planes)
template <bool STREAM = false>
__device__ __forceinline__ void deliver(const LaunchParams& P, NodeRec* parents, int level, uint32_t link, V3 ret) {
    if (level == 1) {
        if (STREAM) sink_ray(P, (size_t)link, ret);
        else sink_sample(P, (size_t)link, ret);
        return;
    }
    store_return(parents, link, ret);
}

// Park a node with children and queue its child rays.  Must be reached by ALL lanes of the
// wave together (converged): slots are handed out with ballot + mbcnt prefix sums and one
// atomic per counter per wave.
template <bool STREAM = false>
__device__ __forceinline__ void emit(const LaunchParams& P, const Shard& sh, int level, bool valid, uint32_t link,
                                     float ior_1, const NodeOut& o) {
    const int lane = threadIdx.x & 63;
    if (valid && o.terminal) deliver<STREAM>(P, sh.nodes_parent, level, link, o.ret);
    const bool parks = valid && !o.terminal;
    const uint64_t m_node = __ballot(parks);
    if (m_node == 0) return;                                   // wave-uniform
    const uint64_t m_refl = __ballot(parks && o.has_refl);
    const uint64_t m_refr = __ballot(parks && o.has_refr);
    const uint32_t n_refl = (uint32_t)__popcll(m_refl), n_refr = (uint32_t)__popcll(m_refr);
    const bool pairs = P.wf_pair_out != 0;                     // sibling pairs in even / odd slots for the last level
    uint32_t node_base = 0, ray_base = 0;
    if (lane == (int)__builtin_ctzll(m_node)) {
        node_base = atomicAdd(sh.ncount_self, (uint32_t)__popcll(m_node));
        ray_base = atomicAdd(sh.count_out, pairs ? 2u * (uint32_t)__popcll(m_node) : n_refl + n_refr);
    }
    node_base = __shfl(node_base, (int)__builtin_ctzll(m_node));
    ray_base = __shfl(ray_base, (int)__builtin_ctzll(m_node));
    if (!parks) return;
    const uint32_t my_node = node_base + lane_rank(m_node);
    park_node(sh.nodes_self + my_node, o, link);
    if (pairs) {
        const uint32_t slot = ray_base + 2u * lane_rank(m_node);
        store_ray(sh.rays_out + slot, o.has_refl, o.refl, ior_1, my_node);
        store_ray(sh.rays_out + slot + 1, o.has_refr, o.refr, o.newIor, my_node | kLinkRefr);
        if (sh.rng_out) { sh.rng_out[slot] = o.rng_refl; sh.rng_out[slot + 1] = o.rng_refr; }
        return;
    }
    if (o.has_refl) {                                           // reflection child keeps ior_1
        const uint32_t slot = ray_base + lane_rank(m_refl);
        store_ray(sh.rays_out + slot, true, o.refl, ior_1, my_node);
        if (sh.rng_out) sh.rng_out[slot] = o.rng_refl;
    }
    if (o.has_refr) {
        const uint32_t slot = ray_base + n_refl + lane_rank(m_refr);
        store_ray(sh.rays_out + slot, true, o.refr, o.newIor, my_node | kLinkRefr);
        if (sh.rng_out) sh.rng_out[slot] = o.rng_refr;
    }
}

// Last level in pair mode (LaunchParams::wf_pair_in): every ray of the level has returned (o.ret), lanes 2k / 2k+1 hold
// the reflection / refraction child of one level-(D-1) node.  The even lane combines them with the node's parked record
// -- "color += reflection_color * KR * specColor + refraction_color * (1 - KR)", RT/main.cpp:719, a never-traced child
// adds zero -- and hands the result one level further up.  Must be reached by all lanes of the wave together.
__device__ __forceinline__ void combine_pair(const LaunchParams& P, const Shard& sh, bool valid, uint32_t link, const NodeOut& o) {
    const int lane = threadIdx.x & 63;
    const V3 mine = valid ? o.ret : mk(0.0f, 0.0f, 0.0f);
    const V3 other = mk(__shfl_xor(mine.x, 1), __shfl_xor(mine.y, 1), __shfl_xor(mine.z, 1));
    const uint32_t other_link = (uint32_t)__shfl_xor((int)link, 1);
    const bool other_valid = __shfl_xor(valid ? 1 : 0, 1) != 0;
    if ((lane & 1) != 0 || !(valid || other_valid)) return;
    const uint32_t parent = (valid ? link : other_link) & ~kLinkRefr;
    const GlobalScene gv = View<false>::make(P);
    uint32_t up;
    const V3 ret = resolve_node<false>(gv, sh.nodes_parent + parent, up, mine, other);
    if (P.wf_level == 2) { sink_sample(P, (size_t)up, ret); return; }
    store_return(sh.nodes_grand, up, ret);
}

// diagnostic stamps (only when a stamp buffer was set with p3d_debug_set_stamps): slot k of the
// record of (tile, wave) gets the 100 MHz real-time counter; slot 7 the hardware id registers
__device__ __forceinline__ void stamp_record(unsigned long long* r, int k) {
    r[k] = __builtin_amdgcn_s_memrealtime();
    if (k == 0) r[7] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |
                       ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) << 32);
}
// ALL stamp hooks exist only in builds with -DP3D_STAMPS (`make stamps`, libp3d_hip_stamps.so; the timeline tools select it):
// each hook is a scalar compare and branch per wave on kernels that are bound by scalar issue (the level-1 kernel of
// config 2: 5 hooks = 20 of its 290 scalar instructions per wave).
#ifdef P3D_STAMPS
constexpr bool kStamps = true;
#else
constexpr bool kStamps = false;
#endif
__device__ __forceinline__ void stamp(const LaunchParams& P, int tile, int k) {
    if (kStamps && P.dbg_stamps && P.dbg_stamp_level <= 1 && (threadIdx.x & 63) == 0)
        stamp_record(P.dbg_stamps + ((size_t)tile * P.wg_waves + (threadIdx.x >> 6)) * 8, k);
}
// the same for the deeper-level kernel (p3d_debug_set_stamp_level(l), l >= 2): one record per WAVE of the launch, written
// for the wave's first batch -- 0 start, 1 queue read, 2 closest hit, 3 shading, 4 emit / pair combine -- then 5 = the wave
// is done and 6 = the number of batches it ran
// (only in builds with -DP3D_STAMPS -- `make stamps`, libp3d_hip_stamps.so, tools/wave_timeline.py: the checks cost the
//  deeper-level kernel 25 spilled scalar registers, and that kernel is bound by instruction issue)
__device__ __forceinline__ bool stamps_on(const LaunchParams& P) {
#ifdef P3D_STAMPS
    return P.dbg_stamps && P.dbg_stamp_level == P.wf_level && (threadIdx.x & 63) == 0;
#else
    return false;
#endif
}
__device__ __forceinline__ void stamp_wave(const LaunchParams& P, uint32_t wave_id, int k, bool first = true) {
    if (first && stamps_on(P)) stamp_record(P.dbg_stamps + (size_t)wave_id * 8, k);
}

// level 1: camera rays of one sample pass over a band of tiles
// OCC = requested waves per SIMD (amdgpu_waves_per_eu): caps the VGPR allocation so that more
// waves hide each other's latency, at the price of a few spilled registers.  Selected at run
// time by p3d_set_tuning(); never changes results.

// One workgroup per 16 x (4 x wg_waves) tile, dispatched by the hardware.  (A persistent variant -- resident-sized
// grid, scene copied once per workgroup, every wave drawing 16x4 tiles from device counters with the next number
// prefetched -- was measured and dropped: 520 us with one counter (a word saturates at ~88 returning atomics per
// microsecond), 110 us with 64 counters on separate lines, against 50 us for this plain grid.)
// (Measured and dropped in round 3, profiles/r03_exp03_sharing_wg_levers.txt: 8- and 16-wave workgroups -- level 1 of
//  config 2 46 -> 51 -> 54 us: the waves of this launch start at ~830 per microsecond whatever the workgroup shape.)
//
template <bool COUNT, bool LDS, int WALK, int OCC, bool STOCH = false, bool SCHLICK = false, bool BATCH = false, bool AOV = false>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void wf_primary_kernel(const LaunchParams P) {
    const uint32_t par = P.wf_ctrl[0] & 1u;                     // this pass's counter set (LaunchParams::wf_alt)
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        if (threadIdx.x == 0) P.wf_ctrl[32] = par;
        for (uint32_t i = threadIdx.x; i < P.wf_clear_words; i += blockDim.x) P.wf_clear[i] = 0u;
        uint32_t* other = P.wf_alt + (size_t)((1u - par) * 2u) * kWfShards;
        for (uint32_t i = threadIdx.x; i < 2u * kWfShards; i += blockDim.x) other[i] = 0u;
    }
    const typename View<LDS>::type sv = View<LDS>::make_shading(P);
    int x, y, row, f, tile;
    const bool valid = tile_pixel<!LDS, BATCH>(P, x, y, row, f, &tile);
    if (__ballot(valid) == 0) return;
    const Shard sh = shard_of(P, (uint32_t)tile % kWfShards, par);
    const TravCtx tc = wave_stack<LDS>(P, 0);
    Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
    const size_t p = (size_t)out_row<BATCH>(P, f, row) * P.res_x + x;
    const unsigned long long t_tile = (!LDS && P.tile_cost) ? __builtin_amdgcn_s_memrealtime() : 0ull;
    stamp(P, tile, 0);
    Ray ray; ray.o = mk(0.0f, 0.0f, 0.0f); ray.d = mk(1.0f, 0.0f, 0.0f);
    if (valid) ray = camera_ray<BATCH>(P, x, y, P.wf_sample, f);
    stamp(P, tile, 1);
    const Hit h = find_closest<COUNT, WALK>(P, sv, ray, valid, tc, ctr);
    stamp(P, tile, 2);
    if (valid && P.hit_id && P.wf_sample == 0) P.hit_id[p] = hit_id_of(h);
    if (AOV && P.wf_sample == 0) write_aov(P, sv, p, valid, ray, h);             // wave-uniform
    // the random stream of a pixel sample is keyed by the pixel's place in the FULL frame, so a frame
    // sharded over several GPUs draws the same numbers as on one (frame f of a batch: seed + f)
    const uint32_t rng = STOCH ? rng_mix(rng_mix(BATCH ? P.seed + (uint32_t)f : P.seed, (uint32_t)(y * P.res_x + x)), (uint32_t)P.wf_sample) : 0u;
    const NodeOut o = shade_hit<COUNT, WALK, typename View<LDS>::type, STOCH, SCHLICK>(P, sv, ray, h, valid, 1, 1.0f, tc, ctr, rng);
    stamp(P, tile, 3);
    emit(P, sh, 1, valid, (uint32_t)p, 1.0f, o);
    stamp(P, tile, 4);
    if (!LDS && P.tile_cost && threadIdx.x == 0) P.tile_cost[tile] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_tile);
    if (valid) flush_counters<COUNT>(P, ctr, P.wf_sample == 0 ? 1u : 0u);
}

// wf_primary_kernel with TILES (2 or 3) tiles per workgroup, for scenes served from LDS on the 2-D launch, built where
// has_primary_tiles() says so: per-lane walk, no counters, no features, one frame, no AOV planes, so the steps below are those of
// wf_primary_kernel<false, true, WALK, OCC> and nothing else.  (wf_primary_kernel keeps its own statements: routed through
// primary_tile_lds() its ~120 builds came out of the compiler with other scalar-register spills, 18 more in the counting
// grid-walk builds, and the registered profiles and the register account, tools/kdiff.py, are those builds'.  For the same
// reason this is a kernel of its own name and not a template parameter of wf_primary_kernel, which would rename them all.)
//
// One tile: the camera rays of the tile's pixels, traced, shaded, and their children queued in the tile's shard
// (tile % kWfShards, whichever workgroup runs the tile: the queues' contents do not depend on the launch's shape).
// Must be reached by all lanes of the wave together (emit).
template <int WALK>
__device__ __forceinline__ void primary_tile_lds(const LaunchParams& P, const LdsScene& sv, const TravCtx& tc, uint32_t par, int tile, bool valid,
                                                 int x, int y, int row) {
    const Shard sh = shard_of(P, (uint32_t)tile % kWfShards, par);
    Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
    const size_t p = (size_t)row * P.res_x + x;
    stamp(P, tile, 0);
    Ray ray; ray.o = mk(0.0f, 0.0f, 0.0f); ray.d = mk(1.0f, 0.0f, 0.0f);
    if (valid) ray = camera_ray<false>(P, x, y, P.wf_sample, 0);
    stamp(P, tile, 1);
    const Hit h = find_closest<false, WALK>(P, sv, ray, valid, tc, ctr);
    stamp(P, tile, 2);
    if (valid && P.hit_id && P.wf_sample == 0) P.hit_id[p] = hit_id_of(h);
    const NodeOut o = shade_hit<false, WALK, LdsScene, false, false>(P, sv, ray, h, valid, 1, 1.0f, tc, ctr, 0u);
    stamp(P, tile, 3);
    emit(P, sh, 1, valid, (uint32_t)p, 1.0f, o);
    stamp(P, tile, 4);
}

// The frame's tile coverage mask (LaunchParams::sky_mask, p3d_tile_coverage.h): is tile (tx, ty) of this band one a primitive
// may project onto?  Wave-uniform, and read through the constant address space so that it is a scalar load whatever the
// compiler can prove about the stores before it: the mask was written by an earlier launch of the stream and nothing in
// this one writes it.
__device__ __forceinline__ bool tile_may_hit(const LaunchParams& P, const uint32_t* mask, int tx, int ty) {
    typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
    const uint32_t w = ((ConstWords)mask)[(uint32_t)(ty + P.wf_tile_row0) * P.sky_mask_row_words + ((uint32_t)tx >> 5)];
    return ((w >> ((uint32_t)tx & 31u)) & 1u) != 0u;
}
// A tile the mask marks empty: every camera ray of it leaves the scene, so each valid pixel gets what such a ray's tree
// returns -- miss_color() = bg, clamped by sink_sample(), through the same write_pixel() -- and hit_id -1.  No camera ray, no
// shard, no walk, no shading, nothing queued (a ray that hits nothing parks no node and queues no child).
__device__ __forceinline__ void fill_sky_tile(const LaunchParams& P, int tx, int ty) {
    int x, y, row;
    const bool valid = tile_pixel_at(P, tx, ty, x, y, row);
    if (!valid) return;
    const size_t p = (size_t)row * P.res_x + x;
    write_pixel(P, p, clampc(mk(P.bg[0], P.bg[1], P.bg[2])));
    if (P.hit_id && P.wf_sample == 0) P.hit_id[p] = -1;
}

// Workgroup (bx, by) runs the tiles of column bx in tile rows by, by + gridDim.y, by + 2 gridDim.y one after the other.
// Once per workgroup: the parity read, the first-block clearing, the scene copy and its barrier, the wave's stack.
// Per tile: tile -> pixel, shard_of(), the camera ray, find_closest(), shade_hit(), emit() -- and the launch parameters
// those read, see below.  The loop carries nothing but its wave-uniform counter from one tile to the next.
// With a coverage mask (sky_mask != nullptr; the host decides which frames have one, p3d_render.cpp): a tile whose bit is
// clear is filled by fill_sky_tile() and the loop goes on, and a workgroup none of whose tiles has its bit set fills them
// and returns before the scene copy and its barrier -- the test is on blockIdx and the mask alone, so the whole workgroup
// takes the same side.  The first block's clearing above it stays unconditional.
template <int WALK, int OCC, int TILES>
__global__ __launch_bounds__(256) P3D_OCC(OCC) void wf_primary_kernel_tiles(const LaunchParams P) {
    static_assert(TILES >= 2 && TILES <= kMaxPrimaryTiles, "one tile per workgroup is wf_primary_kernel");
    const uint32_t par = P.wf_ctrl[0] & 1u;                     // this pass's counter set (LaunchParams::wf_alt)
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        if (threadIdx.x == 0) P.wf_ctrl[32] = par;
        for (uint32_t i = threadIdx.x; i < P.wf_clear_words; i += blockDim.x) P.wf_clear[i] = 0u;
        uint32_t* other = P.wf_alt + (size_t)((1u - par) * 2u) * kWfShards;
        for (uint32_t i = threadIdx.x; i < 2u * kWfShards; i += blockDim.x) other[i] = 0u;
    }
    const int tx = blockIdx.x;
    if (P.sky_mask) {                                                         // (launch-uniform)
        bool any = false;
        for (int k = 0; k < TILES; k++) {
            const int ty = (int)(blockIdx.y + (uint32_t)k * gridDim.y);
            if (ty < P.wf_tile_rows && tile_may_hit(P, P.sky_mask, tx, ty)) any = true;
        }
        if (!any) {                                                           // workgroup-uniform, before the scene copy's barrier
            for (int k = 0; k < TILES; k++) {
                const int ty = (int)(blockIdx.y + (uint32_t)k * gridDim.y);
                if (ty < P.wf_tile_rows) fill_sky_tile(P, tx, ty);
            }
            return;
        }
    }
    const LdsScene sv = View<true>::make_shading(P);
    const TravCtx tc = wave_stack<true>(P, 0);
#pragma nounroll
    for (int k = 0; k < TILES; k++) {
        const int ty = (int)(blockIdx.y + (uint32_t)k * gridDim.y);          // wave-uniform: the loop's state stays in scalar registers
        if (ty >= P.wf_tile_rows) break;                                      // past the band's last tile row (after the barrier)
        // The tile reads its launch parameters through a pointer the compiler cannot see through.  Read from P they are all
        // loop-invariant: the compiler hoists ~100 of them, they stay live across the whole loop, and the kernel spilled 101
        // scalar registers into lanes of 86 vector registers (scratch under the budget of 6 waves per SIMD): what cost round 3's
        // run-time loop its occupancy.  Read here they are scalar loads where they are used, as in wf_primary_kernel: 30 more
        // s_load per tile, 1 spilled scalar register, no scratch.  The kernel's one argument IS the kernarg segment:
        static_assert(std::is_same_v<decltype(&wf_primary_kernel_tiles<WALK, OCC, TILES>), void (*)(const LaunchParams)>,
                      "Q below reads the kernarg segment as the kernel's only argument, a LaunchParams at offset 0");
        auto args = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(args));
        const LaunchParams& Q = *(const LaunchParams*)args;
        if (const uint32_t* mask = Q.sky_mask) {
            if (!tile_may_hit(Q, mask, tx, ty)) { fill_sky_tile(Q, tx, ty); continue; }
        }
        int x, y, row;
        const bool valid = tile_pixel_at(Q, tx, ty, x, y, row);
        if (__ballot(valid) == 0) continue;
        primary_tile_lds<WALK>(Q, sv, tc, par, ty * Q.tiles_x + tx, valid, x, y, row);
    }
}

// Level 1 of a ray stream (p3d_trace_rays): wf_primary_kernel's steps for rays the caller supplies.  Workgroup b of the band
// is the band's "tile" b -- the 64 * wg_waves consecutive rays from (wf_tile_row0 + b) * blockDim on, shard b % kWfShards --
// and a lane's link is its ray's index in the stream, so the deeper levels and the resolve launches run unchanged.  No
// camera, no tile map, no counters, no features with random draws: one build per scene placement and walk
// (p3d_kernel_variant.h: Level::Rays).  Consecutive lanes read consecutive 12-byte records: one 768-byte run per array per wave.
// hit_id / t / normal are written here, under wave-uniform tests of their pointers: a caller that asks for colours only
// pays three scalar compares.  Lanes past the stream's last ray neither read nor write; they stay for the wave-wide steps.
template <bool LDS, int WALK, int OCC>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void wf_rays_kernel(const LaunchParams P, const RayStreamIO R) {
    const uint32_t par = P.wf_ctrl[0] & 1u;                     // this pass's counter set (LaunchParams::wf_alt)
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) P.wf_ctrl[32] = par;
        for (uint32_t i = threadIdx.x; i < P.wf_clear_words; i += blockDim.x) P.wf_clear[i] = 0u;
        uint32_t* other = P.wf_alt + (size_t)((1u - par) * 2u) * kWfShards;
        for (uint32_t i = threadIdx.x; i < 2u * kWfShards; i += blockDim.x) other[i] = 0u;
    }
    const typename View<LDS>::type sv = View<LDS>::make_shading(P);
    const uint32_t i = ((uint32_t)P.wf_tile_row0 + blockIdx.x) * blockDim.x + threadIdx.x;     // (the host keeps streams below 2^31 rays)
    const bool valid = i < R.count;
    if (__ballot(valid) == 0) return;
    const Shard sh = shard_of(P, blockIdx.x % kWfShards, par);
    TravCtx tc = wave_stack<LDS>(P, 0);
    Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
    Ray ray; ray.o = mk(0.0f, 0.0f, 0.0f); ray.d = mk(1.0f, 0.0f, 0.0f);
    if (valid) {                                                 // Ray(origin[i], dir[i]): the direction is NOT normalised
        const float* po = R.origin + 3 * (size_t)i;
        const float* pd = R.dir + 3 * (size_t)i;
        ray.o = mk(po[0], po[1], po[2]); ray.d = mk(pd[0], pd[1], pd[2]);
    }
    tc.lane.walk_all = !slab_can_cull(ray);                      // a caller's ray: p3d_traverse.h, slab_can_cull (its shadow rays too)
    const Hit h = find_closest<false, WALK>(P, sv, ray, valid, tc, ctr);
    if (P.hit_id || R.t || R.normal) {                           // wave-uniform
        const bool hit = valid && h.ref != 0xFFFFFFFFu;
        if (valid && P.hit_id) P.hit_id[i] = hit_id_of(h);
        if (valid && R.t) R.t[i] = hit ? h.t : __builtin_inff();
        if (R.normal) {                                      // getNormal(hit point).normalize(), RT/main.cpp:587-589
            V3 n = mk(0.0f, 0.0f, 0.0f);
            if (hit) n = prim_normal(P, sv, h.ref, ray, add(ray.o, mul(ray.d, h.t)));
            if (valid) { float* pn = R.normal + 3 * (size_t)i; pn[0] = n.x; pn[1] = n.y; pn[2] = n.z; }
        }
    }
    const NodeOut o = shade_hit<false, WALK, typename View<LDS>::type, false, false>(P, sv, ray, h, valid, 1, 1.0f, tc, ctr, 0u);
    emit<true>(P, sh, 1, valid, i, 1.0f, o);
}

// The shadow query of processLight() on segments the caller supplies (p3d_occluded): segment i is Ray(origin[i], dir[i]), the
// "Ray(precise_hit_point, L)" of RT/main.cpp:478, and occluded[i] what the switch below it sets insideShadow to.  The query is
// the frames' own: shadow_segment() and light_occluded() of p3d_shade.h, with "the lane has a segment" as need (the L.N > 0
// test is the caller's).  One segment per lane, consecutive 12-byte records as in wf_rays_kernel, one byte written per
// segment; no queues, no control words, no counters, nothing of a frame.  Workgroup b takes the blockDim.x consecutive
// segments from b * blockDim.x on.  Lanes past the last segment neither read nor write; they stay for the wave-wide walk.
// One build per scene placement and walk (p3d_kernel_variant.h: Level::Occlusion).
// (A workgroup looping over several batches, on a grid sized from the resident workgroups, so that a scene served from LDS
//  is copied once per workgroup and not once per 256 segments, was measured and dropped: no faster at 2 and 4 x the resident
//  workgroups, 1 - 3 % slower at 1 x; profiles/occlusion_cost.txt.)
template <bool LDS, int WALK, int OCC>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void wf_occlusion_kernel(const LaunchParams P, const OcclusionIO R) {
    const typename View<LDS>::type sv = View<LDS>::make(P);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;    // (the host keeps n below 2^31)
    const bool valid = i < R.count;
    if (__ballot(valid) == 0) return;                            // no barrier follows the scene copy's
    TravCtx tc = wave_stack<LDS>(P, 0);
    Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
    V3 o = mk(0.0f, 0.0f, 0.0f), L = mk(1.0f, 0.0f, 0.0f);
    if (valid) {
        const float* po = R.origin + 3 * (size_t)i;
        const float* pd = R.dir + 3 * (size_t)i;
        o = mk(po[0], po[1], po[2]); L = mk(pd[0], pd[1], pd[2]);
    }
    { Ray given; given.o = o; given.d = L; tc.lane.walk_all = !slab_can_cull(given); }   // a caller's segment, as given: p3d_traverse.h
    const bool occluded = light_occluded<false, WALK>(P, sv, shadow_segment(L), o, valid, tc, ctr);
    if (valid) R.occluded[i] = occluded ? 1 : 0;
}

// Lanes a wave of a deeper level uses: a short queue is spread over ALL the shard's waves with
// fewer rays each instead of filling 64-wide waves.  Deeper levels hold few, incoherent rays and
// are bound by the latency of one wave's ray step, not by issue slots: narrow waves diverge less
// (the step lasts as long as the slowest of its lanes) and more of them are in flight to hide
// each other's memory latency.  Scenes served from LDS keep full waves (wf_min_width = 64):
// there the extra waves only cost issue slots (measured: 0.14 -> 0.20 ms on config 2).
__device__ __forceinline__ uint32_t wave_width(uint32_t count, uint32_t waves_per_shard, uint32_t min_width) {
    // narrow only while the rays still fit the waves that can be RESIDENT at once (a quarter of the
    // launched ones): beyond that, narrower waves just spend issue slots on idle lanes
    const unsigned long long resident = waves_per_shard >= 4 ? waves_per_shard / 4 : 1;
    uint32_t width = 64;
    while (width > min_width && resident * (width >> 1) >= count) width >>= 1;
    return width;
}

// One step of a deeper level for one batch of the wave: lane's ray = entry i of the shard's queue (valid: there is one).
// Must be reached by all lanes of the wave together.  st1 = this is the wave's first batch: the one its stamps describe.
template <bool COUNT, bool LDS, int WALK, bool STOCH, bool SCHLICK>
__device__ __forceinline__ void queued_ray_step(const LaunchParams& P, const typename View<LDS>::type& sv, const Shard& sh, const TravCtx& tc,
                                                Ctr& ctr, uint32_t i, bool valid, uint32_t wave_id, bool st1) {
    uint32_t link = 0, rng = 0; float ior_1 = 1.0f;
    Ray ray; ray.o = mk(0.0f, 0.0f, 0.0f); ray.d = mk(1.0f, 0.0f, 0.0f);
    if (valid) {
        load_ray(sh.rays_in + i, ray, ior_1, link);
        if (STOCH) rng = sh.rng_in[i];
    }
    const bool live = valid && link != kPairEmpty;           // (the unused half of a sibling pair)
    // (stamp 1, the queue read, is taken for LDS scenes only)
    if (LDS && stamps_on(P) && st1) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp_wave(P, wave_id, 1); }
    const Hit h = find_closest<COUNT, WALK>(P, sv, ray, live, tc, ctr);
    stamp_wave(P, wave_id, 2, st1);
    const NodeOut o = shade_hit<COUNT, WALK, typename View<LDS>::type, STOCH, SCHLICK>(P, sv, ray, h, live, P.wf_level, ior_1, tc, ctr, rng);
    stamp_wave(P, wave_id, 3, st1);
    if (P.wf_pair_in) combine_pair(P, sh, live, link, o);
    else emit(P, sh, P.wf_level, live, link, ior_1, o);
    stamp_wave(P, wave_id, 4, st1);
}

// Inclusive prefix sum over the 64 lanes of a wave, all of them active, in six vector adds on the data-parallel
// primitives: row shifts by 1, 2, 4 and 8 sum within each row of 16 lanes, then the last lane of rows 0 and 2 is
// broadcast into rows 1 and 3, and lane 31 into rows 2 and 3.  A lane with no source, and a row the mask leaves out,
// adds zero.  Needs a 64-lane wave with every lane enabled (a disabled lane would neither pass its value on nor take
// one) and the row broadcasts of the gfx9 family (gfx950 has them; gfx10 and later do not).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    v += dpp_or_zero<0x111, 0xf>(v);     // row_shr:1
    v += dpp_or_zero<0x112, 0xf>(v);     // row_shr:2
    v += dpp_or_zero<0x114, 0xf>(v);     // row_shr:4
    v += dpp_or_zero<0x118, 0xf>(v);     // row_shr:8
    v += dpp_or_zero<0x142, 0xa>(v);     // row_bcast:15 into rows 1 and 3
    v += dpp_or_zero<0x143, 0xc>(v);     // row_bcast:31 into rows 2 and 3
    return v;
}

// level >= 2: one queued ray per lane, persistent waves striding over the queue
template <bool COUNT, bool LDS, int WALK, int OCC, bool STOCH = false, bool SCHLICK = false>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void wf_secondary_kernel(const LaunchParams P) {
    constexpr uint32_t S = kWfShards;
    const uint32_t wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    const uint32_t par = P.wf_ctrl[32] & 1u;                    // set by the level-1 launch of this pass
    if (P.wf_level == 2 && blockIdx.x == 0 && threadIdx.x == 0) P.wf_ctrl[0] = 1u - par;   // the next pass takes the other set
    const uint32_t* counts_in = count_in_array(P, par);
    if (LDS) {
        // Scenes served from LDS: full 64-ray batches, numbered THROUGH all shards (the host launches S == 64
        // shards, one count per lane: batches per shard, wave-wide prefix sum), batch b goes to wave b % n_waves.
        // A deeper level of a 1080p frame is ~1.15 batches per resident-at-4-per-SIMD wave, and a launch lasts as
        // long as its busiest wave: with the grid sized to what can be RESIDENT (host: occupancy query) and every
        // wave owning at most one batch whichever shard it is in, the level costs one ray step instead of two.
        const uint32_t c = (uint32_t)lane < S ? counts_in[lane] : 0u;
        const uint32_t nb = (c + 63u) >> 6;
        const uint32_t incl = wave_inclusive_scan(nb);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (((blockIdx.x * blockDim.x) >> 6) >= total) return;      // workgroup-uniform, before the scene copy's barrier
        const typename View<LDS>::type sv = View<LDS>::make_shading(P);
        const TravCtx tc = wave_stack<LDS>(P, 0);
        Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
        uint32_t n_batches = 0;
        // Read once per wave, above: parity, counts and their scan, the scene view, the stack.  Everything else a batch
        // reads of the launch parameters it reads through a pointer the compiler cannot see through, for the reason given
        // in wf_primary_kernel_tiles: read from P they are all invariant in this loop, are hoisted out of it and stay live,
        // spilled into lanes of vector registers, across both walks of every batch.  The kernel's one argument IS the
        // kernarg segment:
        static_assert(std::is_same_v<decltype(&wf_secondary_kernel<COUNT, LDS, WALK, OCC, STOCH, SCHLICK>), void (*)(const LaunchParams)>,
                      "Q below reads the kernarg segment as the kernel's only argument, a LaunchParams at offset 0");
        for (uint32_t b = wave_id; b < total; b += n_waves, n_batches++) {
            auto args = __builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(args));
            const LaunchParams& Q = *(const LaunchParams*)args;
            const bool st1 = n_batches == 0;
            stamp_wave(Q, wave_id, 0, st1);
            const int s = (int)__builtin_ctzll(__ballot(incl > b));  // the shard batch b belongs to
            const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)(incl - nb), s);   // batches in the shards before it
            const Shard sh = shard_of(Q, (uint32_t)s, par);
            const uint32_t i = (b - first) * 64u + lane;
            queued_ray_step<COUNT, LDS, WALK, STOCH, SCHLICK>(Q, sv, sh, tc, ctr, i, i < sh.count_in, wave_id, st1);
        }
        if (stamps_on(P) && n_batches) { stamp_wave(P, wave_id, 5); P.dbg_stamps[(size_t)wave_id * 8 + 6] = n_batches; }
        flush_counters<COUNT>(P, ctr, 0u);
        return;
    }
    // Scenes read from HBM: wave g works on shard g % S; the (gridwaves / S) waves of a shard stride over its
    // queue, with narrow waves when the queue is short (wave_width)
    const uint32_t per_shard = n_waves / S;
    {   // workgroup-uniform early exit (before the scene copy's barrier): nothing queued for any of
        // this workgroup's waves
        const uint32_t w0 = (blockIdx.x * blockDim.x) >> 6, nw = blockDim.x >> 6;
        bool any = false;
        for (uint32_t w = w0; w < w0 + nw; w++) {
            const uint32_t c = counts_in[w % S];
            if ((w / S) * wave_width(c, per_shard, (uint32_t)P.wf_min_width) < c) any = true;
        }
        if (!any) return;
    }
    const typename View<LDS>::type sv = View<LDS>::make_shading(P);
    const Shard sh = shard_of(P, wave_id % S, par);
    const TravCtx tc = wave_stack<LDS>(P, 0);
    Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
    const uint32_t width = wave_width(sh.count_in, per_shard, (uint32_t)P.wf_min_width);
    uint32_t n_batches = 0;
    for (uint32_t base = (wave_id / S) * width; base < sh.count_in; base += per_shard * width, n_batches++) {
        const bool st1 = n_batches == 0;
        stamp_wave(P, wave_id, 0, st1);
        const uint32_t i = base + lane;
        queued_ray_step<COUNT, LDS, WALK, STOCH, SCHLICK>(P, sv, sh, tc, ctr, i, (uint32_t)lane < width && i < sh.count_in, wave_id, st1);
    }
    if (stamps_on(P) && n_batches) { stamp_wave(P, wave_id, 5); P.dbg_stamps[(size_t)wave_id * 8 + 6] = n_batches; }
    flush_counters<COUNT>(P, ctr, 0u);
}

// walk one level back up: node = color + (refl_ret*KR*spec + refr_ret*(1-KR)), RT/main.cpp:719
// (STREAM: the builds a ray stream's passes launch, whose level-1 nodes return to sink_ray(); see deliver())
template <bool STREAM>
__global__ __launch_bounds__(256) void wf_resolve_kernel(const LaunchParams P) {
    constexpr uint32_t S = kWfShards;
    const Shard sh = shard_of(P, blockIdx.x % S, P.wf_ctrl[32] & 1u);
    const uint32_t count = *sh.ncount_self;
    const uint32_t per_shard = gridDim.x / S;
    const GlobalScene gv = View<false>::make(P);
    for (uint32_t i = (blockIdx.x / S) * blockDim.x + threadIdx.x; i < count; i += per_shard * blockDim.x) {
        uint32_t link;
        const V3 ret = resolve_node(gv, sh.nodes_self + i, link);
        deliver<STREAM>(P, sh.nodes_parent, P.wf_level, link, ret);
    }
}

// The same for ALL levels in one launch, one 1024-thread workgroup per shard: a ray never leaves its pixel's shard, so a
// shard's levels only depend on each other and a __syncthreads() between levels replaces the launch boundary.  For
// small frames -- a rank's share of a frame tiled over several GPUs -- where a level holds a few nodes per thread and a
// frame is bound by the number of launches (tools/shard_probe.py); large frames keep one wide launch per level.
template <bool STREAM>
__global__ __launch_bounds__(1024) void wf_resolve_fused_kernel(const LaunchParams P, const ResolveLevels R) {
    const uint32_t s = blockIdx.x, par = P.wf_ctrl[32] & 1u;
    const GlobalScene gv = View<false>::make(P);
    for (int l = R.top; l >= 1; l--) {
        const NodeRec* nodes = R.nodes[l] + (size_t)s * R.cap[l];
        NodeRec* parents = l > 1 ? R.nodes[l - 1] + (size_t)s * R.cap[l - 1] : nullptr;
        const uint32_t count = l == 1 ? (P.wf_alt + (size_t)(par * 2u + 1u) * kWfShards)[s] : R.ncount[l][s];
        for (uint32_t i = threadIdx.x; i < count; i += blockDim.x) {
            uint32_t link;
            const V3 ret = resolve_node(gv, nodes + i, link);
            deliver<STREAM>(P, parents, l, link, ret);
        }
        __syncthreads();             // the workgroup's own stores are visible to it after the barrier
    }
}

// ------------------------------------------------------------------ TILE schedule
// ONE launch per frame.  The wavefront schedule above spends six of its seven launches on the deeper
// levels of a 1080p frame, each lasting as long as one or two incoherent ray steps of a wave whatever
// the number of rays (launch ramp + quantisation: 1.15 batches per wave rounds up to 2), and hands rays
// from level to level through device-scope atomics and HBM-sized worst-case queues.  A ray never leaves
// its pixel's tile, so here a 256-thread workgroup keeps a 16x16 tile's whole tree to itself: level 1
// traces the camera rays, child rays are compacted (ballot + mbcnt, one LDS atomic per counter per wave)
// into the workgroup's PRIVATE slot of the workspace, the four waves share each deeper level's batches,
// and the resolve passes walk the levels back up -- all between __syncthreads(), no global atomics, no
// cross-CU hand-off (a workgroup's own stores are visible to it after the barrier).  Workgroups are
// persistent and draw tiles from one counter, so cheap sky tiles flow past expensive glass tiles and the
// workspace is (resident workgroups) x (one tile's worst case): ~200 MB at depth 4 instead of gigabytes.
// Samples of the anti-aliased path run back to back inside the tile: "color += rayTracing().clamp()" in
// sample order is an LDS accumulator, there are no per-sample planes and no summing launch.
// Same shade_hit()/combine_node() as the other schedules: bit-identical frames.
struct TileLds {
    uint32_t n_rays[kMaxTileLevels];      // rays queued for level l (2..D)
    uint32_t n_nodes[kMaxTileLevels];     // nodes parked at level l (1..D-1)
    uint32_t tile, pad;
    float acc[3 * kTilePx];               // sum of the clamped sample colours of each pixel (spp > 0)
};

// LDS scenes: the first kTileLdsRays queued rays of a level stay in LDS -- two buffers, written and read alternately
// by consecutive levels (a level's own barrier separates them); only what does not fit goes through the workgroup's
// slot in HBM.  A 16x16 tile of config 4 queues ~750 rays per sample pass, ~300 of them for its largest level: the
// ray half of the queue traffic (11.6 GB per frame in round 2, profiles/r02_config4_pmc.json) stays on the CU.
constexpr uint32_t kTileLdsRays = 256;
constexpr uint32_t kTileLdsRayDwords = 2u * kTileLdsRays * 8u;        // 16 KB

struct TileCtx {
    uint32_t lds_off;                     // dword offset of the TileLds inside p3d_lds
    uint32_t lq_off;                      // dword offset of the LDS ray buffers (0 = none: scenes read from HBM)
    // ray slot `i` of level `l`: in LDS below kTileLdsRays (when the kernel has the buffers), else in the HBM slot
    __device__ __forceinline__ RayRec* ray_slot(int l, uint32_t i) const {
        if (lq_off != 0u && i < kTileLdsRays)
            return reinterpret_cast<RayRec*>(reinterpret_cast<float4*>(p3d_lds + lq_off) + ((uint32_t)(l & 1) * kTileLdsRays + i) * 2u);   // (two quads per ray)
        return rays + tile_ray_offset(l) + i;
    }
    RayRec* rays; NodeRec* nodes; uint32_t* keys;     // this workgroup's slot
    int tx, ty;                           // tile coordinates
    int oy;                               // batches only: row of the caller's planes that the tile's top row goes to
    __device__ __forceinline__ TileLds* lds() const { return reinterpret_cast<TileLds*>(p3d_lds + lds_off); }
};

// compact pixel index of tile-local pixel `link` (= the thread id that traced it)
template <bool BATCH>
__device__ __forceinline__ size_t tile_pixel_index(const LaunchParams& P, const TileCtx& X, uint32_t link) {
    const int x = X.tx * 16 + (int)(link & 15u);
    const int row = (BATCH ? X.oy : X.ty * 16) + (int)(link >> 6) * 4 + (int)((link >> 4) & 3u);
    return (size_t)row * P.res_x + x;
}

template <bool BATCH>
__device__ __forceinline__ void tile_deliver(const LaunchParams& P, const TileCtx& X, int level, uint32_t link, V3 ret) {
    if (level == 1) {                                            // "rayTracing(...).clamp()" of a pixel sample
        const V3 c = clampc(ret);
        if (P.spp == 0) { write_pixel(P, tile_pixel_index<BATCH>(P, X, link), c); return; }
        float* a = X.lds()->acc + 3 * link;                      // color += ... in sample order (RT/main.cpp:797)
        a[0] = a[0] + c.x; a[1] = a[1] + c.y; a[2] = a[2] + c.z;
        return;
    }
    store_return(X.nodes + tile_node_offset(level - 1), link, ret);
}

// like emit(): must be reached by all lanes of the wave together
template <bool BATCH>
__device__ __forceinline__ void tile_emit(const LaunchParams& P, const TileCtx& X, int level, bool valid, uint32_t link,
                                          float ior_1, const NodeOut& o) {
    const int lane = threadIdx.x & 63;
    if (valid && o.terminal) tile_deliver<BATCH>(P, X, level, link, o.ret);
    const bool parks = valid && !o.terminal;
    const uint64_t m_node = __ballot(parks);
    if (m_node == 0) return;                                   // wave-uniform
    const uint64_t m_refl = __ballot(parks && o.has_refl);
    const uint64_t m_refr = __ballot(parks && o.has_refr);
    const uint32_t n_refl = (uint32_t)__popcll(m_refl), n_refr = (uint32_t)__popcll(m_refr);
    uint32_t node_base = 0, ray_base = 0;
    const int first = (int)__builtin_ctzll(m_node);
    if (lane == first) {
        TileLds* T = X.lds();
        node_base = atomicAdd(&T->n_nodes[level], (uint32_t)__popcll(m_node));
        ray_base = atomicAdd(&T->n_rays[level + 1], n_refl + n_refr);
    }
    node_base = __shfl(node_base, first);
    ray_base = __shfl(ray_base, first);
    if (!parks) return;
    const uint32_t my_node = node_base + lane_rank(m_node);
    park_node(X.nodes + tile_node_offset(level) + my_node, o, link);
    if (o.has_refl) {                                           // reflection child keeps ior_1
        const uint32_t slot = ray_base + lane_rank(m_refl);
        store_ray(X.ray_slot(level + 1, slot), true, o.refl, ior_1, my_node);
        if (X.keys) X.keys[tile_ray_offset(level + 1) + slot] = o.rng_refl;
    }
    if (o.has_refr) {
        const uint32_t slot = ray_base + n_refl + lane_rank(m_refr);
        store_ray(X.ray_slot(level + 1, slot), true, o.refr, o.newIor, my_node | kLinkRefr);
        if (X.keys) X.keys[tile_ray_offset(level + 1) + slot] = o.rng_refr;
    }
}

template <bool COUNT, bool LDS, int WALK, int OCC, bool STOCH = false, bool SCHLICK = false, bool BATCH = false, bool AOV = false>
__global__ __launch_bounds__(256) P3D_OCC(OCC) void wf_tile_kernel(const LaunchParams P) {
    const typename View<LDS>::type sv = View<LDS>::make_shading(P);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TravCtx tc = wave_stack<LDS>(P, 0);
    TileCtx X;
    X.lds_off = View<LDS>::scene_dwords(P) + 4u * P.trav_stack_dwords;
    X.lq_off = LDS ? X.lds_off + (uint32_t)((sizeof(TileLds) + 15) / 16) * 4u : 0u;
    uint8_t* slot = P.tw_base + (size_t)blockIdx.x * P.tw_slot_bytes;
    X.rays = reinterpret_cast<RayRec*>(slot + P.tw_rays_off);
    X.nodes = reinterpret_cast<NodeRec*>(slot + P.tw_nodes_off);
    X.keys = STOCH ? reinterpret_cast<uint32_t*>(slot + P.tw_rng_off) : nullptr;
    TileLds* T = X.lds();
    Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
    const int D = P.max_depth, ns = P.spp > 0 ? P.spp * P.spp : 1;
    uint32_t my_pixels = 0;
    int prev_tile = -1;
    unsigned long long t_tile = 0;
    for (;;) {
        if (tid == 0) T->tile = atomicAdd(&P.tw_ctrl[0], 1u);
        __syncthreads();
        if ((int)T->tile >= P.n_tiles) {                         // workgroup-uniform
            if (P.tile_cost && tid == 0 && prev_tile >= 0) P.tile_cost[prev_tile] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_tile);
            break;
        }
        const int tile = P.tile_order ? (int)P.tile_order[T->tile] : (int)T->tile;     // (heaviest first, once measured)
        if (tid == 0 && (P.tile_cost || (kStamps && P.dbg_stamps))) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (P.tile_cost && prev_tile >= 0) P.tile_cost[prev_tile] = (uint32_t)(now - t_tile);
            if (kStamps && P.dbg_stamps) {                       // diagnostic: one record per TILE (0 start, 1 end, 2 workgroup)
                if (prev_tile >= 0) P.dbg_stamps[(size_t)prev_tile * 8 + 1] = now;
                P.dbg_stamps[(size_t)tile * 8] = now;
                P.dbg_stamps[(size_t)tile * 8 + 2] = blockIdx.x;
            }
            t_tile = now;
        }
        prev_tile = tile;
        X.tx = tile % P.tiles_x; X.ty = tile / P.tiles_x;
        const int f = batch_frame<BATCH>(P, X.ty * 16);          // (batches: the frame, and its rows in the planes)
        if (BATCH) X.oy = out_row<BATCH>(P, f, X.ty * 16);
        const int x = X.tx * 16 + (lane & 15);
        const int row = X.ty * 16 + wave * 4 + (lane >> 4);      // row in the compact local buffer
        const int y = image_row(P, BATCH ? row - f * P.frame_rows : row);
        const bool inside = x < P.res_x && y < P.res_y;
        const size_t p = (size_t)(BATCH ? X.oy + wave * 4 + (lane >> 4) : row) * P.res_x + x;
        if (P.spp > 0) { T->acc[3 * tid] = 0.0f; T->acc[3 * tid + 1] = 0.0f; T->acc[3 * tid + 2] = 0.0f; }
        for (int smp = 0; smp < ns; smp++) {
            if (tid < 2 * kMaxTileLevels) T->n_rays[tid] = 0u;   // n_rays and n_nodes are contiguous
            __syncthreads();
            // ---- trace: level 1 = this sample's camera rays (one per thread), level l >= 2 = the queue the
            // level above filled, shared by the four waves.  ONE call site for both, so that the per-node code
            // is instantiated once per kernel.
            for (int l = 1; l <= D; l++) {
                const uint32_t n = l == 1 ? kTilePx : T->n_rays[l];
                // Whole rounds of 4 x 64 rays, then the remainder.  With the work-sharing walk (scenes read from HBM) the
                // remainder is SPREAD over the four waves -- 40 queued rays are 10 per wave with 54 helper lanes each, not
                // one wave of 40 beside three idle ones: the levels of a heavy tile are short queues of long walks.
                constexpr bool kSpread = WALK == WALK_SHARED && !LDS;
                const uint32_t full = (kSpread && l > 1) ? (n / 256u) * 256u : n, rem = n - full;     // (not spread: the plain loop)
                const uint32_t per = (rem + 3u) / 4u;
                for (uint32_t base = (uint32_t)wave * 64u; base < full || (base == full + (uint32_t)wave * 64u && rem > 0u); base += 256u) {
                    const bool tail = base >= full;
                    const uint32_t i = tail ? full + (uint32_t)wave * per + lane : base + lane;
                    const bool in_batch = tail ? ((uint32_t)lane < per && i < n) : true;
                    bool valid; uint32_t link = (uint32_t)tid, rng = 0; float ior_1 = 1.0f;
                    Ray ray; ray.o = mk(0.0f, 0.0f, 0.0f); ray.d = mk(1.0f, 0.0f, 0.0f);
                    if (l == 1) {
                        valid = inside;
                        if (inside) ray = camera_ray<BATCH>(P, x, y, smp, f);
                        if (STOCH) rng = rng_mix(rng_mix(BATCH ? P.seed + (uint32_t)f : P.seed, (uint32_t)(y * P.res_x + x)), (uint32_t)smp);
                    } else {
                        valid = in_batch && i < n;
                        if (valid) {
                            load_ray(X.ray_slot(l, i), ray, ior_1, link);
                            if (STOCH) rng = X.keys[tile_ray_offset(l) + i];
                        }
                    }
                    const Hit h = find_closest<COUNT, WALK>(P, sv, ray, valid, tc, ctr);
                    if (l == 1 && smp == 0 && inside && P.hit_id) P.hit_id[p] = hit_id_of(h);
                    if (AOV && l == 1 && smp == 0) write_aov(P, sv, p, inside, ray, h);        // wave-uniform
                    const NodeOut o = shade_hit<COUNT, WALK, typename View<LDS>::type, STOCH, SCHLICK>(P, sv, ray, h, valid, l, ior_1, tc,
                                                                                              ctr, rng, smp);
                    tile_emit<BATCH>(P, X, l, valid, link, ior_1, o);
                }
                __syncthreads();
            }
            for (int l = D - 1; l >= 1; l--) {                   // ---- resolve: RT/main.cpp:719, deepest level first
                const uint32_t n = T->n_nodes[l];
                for (uint32_t i = (uint32_t)tid; i < n; i += 256u) {
                    uint32_t link;
                    const V3 ret = resolve_node(sv, X.nodes + tile_node_offset(l) + i, link);
                    tile_deliver<BATCH>(P, X, l, link, ret);
                }
                __syncthreads();
            }
        }
        if (P.spp > 0 && inside) {                               // "color / (4 * 4)", RT/main.cpp:800
            const float* a = T->acc + 3 * tid;
            write_pixel(P, p, div16(mk(a[0], a[1], a[2])));
        }
        my_pixels += inside ? 1u : 0u;
    }
    if (kStamps && P.dbg_stamps && tid == 0 && prev_tile >= 0) P.dbg_stamps[(size_t)prev_tile * 8 + 1] = __builtin_amdgcn_s_memrealtime();
    flush_counters<COUNT>(P, ctr, my_pixels);
    // the last workgroup out re-arms the tile counter for the next launch on this workspace (the frame
    // is self-contained on the device: safe to capture into a HIP graph and replay)
    if (tid == 0 && atomicAdd(&P.tw_ctrl[1], 1u) == gridDim.x - 1u) {
        atomicExch(&P.tw_ctrl[0], 0u);
        atomicExch(&P.tw_ctrl[1], 0u);
    }
}


// ------------------------------------------------------------------ TREE schedule
// shade-stack frame: 12 dwords.  STRIDE 64: in LDS, [field][lane] (scenes rendered from an LDS copy, and trees deeper
// than 8 levels).  STRIDE 1: in the lane's PRIVATE memory (scratch) -- scenes read from HBM are bound by how many waves
// are resident to hide fetch latency, frames are touched once per tree node, and 9 KB of LDS per wave for three of them
// held the dragon to 10 waves per CU: 1.81 -> 1.55 ms with the frames in scratch (16-25 waves per CU).
template <int STRIDE>
struct Frames {
    uint32_t* base;   // this lane's field-0 of frame-0; field stride STRIDE, frame stride 12 * STRIDE
    __device__ __forceinline__ uint32_t& f(int frame, int field) { return base[(frame * 12 + field) * STRIDE]; }
    __device__ __forceinline__ void put3(int frame, int field, V3 v) {
        f(frame, field) = __float_as_uint(v.x); f(frame, field + 1) = __float_as_uint(v.y);
        f(frame, field + 2) = __float_as_uint(v.z);
    }
    __device__ __forceinline__ V3 get3(int frame, int field) {
        return mk(__uint_as_float(f(frame, field)), __uint_as_float(f(frame, field + 1)),
                  __uint_as_float(f(frame, field + 2)));
    }
};
// frame fields.  While the reflection child runs, A/RD/IOR hold the parked refraction ray;
// afterwards A holds reflection_color * KR * specColor.
enum { FR_C = 0, FR_KR = 3, FR_META = 4, FR_A = 5, FR_RD = 8, FR_IOR = 11 };
#define FR_HAS_REFR 0x40000000u
#define FR_WAIT_REFR 0x80000000u

// A node with children: push its frame and go on with its first child (the reflection ray, if it has one).
// (fr by value and, below, a flag with break: as references / an early return the tree kernels spill more registers)
template <class SV, class FR>
__device__ __forceinline__ void push_frame(const SV& sv, FR fr, int& fsp, const NodeOut& o, Ray& ray, float& ior_1) {
    const V3 zero = mk(0.0f, 0.0f, 0.0f);
    fr.put3(fsp, FR_C, o.color);
    fr.f(fsp, FR_KR) = __float_as_uint(o.KR);
    if (o.has_refl) {
        fr.f(fsp, FR_META) = o.mat | (o.has_refr ? FR_HAS_REFR : 0u);
        fr.put3(fsp, FR_A, o.refr.o);
        fr.put3(fsp, FR_RD, o.refr.d);
        fr.f(fsp, FR_IOR) = __float_as_uint(o.newIor);
        ray = o.refl;                                    // ior_1 unchanged
    } else {
        Mtl M = load_material(sv, o.mat);
        fr.f(fsp, FR_META) = o.mat | FR_WAIT_REFR;
        fr.put3(fsp, FR_A, cmul(mul(zero, o.KR), M.spec));
        ray = o.refr; ior_1 = o.newIor;
    }
    fsp++;
}
// Return path of a finished node: combine ret into its parents (RT/main.cpp:719) until one of them still has its
// refraction child to trace -- then ray / ior_1 are that child's and the result is true -- or the stack is empty.
template <class SV, class FR>
__device__ __forceinline__ bool pop_frames(const SV& sv, FR fr, int& fsp, V3& ret, Ray& ray, float& ior_1) {
    const V3 zero = mk(0.0f, 0.0f, 0.0f);
    bool resumed = false;
    while (fsp > 0) {
        const int k = fsp - 1;
        const uint32_t meta = fr.f(k, FR_META);
        const V3 C = fr.get3(k, FR_C);
        const float KR = __uint_as_float(fr.f(k, FR_KR));
        if (!(meta & FR_WAIT_REFR)) {
            Mtl M = load_material(sv, meta & 0x3FFFFFFFu);
            const V3 A = cmul(mul(ret, KR), M.spec);
            if (meta & FR_HAS_REFR) {
                ray.o = fr.get3(k, FR_A);
                ray.d = fr.get3(k, FR_RD);
                ior_1 = __uint_as_float(fr.f(k, FR_IOR));
                fr.put3(k, FR_A, A);
                fr.f(k, FR_META) = meta | FR_WAIT_REFR;
                resumed = true;
                break;
            }
            ret = add(C, add(A, mul(zero, 1.0f - KR)));
        } else {
            const V3 A = fr.get3(k, FR_A);
            ret = add(C, add(A, mul(ret, 1.0f - KR)));
        }
        fsp--;
    }
    return resumed;
}

// One primary ray's whole tree: rayTracing(ray, 1, 1.0) of RT/main.cpp:530-721, iterative.
// AOV builds: aov_p() is the pixel's place in the AOV planes, written from the primary hit of the tree that is asked to
// (aov: sample 0's)
template <bool COUNT, bool GRID, class SV, class FR, bool SCHLICK = false, bool AOV = false, class PX>
__device__ __forceinline__ V3 trace_tree(const LaunchParams& P, const SV& sv, Ray ray, const TravCtx& tc, FR fr,
                                         int32_t& primary_hit, Ctr& ctr, bool aov, PX aov_p) {
    int fsp = 0;              // frames on the stack == depth - 1
    float ior_1 = 1.0f;
    bool first = true;
    V3 ret = mk(0.0f, 0.0f, 0.0f);
    for (;;) {
        Hit h = find_closest<COUNT, GRID ? WALK_GRID : WALK_LANE>(P, sv, ray, true, tc, ctr);
        if (first) {
            primary_hit = hit_id_of(h); first = false;
            if (AOV && aov) write_aov(P, sv, aov_p(), true, ray, h);
        }
        NodeOut o = shade_hit<COUNT, GRID ? WALK_GRID : WALK_LANE, SV, false, SCHLICK>(P, sv, ray, h, true, fsp + 1, ior_1, tc, ctr);
        if (!o.terminal) {
            push_frame(sv, fr, fsp, o, ray, ior_1);
            continue;
        }
        ret = o.ret;
        if (!pop_frames(sv, fr, fsp, ret, ray, ior_1)) return ret;
    }
}

// The same trees with the wave's lanes in ONE loop (work-sharing walk, WALK_SHARED): every iteration all 64 lanes reach
// find_closest() / shade_hit() together -- a lane whose pixel is finished (or outside the image) comes along as a helper
// of the others' walks -- and a lane that finishes a sample's tree starts its next sample at once.
template <bool COUNT, class SV, class FR, bool SCHLICK = false, bool BATCH = false, bool AOV = false, class PX>
__device__ __forceinline__ void trace_trees_shared(const LaunchParams& P, const SV& sv, int x, int y, int f, bool valid, const TravCtx& tc, FR fr,
                                                   V3& color, int32_t& hid, Ctr& ctr, PX aov_p) {
    const int ns = P.spp > 0 ? P.spp * P.spp : 1;
    const V3 zero = mk(0.0f, 0.0f, 0.0f);
    int smp = 0, fsp = 0;
    float ior_1 = 1.0f;
    bool alive = valid, first = true;
    V3 acc = zero;
    Ray ray; ray.o = zero; ray.d = mk(1.0f, 0.0f, 0.0f);
    if (alive) ray = camera_ray<BATCH>(P, x, y, 0, f);
    while (__ballot(alive) != 0) {
        const Hit h = find_closest<COUNT, WALK_SHARED>(P, sv, ray, alive, tc, ctr);
        if (AOV && __ballot(alive && first && smp == 0) != 0) write_aov(P, sv, aov_p(), alive && first && smp == 0, ray, h);   // wave-uniform
        if (alive && first) { if (smp == 0) hid = hit_id_of(h); first = false; }
        const NodeOut o = shade_hit<COUNT, WALK_SHARED, SV, false, SCHLICK>(P, sv, ray, h, alive, fsp + 1, ior_1, tc, ctr);
        if (!alive) continue;
        if (!o.terminal) {
            push_frame(sv, fr, fsp, o, ray, ior_1);
            continue;
        }
        V3 ret = o.ret;
        if (pop_frames(sv, fr, fsp, ret, ray, ior_1)) continue;
        const V3 c = clampc(ret);                                // "rayTracing(...).clamp()" of this sample
        if (P.spp == 0) { color = c; alive = false; continue; }
        acc = add(acc, c);                                       // RT/main.cpp:797, in sample order
        smp++;
        if (smp < ns) { ray = camera_ray<BATCH>(P, x, y, smp, f); fsp = 0; ior_1 = 1.0f; }
        else { color = div16(acc); alive = false; }
    }
}

// PRIV = dwords of private memory for the frames (12 per level below the first), 0 = frames in LDS
template <bool COUNT, bool LDS, int OCC, bool GRID = false, int PRIV = 0, bool SHARED = false, bool SCHLICK = false, bool BATCH = false, bool AOV = false>
__global__ __launch_bounds__(LDS ? 256 : 64) P3D_OCC(OCC) void whitted_tree_kernel(const LaunchParams P) {
    const typename View<LDS>::type sv = View<LDS>::make_shading(P);
    const int lane = threadIdx.x & 63;
    int x, y, row, f, tile;
    const bool in_image = tile_pixel<!LDS, BATCH>(P, x, y, row, f, &tile);
    if (SHARED ? __ballot(in_image) == 0 : !in_image) return;   // no barriers below: early exit is safe
    const unsigned long long t_tile = (!LDS && P.tile_cost) ? __builtin_amdgcn_s_memrealtime() : 0ull;
    stamp(P, tile, 0);
    uint32_t priv[PRIV > 0 ? PRIV : 1];
    uint32_t* wbase;
    const uint32_t frame_dwords = PRIV > 0 ? 0u : (uint32_t)(P.max_depth > 1 ? (P.max_depth - 1) : 1) * 12 * 64;
    const TravCtx st = wave_stack<LDS>(P, frame_dwords, &wbase);
    Frames<(PRIV > 0) ? 1 : 64> fr;
    if constexpr (PRIV > 0) fr.base = priv; else fr.base = wbase + P.trav_stack_dwords + lane;

    Ctr ctr = {0, 0, 0, 0, 0, 0, 0};
    V3 color = mk(0.0f, 0.0f, 0.0f);
    int32_t hid = -1;
    // the pixel's place in the AOV planes (the final write's p), formed only where an AOV build writes them
    const auto aov_p = [&]() { return (size_t)out_row<BATCH>(P, f, row) * P.res_x + x; };
    if constexpr (SHARED) {
        trace_trees_shared<COUNT, typename View<LDS>::type, decltype(fr), SCHLICK, BATCH, AOV>(P, sv, x, y, f, in_image, st, fr, color, hid, ctr, aov_p);
    } else if (P.spp == 0) {                                    // RT/main.cpp:756-775
        color = clampc(trace_tree<COUNT, GRID, typename View<LDS>::type, decltype(fr), SCHLICK, AOV>(P, sv, camera_ray<BATCH>(P, x, y, 0, f), st, fr, hid, ctr, true, aov_p));
    } else {                                             // RT/main.cpp:776-801
        const int ns = P.spp * P.spp;
        for (int s = 0; s < ns; s++) {
            int32_t h2 = -1;
            V3 c = clampc(trace_tree<COUNT, GRID, typename View<LDS>::type, decltype(fr), SCHLICK, AOV>(P, sv, camera_ray<BATCH>(P, x, y, s, f), st, fr, h2, ctr, s == 0, aov_p));
            color = add(color, c);
            if (s == 0) hid = h2;
        }
        color = div16(color);
    }
    if (!SHARED || in_image) {      // (shared walk: lanes outside the image came along as helpers)
        const size_t p = (size_t)out_row<BATCH>(P, f, row) * P.res_x + x;
        write_pixel(P, p, color);
        if (P.hit_id) P.hit_id[p] = hid;
        flush_counters<COUNT>(P, ctr, 1u);
    }
    stamp(P, tile, 4);              // (diagnostic; the wave has reconverged here: its slowest lane is done)
    if (!LDS && P.tile_cost && threadIdx.x == 0) P.tile_cost[tile] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_tile);
}

// per-column / per-row factors of the pixel-centre camera rays (one launch per resolution)
__global__ void raygen_table_kernel(float* fx, float* fy, int res_x, int res_y) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < res_x) fx[i] = fdiv((float)i + 0.5f, (float)res_x) - 0.5f;      // pixel.x / res_x - 0.5f
    if (i < res_y) fy[i] = fdiv((float)i + 0.5f, (float)res_y) - 0.5f;
}

// ------------------------------------------------------------------ rank-0 de-interleave
// T = uint4 when rows, strides and pointers are 16-byte multiples (1920 x 3 B rows are), else uint8_t.
// blockIdx.y = frame of a batch (frame f of rank r starts at r * rank_stride + f * in_stride).
template <class T>
__global__ void deinterleave_kernel(const uint8_t* __restrict__ gathered, uint8_t* __restrict__ frames,
                                    size_t row_bytes, int res_y, int row_block, int world, size_t rank_stride,
                                    size_t in_stride, size_t out_stride) {
    const size_t row_units = row_bytes / sizeof(T);
    const size_t total = row_units * res_y;
    const uint8_t* src = gathered + (size_t)blockIdx.y * in_stride;
    uint8_t* dst = frames + (size_t)blockIdx.y * out_stride;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        size_t y = i / row_units, off = (i - y * row_units) * sizeof(T);
        int blk = (int)(y / row_block);
        int rank = blk % world, lblk = blk / world;
        size_t lrow = (size_t)lblk * row_block + (y - (size_t)blk * row_block);
        *reinterpret_cast<T*>(dst + y * row_bytes + off) =
            *reinterpret_cast<const T*>(src + (size_t)rank * rank_stride + lrow * row_bytes + off);
    }
}

// ------------------------------------------------------------------ launchers (host)
static size_t scene_lds_bytes(const LaunchParams& P, bool lds) { return lds ? (size_t)P.blob_quads * 16 : 0; }
// frames of the tree kernel: private memory for scenes read from HBM up to depth 8, LDS otherwise
static int tree_private_dwords(const LaunchParams& P, bool lds) {
    if (lds || P.accel == 1) return 0;
    return P.max_depth <= 4 ? 36 : (P.max_depth <= 8 ? 84 : 0);
}
size_t tree_kernel_lds_bytes(const LaunchParams& P, bool lds) {
    if (tree_private_dwords(P, lds)) return scene_lds_bytes(P, lds) + (size_t)P.trav_stack_dwords * 4 * P.wg_waves;
    int frames = P.max_depth > 1 ? (P.max_depth - 1) : 1;
    size_t wave_dwords = (size_t)P.trav_stack_dwords + (size_t)frames * 12 * 64;
    return scene_lds_bytes(P, lds) + wave_dwords * 4 * P.wg_waves;
}
size_t wavefront_lds_bytes(const LaunchParams& P, bool lds) {
    return scene_lds_bytes(P, lds) + (size_t)P.trav_stack_dwords * 4 * P.wg_waves;
}

// Kernel variants.  The host asks with a KernelVariant (p3d_launch.h); not every combination of its switches is built.
// Per kernel family: canonical_*() maps a request to the build that serves it, built_*() is the one statement of which
// builds exist, and a table over all combinations holds the kernels' pointers -- nullptr where nothing is built.
using KernelFn = void (*)(const LaunchParams);
constexpr int kOccs[3] = {1, 5, 6};               // register budgets: the compiler's default, 5 and 6 waves per SIMD
constexpr int kPrivs[3] = {0, 36, 84};            // tree kernel: dwords of private frames (0: frames in LDS)
constexpr int kLevelVariants = 2 * 2 * 4 * 3 * 2 * 2 * 2 * 2, kTreeVariants = kLevelVariants * 3;

// position of a canonical variant (occ is 1, 5 or 6) in a family's table, and the variant at a position.  A walk that is
// none of the four has no position, so the launch fails with hipErrorInvalidDeviceFunction; no caller passes one.
constexpr int variant_index(const KernelVariant& v) {
    if (v.walk < WALK_LANE || v.walk > WALK_SHARED) return -1;
    return ((((((v.count * 2 + v.lds) * 4 + v.walk) * 3 + (v.occ == 5 ? 1 : v.occ == 6 ? 2 : 0)) * 2 + v.stoch) * 2 + v.schlick) * 2 + v.batch) * 2 + v.aov;
}
constexpr KernelVariant variant_at(int i) {
    KernelVariant v;
    v.aov = i % 2; i /= 2; v.batch = i % 2; i /= 2; v.schlick = i % 2; i /= 2; v.stoch = i % 2; i /= 2;
    v.occ = kOccs[i % 3]; i /= 3; v.walk = i % 4; i /= 4; v.lds = i % 2; v.count = i / 2;
    return v;
}

// The level kernels: canonical_level() and built_level() of p3d_kernel_variant.h.
// The tree kernel: GRID = grid walk, SHARED = shared walk (the packet walk is the lane walk here), PRIV from the depth
// (tree_private_dwords); the schedule never runs features with random draws.
constexpr int canonical_priv(const KernelVariant& v, int priv) {
    return (v.lds || v.walk == WALK_GRID || (priv != 36 && priv != 84)) ? 0 : priv;      // LDS scenes and the grid walk: frames in LDS
}
constexpr KernelVariant canonical_tree(KernelVariant v, int priv) {
    v.stoch = false;
    if (v.walk == WALK_PACKET || (v.walk == WALK_SHARED && v.lds)) v.walk = WALK_LANE;
    if ((v.occ != 5 && v.occ != 6) || v.walk == WALK_GRID || v.count || v.schlick || v.batch || v.aov || (v.walk == WALK_SHARED && priv == 0)) v.occ = 1;
    return v;
}
constexpr bool built_tree(const KernelVariant& v, int priv) {
    if (v.stoch || v.walk == WALK_PACKET || (v.walk == WALK_SHARED && v.lds)) return false;
    if (priv != 0 && (v.lds || v.walk == WALK_GRID)) return false;
    if (v.occ == 1) return true;
    return v.walk != WALK_GRID && !v.count && !v.schlick && !v.batch && !v.aov && !(v.walk == WALK_SHARED && priv == 0);
}

// Every request reaches a build, and nothing is built that no request reaches: checked for the variants at positions
// [first, last) (in four parts below: one constant evaluation over all of them passes the compiler's step limit).
constexpr bool variants_are_consistent(int first, int last) {
    constexpr int raw_occs[] = {0, 1, 5, 6, 8}, raw_privs[] = {0, 36, 84, 12};
    for (int i = first; i < last; i++) {
        for (int occ : raw_occs) {
            KernelVariant v = variant_at(i);
            v.occ = occ;
            v.tiles = kMaxPrimaryTiles;                 // (only the level-1 kernel has the variant)
            if (!built_level(canonical_level(v, Level::Tile), Level::Tile) || !built_level(canonical_level(v, Level::Secondary), Level::Secondary)) return false;
            if (!built_level(canonical_level(v, Level::Rays), Level::Rays)) return false;
            if (!built_level(canonical_level(v, Level::Occlusion), Level::Occlusion)) return false;
            if (!built_level(canonical_level(v, Level::AmbientOcclusion), Level::AmbientOcclusion)) return false;
            if (!built_level(canonical_level(v, Level::IndirectDiffuse), Level::IndirectDiffuse)) return false;
            if (!built_level(canonical_level(v, Level::IndirectPaths), Level::IndirectPaths)) return false;
            for (int tiles = 0; tiles <= kMaxPrimaryTiles + 1; tiles++) {
                v.tiles = tiles;
                if (!built_level(canonical_level(v, Level::Primary), Level::Primary)) return false;
            }
            v.tiles = 1;
            for (int priv : raw_privs)
                if (!built_tree(canonical_tree(v, canonical_priv(v, priv)), canonical_priv(v, priv))) return false;
        }
        KernelVariant v = variant_at(i);
        for (v.tiles = kMaxPrimaryTiles; v.tiles >= 1; v.tiles--)
            for (Level k : {Level::Primary, Level::Secondary, Level::Tile, Level::Rays, Level::Occlusion, Level::AmbientOcclusion, Level::IndirectDiffuse, Level::IndirectPaths})
                if (built_level(v, k) && !(canonical_level(v, k) == v)) return false;
        v.tiles = 1;
        for (int priv : kPrivs)
            if (built_tree(v, priv) && !(canonical_priv(v, priv) == priv && canonical_tree(v, priv) == v)) return false;
    }
    return true;
}
#define P3D_VARIANTS_CONSISTENT(q)                                                                      \
    static_assert(variants_are_consistent((q) * kLevelVariants / 4, ((q) + 1) * kLevelVariants / 4), \
                  "a kernel request maps to a variant that is not built, or a built variant is unreachable")
P3D_VARIANTS_CONSISTENT(0); P3D_VARIANTS_CONSISTENT(1); P3D_VARIANTS_CONSISTENT(2); P3D_VARIANTS_CONSISTENT(3);
#undef P3D_VARIANTS_CONSISTENT

using RaysKernelFn = void (*)(const LaunchParams, const RayStreamIO);
using OcclusionKernelFn = void (*)(const LaunchParams, const OcclusionIO);
template <Level KERNEL> struct LevelKernels {       // position: variant_index * per_variant + (TILES - 1)
    using Fn = std::conditional_t<KERNEL == Level::Rays, RaysKernelFn, std::conditional_t<KERNEL == Level::Occlusion, OcclusionKernelFn, KernelFn>>;
    static constexpr Level level = KERNEL;
    static constexpr int per_variant = KERNEL == Level::Primary ? kMaxPrimaryTiles : 1;
    static constexpr int n = kLevelVariants * per_variant;
    static constexpr KernelVariant at(int i) { KernelVariant v = variant_at(i / per_variant); v.tiles = 1 + i % per_variant; return v; }
    static constexpr bool built(int i) { return built_level(at(i), KERNEL); }
    template <int I> static constexpr Fn fn() {
        constexpr KernelVariant v = at(I);
        if constexpr (KERNEL == Level::Primary && v.tiles > 1) return wf_primary_kernel_tiles<v.walk, v.occ, v.tiles>;
        else if constexpr (KERNEL == Level::Primary) return wf_primary_kernel<v.count, v.lds, v.walk, v.occ, v.stoch, v.schlick, v.batch, v.aov>;
        else if constexpr (KERNEL == Level::Secondary) return wf_secondary_kernel<v.count, v.lds, v.walk, v.occ, v.stoch, v.schlick>;
        else if constexpr (KERNEL == Level::Rays) return wf_rays_kernel<v.lds, v.walk, v.occ>;
        else if constexpr (KERNEL == Level::Occlusion) return wf_occlusion_kernel<v.lds, v.walk, v.occ>;
        else return wf_tile_kernel<v.count, v.lds, v.walk, v.occ, v.stoch, v.schlick, v.batch, v.aov>;
    }
};
struct TreeKernels {                                // position: variant_index * 3 + position of PRIV in kPrivs
    using Fn = KernelFn;
    static constexpr int n = kTreeVariants;
    static constexpr bool built(int i) { return built_tree(variant_at(i / 3), kPrivs[i % 3]); }
    template <int I> static constexpr KernelFn fn() {
        constexpr KernelVariant v = variant_at(I / 3);
        return whitted_tree_kernel<v.count, v.lds, v.occ, v.walk == WALK_GRID, kPrivs[I % 3], v.walk == WALK_SHARED, v.schlick, v.batch, v.aov>;
    }
};
// the walk over a family's positions: a kernel is instantiated only where built() says so
template <class K, int I> constexpr typename K::Fn variant_fn() {
    if constexpr (K::built(I)) return K::template fn<I>();
    else return nullptr;
}
template <class K, int... I> static const void* kernel_lookup(int i, std::integer_sequence<int, I...>) {
    static constexpr typename K::Fn table[] = {variant_fn<K, I>()...};
    return i >= 0 && i < K::n ? reinterpret_cast<const void*>(table[i]) : nullptr;
}
template <class K> static const void* kernel_at(int i) { return kernel_lookup<K>(i, std::make_integer_sequence<int, K::n>{}); }

KernelVariant level_variant(KernelVariant v, Level k) { return canonical_level(v, k); }
template <class K> static const void* level_kernel(const KernelVariant& v) {
    const KernelVariant served = canonical_level(v, K::level);
    const int i = variant_index(served);
    return i < 0 ? nullptr : kernel_at<K>(i * K::per_variant + served.tiles - 1);
}
static const void* tree_kernel(const LaunchParams& P, const KernelVariant& v) {
    const int priv = canonical_priv(v, tree_private_dwords(P, v.lds));
    const int i = variant_index(canonical_tree(v, priv));
    return i < 0 ? nullptr : kernel_at<TreeKernels>(i * 3 + (priv == 36 ? 1 : priv == 84 ? 2 : 0));
}
// A launch with more dynamic LDS than the 64 KiB default says so first.  Any kernel can need it: the stacks grow with the
// depth of the BVH (a device-built tree over clustered centroids is a chain of up to 96 levels, bvh_device.hip), and the
// four waves of a workgroup that renders from an LDS copy of the scene each have one.  The limit is a maximum, so the
// largest one set for a kernel on a device is remembered and the runtime is asked only to raise it further.
hipError_t allow_lds(const void* fn, size_t shmem) {
    if (shmem <= 64 * 1024) return hipSuccess;
    static std::mutex lock;
    static std::map<std::pair<int, const void*>, size_t> raised;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> guard(lock);
    size_t& limit = raised[{dev, fn}];
    if (shmem <= limit) return hipSuccess;
    if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)) == hipSuccess) limit = shmem;
    return e;
}
static hipError_t launch_by_pointer(const void* fn, const LaunchParams& P, dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
    if (!fn) return hipErrorInvalidDeviceFunction;
    hipError_t e = allow_lds(fn, shmem);
    if (e != hipSuccess) return e;
    LaunchParams Pc = P;
    void* args[] = {&Pc};
    return hipLaunchKernel(fn, grid, block, args, shmem, stream);
}
// workgroups of `fn` that can be resident on the whole device
static hipError_t resident_blocks(const void* fn, int block, size_t shmem, int* blocks) {
    if (!fn) return hipErrorInvalidDeviceFunction;
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e = allow_lds(fn, shmem);
    if (e != hipSuccess) return e;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, shmem)) != hipSuccess) return e;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    *blocks = (per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1);
    return hipSuccess;
}

hipError_t launch_tree(const LaunchParams& P, const KernelVariant& v, hipStream_t stream) {
    return launch_by_pointer(tree_kernel(P, v), P, dim3((unsigned)P.grid_blocks), dim3(64 * P.wg_waves), tree_kernel_lds_bytes(P, v.lds), stream);
}
hipError_t launch_wf_primary(const LaunchParams& P, const KernelVariant& v, hipStream_t stream) {
    // identity tile map and no learned order: a 2-D grid, blockIdx = (tile column, tile row) -- see tile_pixel() and
    // primary_grid() (LDS scenes only: the kernels of scenes read from HBM number their tiles through the learned order)
    const KernelVariant served = served_primary(v, P.tiles_x, P.wf_tile_rows, P.n_tiles, P.xcd_chunk);
    const PrimaryGrid g = primary_grid(served, P.tiles_x, P.wf_tile_rows, P.n_tiles, P.xcd_chunk, P.grid_blocks);
    return launch_by_pointer(level_kernel<LevelKernels<Level::Primary>>(served), P, dim3(g.x, g.y), dim3(64 * P.wg_waves), wavefront_lds_bytes(P, v.lds), stream);
}
// level 1 of a ray stream: one workgroup per 64 * wg_waves rays of the band (wf_tile_rows workgroups)
hipError_t launch_wf_rays(const LaunchParams& P, const RayStreamIO& R, const KernelVariant& v, hipStream_t stream) {
    const void* fn = level_kernel<LevelKernels<Level::Rays>>(v);
    if (!fn) return hipErrorInvalidDeviceFunction;
    const size_t shmem = wavefront_lds_bytes(P, v.lds);
    hipError_t e = allow_lds(fn, shmem);
    if (e != hipSuccess) return e;
    LaunchParams Pc = P;
    RayStreamIO Rc = R;
    void* args[] = {&Pc, &Rc};
    return hipLaunchKernel(fn, dim3((unsigned)P.wf_tile_rows), dim3(64 * P.wg_waves), args, shmem, stream);
}
// p3d_occluded: one workgroup per 64 * wg_waves segments (wf_occlusion_kernel)
hipError_t launch_wf_occlusion(const LaunchParams& P, const OcclusionIO& R, const KernelVariant& v, hipStream_t stream) {
    const void* fn = level_kernel<LevelKernels<Level::Occlusion>>(v);
    if (!fn) return hipErrorInvalidDeviceFunction;
    const size_t shmem = wavefront_lds_bytes(P, v.lds);
    hipError_t e = allow_lds(fn, shmem);
    if (e != hipSuccess) return e;
    LaunchParams Pc = P;
    OcclusionIO Rc = R;
    void* args[] = {&Pc, &Rc};
    const unsigned per_batch = 64u * (unsigned)P.wg_waves;
    return hipLaunchKernel(fn, dim3((R.count + per_batch - 1) / per_batch), dim3(per_batch), args, shmem, stream);
}
hipError_t launch_wf_secondary(const LaunchParams& P, const KernelVariant& v, unsigned waves, hipStream_t stream) {
    return launch_by_pointer(level_kernel<LevelKernels<Level::Secondary>>(v), P, dim3((waves + P.wg_waves - 1) / P.wg_waves),
                             dim3(64 * P.wg_waves), wavefront_lds_bytes(P, v.lds), stream);
}
// waves of the deeper-level kernel that can be resident on the device at once (LDS-scene variants: 256-thread workgroups)
hipError_t wf_resident_waves(const LaunchParams& P, const KernelVariant& v, unsigned* waves) {
    int blocks = 0;
    hipError_t e = resident_blocks(level_kernel<LevelKernels<Level::Secondary>>(v), 64 * P.wg_waves, wavefront_lds_bytes(P, v.lds), &blocks);
    if (e == hipSuccess) *waves = (unsigned)(blocks * P.wg_waves);
    return e;
}
// tile schedule: 256-thread workgroups
size_t tile_kernel_lds_bytes(const LaunchParams& P, bool lds) {
    return scene_lds_bytes(P, lds) + (size_t)P.trav_stack_dwords * 4 * 4 + (sizeof(TileLds) + 15) / 16 * 16 + (lds ? (size_t)kTileLdsRayDwords * 4 : 0);
}
// workgroups of this variant that can be resident on the whole device (persistent grid size)
hipError_t tile_kernel_resident_blocks(const LaunchParams& P, const KernelVariant& v, int* blocks) {
    return resident_blocks(level_kernel<LevelKernels<Level::Tile>>(v), 256, tile_kernel_lds_bytes(P, v.lds), blocks);
}
hipError_t launch_wf_tile(const LaunchParams& P, const KernelVariant& v, unsigned blocks, hipStream_t stream) {
    return launch_by_pointer(level_kernel<LevelKernels<Level::Tile>>(v), P, dim3(blocks), dim3(256), tile_kernel_lds_bytes(P, v.lds), stream);
}


hipError_t launch_wf_resolve_fused(const LaunchParams& P, const ResolveLevels& R, unsigned shards, bool ray_stream, hipStream_t stream) {
    if (ray_stream) hipLaunchKernelGGL(wf_resolve_fused_kernel<true>, dim3(shards), dim3(1024), 0, stream, P, R);
    else hipLaunchKernelGGL(wf_resolve_fused_kernel<false>, dim3(shards), dim3(1024), 0, stream, P, R);
    return hipGetLastError();
}
hipError_t launch_wf_resolve(const LaunchParams& P, unsigned blocks, bool ray_stream, hipStream_t stream) {
    if (ray_stream) hipLaunchKernelGGL(wf_resolve_kernel<true>, dim3(blocks), dim3(256), 0, stream, P);
    else hipLaunchKernelGGL(wf_resolve_kernel<false>, dim3(blocks), dim3(256), 0, stream, P);
    return hipGetLastError();
}

// The pre-pass of a frame with a tile coverage mask (p3d_tile_coverage.h): workgroup ty makes tile row ty's words.  Lane i takes
// primitives i, i + 64, ... of the device-resident scene blob -- so the mask follows p3d_scene_update and p3d_scene_rebuild
// with nothing copied from the host -- and ORs the columns each can touch into the row's words in LDS; then the words are
// stored whole: no atomics on memory, nothing to clear beforehand, and no launch of the frame before this one reads them.
// The camera travels in the arguments, so a captured frame replays with the mask of the camera it was captured with.
__global__ __launch_bounds__(64) void tile_coverage_kernel(const TileCoverageJob J) {
    __shared__ uint32_t words[kCoverMaxRowWords];
    __shared__ uint32_t all;
    const int32_t ty = (int32_t)blockIdx.x;
    if (threadIdx.x < kCoverMaxRowWords) words[threadIdx.x] = 0u;
    if (threadIdx.x == 0) all = 0u;
    __syncthreads();
    const CoverCamera cam = cover_camera(J.eye, J.uw, J.vh, J.vz);
    const float4* q = reinterpret_cast<const float4*>(J.blob);
    const uint32_t n = J.n_spheres + J.n_tris + J.n_boxes;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        double pts[kCoverMaxPoints][3];
        CoverRow r;
        if (i < J.n_spheres + J.n_boxes) {
            double lo[3], hi[3];
            if (i < J.n_spheres) {
                const float4 s = q[J.off_spheres + i];                          // SphereRec
                lo[0] = (double)s.x - (double)s.w; lo[1] = (double)s.y - (double)s.w; lo[2] = (double)s.z - (double)s.w;
                hi[0] = (double)s.x + (double)s.w; hi[1] = (double)s.y + (double)s.w; hi[2] = (double)s.z + (double)s.w;
            } else {
                const uint32_t b = J.off_boxes + (i - J.n_spheres) * 2u;         // BoxRec
                const float4 mn = q[b], mx = q[b + 1];
                lo[0] = mn.x; lo[1] = mn.y; lo[2] = mn.z; hi[0] = mx.x; hi[1] = mx.y; hi[2] = mx.z;
            }
            cover_box_points(lo, hi, pts);
            r = cover_row<8>(cam, J.tiles, pts, ty);
        } else {
            const uint32_t t = J.off_tris + (i - J.n_spheres - J.n_boxes) * J.tri_quads;   // TriRec's test record
            const float4 a = q[t], b = q[t + 1], c = q[t + 2];
            const float p0[3] = {a.x, a.y, a.z}, e1[3] = {b.x, b.y, b.z}, e2[3] = {c.x, c.y, c.z};
            cover_triangle_points(p0, e1, e2, pts);
            r = cover_row<3>(cam, J.tiles, pts, ty);
        }
        if (r.all) atomicOr(&all, 1u);
        else if (r.any)
            for (uint32_t w = (uint32_t)(r.tx0 < 0 ? 0 : r.tx0) >> 5; w < J.row_words && (int32_t)(32u * w) <= r.tx1; w++)
                atomicOr(&words[w], cover_word_bits(r.tx0, r.tx1, w));
    }
    __syncthreads();
    const bool every = all != 0u || !cam.ok;
    uint32_t mine = 0u;
    if (threadIdx.x < J.row_words) {
        const uint32_t valid = cover_word_bits(0, J.tiles.tiles_x - 1, threadIdx.x);   // the row's tiles in this word
        mine = (every ? 0xFFFFFFFFu : words[threadIdx.x]) & valid;
        J.mask[(size_t)ty * J.row_words + threadIdx.x] = mine;
    }
    __syncthreads();
    if (threadIdx.x < kCoverMaxRowWords) words[threadIdx.x] = (uint32_t)__popc(mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t active = 0u;
        for (uint32_t w = 0; w < J.row_words; w++) active += words[w];
        J.status[ty] = active | (every ? kCoverAllFlag : 0u);
    }
}
hipError_t launch_tile_coverage(const TileCoverageJob& J, hipStream_t stream) {
    static_assert(kCoverMaxRowWords <= 64, "one lane per word of a row");
    if (J.row_words > kCoverMaxRowWords || J.tiles.tiles_y < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_coverage_kernel, dim3((unsigned)J.tiles.tiles_y), dim3(64), 0, stream, J);
    return hipGetLastError();
}

__global__ void clear_words_kernel(uint32_t* p, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
}
// Per-frame cameras of a batch, carried by the launch's own arguments (kFrameCamsPerLaunch records, 2 KiB): a stream capture
// bakes them into the graph, so a replay writes the cameras it was captured with, and no host buffer has to outlive the call.
constexpr int kFrameCamsPerLaunch = 16;
struct FrameCamChunk { FrameCam cam[kFrameCamsPerLaunch]; };
__global__ __launch_bounds__(256) void frame_cams_kernel(const FrameCamChunk c, FrameCam* dst, uint32_t n_floats) {
    for (uint32_t i = threadIdx.x; i < n_floats; i += blockDim.x)
        reinterpret_cast<float*>(dst)[i] = reinterpret_cast<const float*>(c.cam)[i];
}
hipError_t launch_frame_cams(FrameCam* dst, const FrameCam* cams, int n, hipStream_t stream) {
    for (int f0 = 0; f0 < n; f0 += kFrameCamsPerLaunch) {
        const int k = n - f0 < kFrameCamsPerLaunch ? n - f0 : kFrameCamsPerLaunch;
        FrameCamChunk c;
        memset(&c, 0, sizeof c);
        memcpy(c.cam, cams + f0, (size_t)k * sizeof(FrameCam));
        hipLaunchKernelGGL(frame_cams_kernel, dim3(1), dim3(256), 0, stream, c, dst + f0,
                           (uint32_t)(k * (sizeof(FrameCam) / sizeof(float))));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_clear_words(uint32_t* p, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(clear_words_kernel, dim3((n + 255) / 256 < 64 ? (n + 255) / 256 : 64), dim3(256), 0, stream, p, n);
    return hipGetLastError();
}

hipError_t launch_sum_samples(const LaunchParams& P, size_t first_px, size_t n_px, hipStream_t stream) {
    const unsigned blocks = (unsigned)std::min<size_t>((n_px + 255) / 256, 256 * 32);
    if (P.n_frames > 1) hipLaunchKernelGGL(sum_samples_kernel<true>, dim3(blocks ? blocks : 1), dim3(256), 0, stream, P, first_px, n_px);
    else hipLaunchKernelGGL(sum_samples_kernel<false>, dim3(blocks ? blocks : 1), dim3(256), 0, stream, P, first_px, n_px);
    return hipGetLastError();
}

hipError_t launch_raygen_table(float* fx, float* fy, int res_x, int res_y, hipStream_t stream) {
    int n = res_x > res_y ? res_x : res_y;
    hipLaunchKernelGGL(raygen_table_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fx, fy, res_x, res_y);
    return hipGetLastError();
}
hipError_t launch_deinterleave(const void* gathered, void* frames, int res_x, int res_y, int row_block,
                               int world, size_t rank_stride, int bpp, int n_frames, size_t in_stride,
                               size_t out_stride, hipStream_t stream) {
    const size_t row_bytes = (size_t)res_x * bpp;
    const bool wide = row_bytes % 16 == 0 && rank_stride % 16 == 0 && in_stride % 16 == 0 && out_stride % 16 == 0 &&
                      (uintptr_t)gathered % 16 == 0 && (uintptr_t)frames % 16 == 0;
    const size_t units = (wide ? row_bytes / 16 : row_bytes) * (size_t)res_y;
    const dim3 grid((unsigned)std::min<size_t>((units + 255) / 256, 2048), (unsigned)n_frames);
    if (wide)
        hipLaunchKernelGGL(deinterleave_kernel<uint4>, grid, dim3(256), 0, stream, (const uint8_t*)gathered, (uint8_t*)frames,
                           row_bytes, res_y, row_block, world, rank_stride, in_stride, out_stride);
    else
        hipLaunchKernelGGL(deinterleave_kernel<uint8_t>, grid, dim3(256), 0, stream, (const uint8_t*)gathered, (uint8_t*)frames,
                           row_bytes, res_y, row_block, world, rank_stride, in_stride, out_stride);
    return hipGetLastError();
}

bool kernels_have_stamps() { return kStamps; }
}  // namespace p3d
