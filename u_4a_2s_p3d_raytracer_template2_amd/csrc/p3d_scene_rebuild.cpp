// p3d_scene_rebuild.cpp -- p3d_scene_rebuild, p3d_scene_rebuild_with and p3d_scene_tree_cost of include/p3d_hip.h: the tree
// of a live scene handle is built again on the device (bvh_device.hip; builder 2: with bvh_ploc.hip's rounds, a wait each)
// from the primitive records the handle holds there, the leaves are typed and the records put into the new leaf order on
// the device too (scene_rebuild.hip).  Everything is enqueued on the scene's
// stream; the call waits for the old tree's cost (a handle that has f32 node pairs), for the number of leaf records, which
// sizes the new blob, and for the finished handle.
// Every allocation is made before anything of the handle changes, and what the handle held is freed after the last wait.
#include <cmath>
#include <cstring>

#include "p3d_scene_state.h"
#include "scene_flatten.h"
#include "scene_rebuild.h"
#include "scene_update.h"

using namespace p3d;

namespace {

// the f32 node pairs of the tree the handle walks, or nullptr: a handle read from HBM has none before its first update
const NodePair* f32_nodes(const p3d_scene* s) {
    if (s->lds_capable) return (const NodePair*)(s->blob.p + 4 * (size_t)s->off_nodes);
    return s->refit.ready ? (const NodePair*)s->refit.nodes.p : nullptr;
}

// SAH cost of the tree as it stands.  Synchronous.
int current_cost(p3d_scene* s, float* out) {
    const NodePair* nodes = f32_nodes(s);
    if (!nodes) { *out = s->stats.sah_cost; return P3D_OK; }       // never updated nor rebuilt: nothing has moved
    RawBuf word;
    HIP_TRY(word.ensure(sizeof(float)));
    HIP_TRY(hipMemsetAsync(word.p, 0, sizeof(float), s->stream));
    const BvhOptions bo;
    HIP_TRY(launch_tree_cost(nodes, (uint32_t)s->qnodes.n, s->blob.p, s->off_leaves, bo.cost_traverse, bo.cost_intersect, (float*)word.p, s->stream));
    HIP_TRY(hipMemcpyAsync(out, word.p, sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return P3D_OK;
}

template <typename T>
hipError_t alloc_devbuf(DevBuf<T>& b, size_t n) {
    hipError_t e = hipMalloc((void**)&b.p, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) b.n = n;
    return e;
}

size_t refit_bytes(const p3d_scene* s) {
    const p3d_scene::Refit& R = s->refit;
    return R.ready ? R.nodes.cap + R.parent.cap + R.arrived.cap + R.status.cap : 0;
}

}  // namespace

extern "C" int p3d_scene_tree_cost(p3d_scene* s, float* sah_cost) {
    if (!s || !sah_cost) return fail(P3D_ERR_ARG, "scene/sah_cost is NULL");
    HIP_TRY(hipSetDevice(s->device));
    if (stream_capturing(s->stream))
        return fail(P3D_ERR_STATE, "p3d_scene_tree_cost waits on the device: not while the stream is being captured");
    return current_cost(s, sah_cost);
}

extern "C" int p3d_scene_rebuild(p3d_scene* s, p3d_rebuild_info* info) { return p3d_scene_rebuild_with(s, 1u, info); }

extern "C" int p3d_scene_rebuild_with(p3d_scene* s, uint32_t builder, p3d_rebuild_info* info) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    if (builder != 1u && builder != 2u)
        return fail(P3D_ERR_ARG, "builder must be 1 (device LBVH) or 2 (device clustering): the host builder needs the host's geometry");
    if (s->cull_never_hit)
        return fail(P3D_ERR_STATE, "scene was built with cull_never_hit: a moved triangle may no longer be one no ray can hit; create a new handle");
    HIP_TRY(hipSetDevice(s->device));
    if (stream_capturing(s->stream))
        return fail(P3D_ERR_STATE, "p3d_scene_rebuild waits on the device and changes launch parameters: not while the stream is being captured");
    const uint32_t n_prims = (uint32_t)s->prim_map.n;
    const uint32_t n = s->stats.n_spheres + s->stats.n_triangles + s->stats.n_boxes;     // the bounded primitives
    float before = 0.0f;
    int rc = current_cost(s, &before);
    if (rc) return rc;
    auto report = [&](uint32_t rebuilt, float after) {
        if (!info) return;
        info->rebuilt = rebuilt;
        info->n_nodes = s->stats.n_nodes; info->n_leaves = s->stats.n_leaves; info->max_depth = s->stats.max_depth;
        info->sah_cost_before = before; info->sah_cost_after = after;
    };
    // scenes served from LDS, and scenes the creation path builds on the host either way, keep their tree
    if (s->lds_capable || n < 64) { report(0u, before); return P3D_OK; }

    const uint32_t L = (n + 1) / 2, n_nodes = L - 1;
    hipStream_t st = s->stream;
    // ---- allocations: scratch, then what the handle will hold
    size_t scan_bytes = 0, lbvh_bytes = 0;
    HIP_TRY(rebuild_scan_temp_bytes(std::max(n_prims, n), &scan_bytes, st));
    HIP_TRY(builder == 2u ? ploc_scratch_bytes(n, &lbvh_bytes, st) : lbvh_scratch_bytes(n, &lbvh_bytes, st));
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return at; };
    const size_t o_bounded = carve((size_t)n_prims * 4), o_pos = carve((size_t)n_prims * 4), o_prims = carve((size_t)n * sizeof(BuildPrim));
    const size_t o_refs = carve((size_t)n * 4), o_is_tri = carve((size_t)n * 4), o_is_sph = carve((size_t)n * 4);
    const size_t o_tri_idx = carve((size_t)n * 4), o_sph_idx = carve((size_t)n * 4);
    const size_t o_need = carve((size_t)L * 4), o_rec_idx = carve((size_t)L * 4);
    const size_t o_scan = carve(scan_bytes), o_lbvh = carve(lbvh_bytes);
    RawBuf pool, new_nodes, new_parent, new_arrived, new_status;
    DevBuf<QNode> new_qnodes; DevBuf<uint32_t> new_map, new_blob;
    HIP_TRY(pool.ensure(off));
    HIP_TRY(new_nodes.ensure((size_t)n_nodes * sizeof(NodePair)));
    HIP_TRY(new_parent.ensure((size_t)n_nodes * sizeof(int32_t)));
    HIP_TRY(new_arrived.ensure((size_t)n_nodes * sizeof(uint32_t)));
    HIP_TRY(new_status.ensure(kStatusWords * sizeof(uint32_t)));
    HIP_TRY(alloc_devbuf(new_qnodes, n_nodes));
    HIP_TRY(alloc_devbuf(new_map, n_prims));
    char* base = (char*)pool.p;
    RebuildScratch W;
    W.bounded = (uint32_t*)(base + o_bounded); W.pos = (uint32_t*)(base + o_pos); W.prims = (BuildPrim*)(base + o_prims);
    W.refs = (uint32_t*)(base + o_refs); W.is_tri = (uint32_t*)(base + o_is_tri); W.is_sph = (uint32_t*)(base + o_is_sph);
    W.tri_idx = (uint32_t*)(base + o_tri_idx); W.sph_idx = (uint32_t*)(base + o_sph_idx);
    W.need = (uint32_t*)(base + o_need); W.rec_idx = (uint32_t*)(base + o_rec_idx);
    W.scan_temp = base + o_scan; W.scan_temp_bytes = scan_bytes;

    // ---- the tree over the records as they are, and how its leaves are typed
    SceneRecords S;
    S.blob = s->blob.p; S.off_leaves = s->off_leaves; S.off_spheres = s->off_spheres; S.off_tris = s->off_tris;
    S.off_tri_normals = s->off_tri_normals; S.off_boxes = s->off_boxes; S.tri_quads = s->tri_quads;
    S.planes = s->planes.p; S.prim_map = s->prim_map.p; S.n_prims = n_prims;
    NodePair* nodes = (NodePair*)new_nodes.p;
    const BvhOptions bo;
    uint32_t* d_result = nullptr;
    HIP_TRY(launch_rebuild_prims(S, n, W, st));
    PlocInfo ploc;
    if (builder == 2u) HIP_TRY(ploc_enqueue(W.prims, n, bo, nodes, W.refs, base + o_lbvh, &d_result, &ploc, st));   // waits once per round
    else HIP_TRY(lbvh_enqueue(W.prims, n, bo, nodes, W.refs, base + o_lbvh, &d_result, st));
    HIP_TRY(launch_rebuild_type(n, W, st));
    uint32_t result[2] = {0, 0}, last_rec = 0, last_need = 0;
    float root[kStatusRootFloats];
    HIP_TRY(hipMemcpyAsync(result, d_result, sizeof result, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_rec, W.rec_idx + (L - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_need, W.need + (L - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(root, nodes, sizeof root, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    BvhStats bs;
    lbvh_stats(n, result, bs);
    const uint32_t n_leaf_recs = 1u + last_rec + last_need;        // leaf 0: the empty leaf
    if (n_leaf_recs >= (1u << kLeafKindShift)) return fail(P3D_ERR_LIMIT, "too many mixed-type leaves");

    // ---- the new blob: creation's section order
    BlobSections N;
    uint32_t quads = 0;
    auto section = [&](size_t bytes) { const uint32_t at = quads; quads += (uint32_t)std::max<size_t>((bytes + 15) / 16, 1); return at; };
    const size_t mat_bytes = (size_t)s->n_materials * sizeof(MaterialRec);
    (void)section((size_t)s->off_leaves * 16);                     // powf's tables lead the blob
    N.off_leaves = section((size_t)n_leaf_recs * sizeof(LeafRec));
    N.off_spheres = section((size_t)s->stats.n_spheres * sizeof(SphereRec));
    N.off_sphere_meta = section((size_t)s->stats.n_spheres * sizeof(PrimMeta));
    N.off_tris = section((size_t)s->stats.n_triangles * 16 * s->tri_quads);
    N.off_tri_normals = section((size_t)s->stats.n_triangles * 16);
    N.off_boxes = section((size_t)s->stats.n_boxes * sizeof(BoxRec));
    N.off_mats = section(mat_bytes);
    N.tri_quads = s->tri_quads;
    HIP_TRY(alloc_devbuf(new_blob, (size_t)quads * 4));
    HIP_TRY(hipMemsetAsync(new_blob.p, 0, (size_t)quads * 16, st));
    HIP_TRY(hipMemcpyAsync(new_blob.p, s->blob.p, (size_t)s->off_leaves * 16, hipMemcpyDeviceToDevice, st));
    // The material records travel as the blob holds them, that is in the encoding p3d_set_prune_reflections last wrote
    // (p3d_scene_create.cpp: encoded_materials; refl of a T != 0 material negated while the handle prunes, a caller's
    // negative refl stored as 0): p3d_scene::host_materials and blob_prunes describe the new blob as they did the old one.
    if (mat_bytes)
        HIP_TRY(hipMemcpyAsync(new_blob.p + 4 * (size_t)N.off_mats, s->blob.p + 4 * (size_t)s->off_mats, mat_bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(new_map.p, s->prim_map.p, (size_t)n_prims * 4, hipMemcpyDeviceToDevice, st));   // the planes keep theirs
    HIP_TRY(launch_rebuild_emit(S, s->off_sphere_meta, n, W, nodes, new_blob.p, N, new_map.p, st));

    // ---- quantised nodes under a grid over the root pair's boxes, and the parents the next refit climbs
    QuantGrid G;
    {
        double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
        for (int c = 0; c < 2; c++) {
            const float* lo = root + 6 * c; const float* hi = lo + 3;
            if (!(lo[0] <= hi[0])) continue;
            for (int a = 0; a < 3; a++) { mn[a] = std::min<double>(mn[a], lo[a]); mx[a] = std::max<double>(mx[a], hi[a]); }
        }
        quantisation_grid(mn, mx, G.scale, G.base);
    }
    HIP_TRY(launch_requantise(nodes, new_qnodes.p, n_nodes, G, st));
    HIP_TRY(launch_refit_prepare(new_qnodes.p, n_nodes, nullptr, (int32_t*)new_parent.p, st));
    std::vector<uint32_t> map(n_prims);
    HIP_TRY(hipMemcpyAsync(map.data(), new_map.p, (size_t)n_prims * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    // ---- swap in: from here on nothing fails.  What the handle held moves into the locals and is freed with them.
    size_t held = s->blob.bytes() + s->qnodes.bytes() + s->prim_map.bytes() + refit_bytes(s);
    if (s->grid_ready) {                  // its items are references in the old numbering
        held += s->grid_cells.bytes() + s->grid_items.bytes();
        s->grid_cells.release(); s->grid_items.release();
        s->grid_ready = false;
    }
    s->blob = std::move(new_blob); s->qnodes = std::move(new_qnodes); s->prim_map = std::move(new_map);
    s->blob_quads = quads;
    s->off_leaves = N.off_leaves; s->off_spheres = N.off_spheres; s->off_sphere_meta = N.off_sphere_meta; s->off_tris = N.off_tris;
    s->off_tri_normals = N.off_tri_normals; s->off_boxes = N.off_boxes; s->off_mats = N.off_mats;
    memcpy(s->q_scale, G.scale, sizeof s->q_scale); memcpy(s->q_base, G.base, sizeof s->q_base);
    s->refit.nodes = std::move(new_nodes); s->refit.parent = std::move(new_parent); s->refit.arrived = std::move(new_arrived);
    if (!s->refit.status.p) s->refit.status = std::move(new_status);
    s->refit.ready = true;
    s->builder = (builder == 2u && !ploc.fell_back) ? 2 : 1;
    for (uint32_t i = 0; i < n_prims; i++) s->grid_src[i].ref = map[i];
    // max_depth sizes the walk stacks: the occupancy caches (tile_occ, wf_occ) are keyed on the stack size and the LDS
    // they were asked with, and the launch parameters are filled from the handle every frame, so nothing else holds it
    s->stats.n_nodes = bs.n_nodes; s->stats.n_leaves = bs.n_leaves; s->stats.n_leaf_refs = bs.n_leaf_refs;
    s->stats.max_depth = bs.max_depth; s->stats.sah_cost = bs.sah_cost;
    s->stats.device_bytes += s->blob.bytes() + s->qnodes.bytes() + s->prim_map.bytes() + refit_bytes(s);
    s->stats.device_bytes -= held;
    report(1u, bs.sah_cost);
    return P3D_OK;
}
