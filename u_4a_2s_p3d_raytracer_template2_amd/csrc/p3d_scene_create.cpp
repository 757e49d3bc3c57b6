// p3d_scene_create.cpp -- the life of a scene handle (include/p3d_hip.h): flattens the caller's scene into the device
// records, builds the BVH (bvh_builder.cpp) and uploads them; skybox, statistics, stream and tuning of a handle.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "bvh_builder.h"
#include "p3d_scene_state.h"
#include "scene_flatten.h"
#define P3D_POWF_TABLES_ONLY
#include "p3d_powf.h"

using namespace p3d;

namespace {
// The materials as the scene blob holds them.  shade_hit() (p3d_shade.h) spawns a reflection child where refl > 0; a
// material with T != 0 gets its refl negated while the handle prunes (p3d_set_prune_reflections), which the builds that must
// trace the child anyway -- counting, Schlick -- read as set.  So that a negative refl of such a material can only mean
// that, one the caller gave (never a reflection, like zero) is stored as zero.
std::vector<MaterialRec> encoded_materials(const std::vector<MaterialRec>& mats, bool prune) {
    std::vector<MaterialRec> out = mats;
    for (MaterialRec& m : out)
        if (m.T != 0.0f) m.refl = m.refl > 0.0f ? (prune ? -m.refl : m.refl) : 0.0f;
    return out;
}
}  // namespace

extern "C" {

int p3d_scene_create(const p3d_scene_desc* d, const p3d_build_opts* opts, int device, p3d_scene** out) {
    if (!d || !out) return fail(P3D_ERR_ARG, "desc/out is NULL");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(P3D_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(P3D_ERR_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));

    FlatScene F;
    std::string why = flatten_scene(*d, F);
    if (!why.empty()) return fail(why == "too many primitives" ? P3D_ERR_LIMIT : P3D_ERR_ARG, why);
    BvhOptions bo;
    if (opts) {
        if (opts->leaf_max) bo.leaf_max = std::min<uint32_t>(opts->leaf_max, 8);
        if (opts->sah_bins) bo.bins = opts->sah_bins;
    }
    // optional: triangles no ray of length <= sqrt(2) can hit (see p3d_build_opts::cull_never_hit).
    // Bound on the FLOAT determinant the reference computes: |det| <= |d| (|e1 x e2| + 1e-6 |e1| |e2|)
    // (products and sums of RT/scene.cpp:64-65 each round once, 6e-8 relative; 1e-6 covers them all).
    uint32_t n_culled = 0;
    if (opts && opts->cull_never_hit) {
        std::vector<BuildPrim> kept;
        kept.reserve(F.build_prims.size());
        for (const BuildPrim& b : F.build_prims) {
            bool never = false;
            if ((b.ref >> kRefKindShift) == 1u) {
                const TriRec& t = F.tris[b.ref & kRefIndexMask];
                const double e1[3] = {t.e1[0], t.e1[1], t.e1[2]}, e2[3] = {t.e2[0], t.e2[1], t.e2[2]};
                const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
                const double cross = std::sqrt(cx * cx + cy * cy + cz * cz);
                const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
                const double l2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
                never = 1.41422 * (cross + 1e-6 * l1 * l2) < 0.999e-3;
            }
            if (never) n_culled++; else kept.push_back(b);
        }
        F.build_prims.swap(kept);
    }
    std::vector<NodePair> nodes; std::vector<uint32_t> refs; BvhStats bs;
    if (opts && opts->builder > 2) return fail(P3D_ERR_ARG, "builder must be 0 (host SAH), 1 (device LBVH) or 2 (device clustering)");
    // the device builders need at least two leaves; tiny scenes are built on the host either way
    const bool device_build = opts && opts->builder >= 1 && F.build_prims.size() >= 64;
    PlocInfo ploc;
    if (device_build) {
        // built on the device into scratch buffers, read back: the leaves are typed and the primitive arrays put
        // into leaf order on the host (type_leaves) before anything is uploaded for rendering
        nodes.assign((F.build_prims.size() + 1) / 2 - 1, NodePair());
        refs.assign(F.build_prims.size(), 0u);
        NodePair* d_nodes = nullptr; uint32_t* d_refs = nullptr;
        hipError_t be = hipMalloc((void**)&d_nodes, nodes.size() * sizeof(NodePair));
        if (be == hipSuccess) be = hipMalloc((void**)&d_refs, refs.size() * sizeof(uint32_t));
        if (be == hipSuccess) be = build_bvh_device(opts->builder, F.build_prims, bo, d_nodes, d_refs, bs, &ploc, nullptr);
        if (be == hipSuccess) be = hipMemcpy(nodes.data(), d_nodes, nodes.size() * sizeof(NodePair), hipMemcpyDeviceToHost);
        if (be == hipSuccess) be = hipMemcpy(refs.data(), d_refs, refs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
        (void)hipFree(d_nodes); (void)hipFree(d_refs);
        if (be != hipSuccess) return fail(P3D_ERR_HIP, std::string("device BVH build: ") + hipGetErrorString(be));
    } else {
        build_bvh(F.build_prims, bo, nodes, refs, bs);
    }
    TypedLeaves TL;
    // Scenes small enough to be rendered from an LDS copy keep a record per leaf; the others name single-type leaves
    // in the reference itself (p3d_traverse.h: sv_leaf).  Upper bound of the blob with a record per leaf:
    const size_t blob_bound = nodes.size() * (sizeof(NodePair) + 2 * sizeof(LeafRec)) + 16 + F.spheres.size() * (sizeof(SphereRec) + sizeof(PrimMeta)) +
                              F.tris.size() * sizeof(TriRec) + F.boxes.size() * sizeof(BoxRec) + F.materials.size() * sizeof(MaterialRec) + 8 * 16 + P3D_POW_TAB_BYTES;
    const bool small_scene = blob_bound <= kLdsSceneLimit;
    type_leaves(nodes, refs, F, TL, !small_scene);
    if (TL.overflow) return fail(P3D_ERR_LIMIT, "too many mixed-type leaves");
    std::vector<SphereRec>& spheres = F.spheres; std::vector<PrimMeta>& sphere_meta = F.sphere_meta;
    std::vector<TriRec>& tris = F.tris; std::vector<BoxRec>& boxes = F.boxes;
    std::vector<PlaneRec>& planes = F.planes; std::vector<PrimMeta>& plane_meta = F.plane_meta;
    std::vector<MaterialRec>& mats = F.materials; std::vector<LightRec>& lights = F.lights;

    std::unique_ptr<p3d_scene> s(new p3d_scene());      // every early return below frees what the handle holds so far
    s->device = device;
    s->builder = !device_build ? 0 : (opts->builder == 2 && !ploc.fell_back) ? 2 : 1;
    if (const char* e = getenv("P3D_FRAME_STREAMS")) { int v = atoi(e); if (v >= 1 && v <= kLanes) s->frame_streams = v; }
    if (const char* e = getenv("P3D_RESOLVE_BLOCKS")) { int v = atoi(e); if (v >= 1 && v <= 64) s->resolve_blocks_per_shard = v; }   // tuning experiments
    if (const char* e = getenv("P3D_FUSED_RESOLVE_PX")) { int v = atoi(e); if (v >= 0 && v <= (1 << 24)) s->fused_resolve_shard_px = v; }
    s->pair_mode = getenv("P3D_NO_PAIR_MODE") == nullptr;
    s->verbose = getenv("P3D_VERBOSE") != nullptr;
    if (const char* e = getenv("P3D_TILE_LPT")) s->tile_lpt_enabled = atoi(e) != 0;
    if (const char* e = getenv("P3D_OCC")) { int v = atoi(e); if (v == 0 || v == 5 || v == 6) s->occupancy = v; }
    if (const char* e = getenv("P3D_PRIMARY_TILES")) { int v = atoi(e); if (v >= 1 && v <= kMaxPrimaryTiles) s->primary_tiles = v; }
    if (const char* e = getenv("P3D_SKY_TILES")) s->sky_tiles = atoi(e) != 0;
    if (const char* e = getenv("P3D_PRUNE_REFLECTIONS")) s->prune_reflections = atoi(e) != 0;
    {   // p3d_set_prune_reflections applies to finite scenes only: what the host can see of that, it checks here, once
        bool finite = std::isfinite(d->background[0]) && std::isfinite(d->background[1]) && std::isfinite(d->background[2]);
        auto all_finite = [&](const float* p, size_t n) { for (size_t i = 0; i < n; i++) finite = finite && std::isfinite(p[i]); };
        // (a negative shininess: powf(+0, shine) is +inf where the half vector is at right angles to the normal)
        for (const MaterialRec& m : mats) { all_finite(reinterpret_cast<const float*>(&m), sizeof(MaterialRec) / sizeof(float)); finite = finite && !(m.shine < 0.0f); }
        for (const LightRec& l : lights) { all_finite(l.pos, 3); all_finite(l.col, 3); }
        for (const TriRec& t : tris) all_finite(t.n, 3);                 // (a zero-area triangle's is NaN)
        for (const PlaneRec& p : planes) {                               // (normalised per hit: a zero normal becomes NaN there)
            const float n[3] = {p.nx, p.ny, p.nz};
            all_finite(n, 3);
            finite = finite && (p.nx != 0.0f || p.ny != 0.0f || p.nz != 0.0f);
        }
        s->finite_scene = finite;
    }
    if (const char* e = getenv("P3D_TRI_STRIDE")) s->tri_quads = atoi(e) == 64 ? 4u : 3u;
    if (const char* e = getenv("P3D_SHARE_MIN_IDLE")) { int v = atoi(e); if (v >= 0 && v <= 65) s->share_min_idle = v; }
    if (const char* e = getenv("P3D_DEBUG_SKIP")) s->dbg_skip = (uint32_t)atoi(e);      // read by -DP3D_DEBUG_SKIP builds only
    auto hip_fail = [](hipError_t e, const char* what) { return fail(P3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
    hipError_t e;
    if ((e = s->own_stream.create()) != hipSuccess) return hip_fail(e, "hipStreamCreate");
    s->stream = s->own_stream;
    if ((e = s->ev0.create()) != hipSuccess) return hip_fail(e, "hipEventCreate");
    if ((e = s->ev1.create()) != hipSuccess) return hip_fail(e, "hipEventCreate");
    for (auto& ev : s->ev_prof) if ((e = ev.create()) != hipSuccess) return hip_fail(e, "hipEventCreate");
    for (auto& ev : s->ev_pick) if ((e = ev.create()) != hipSuccess) return hip_fail(e, "hipEventCreate");
    for (auto& ev : s->ev_pick_batch) if ((e = ev.create()) != hipSuccess) return hip_fail(e, "hipEventCreate");
    if ((e = s->ev_fork.create()) != hipSuccess) return hip_fail(e, "hipEventCreate");
    for (int i = 1; i < kLanes; i++) {
        if ((e = s->lane_stream[i].create()) != hipSuccess) return hip_fail(e, "hipStreamCreate");
        if ((e = s->ev_join[i].create()) != hipSuccess) return hip_fail(e, "hipEventCreate");
    }
    {   // pack the per-lane-indexed arrays into one blob of 16-byte quads
        std::vector<uint32_t> blob;
        auto section = [&](const void* data, size_t bytes) {
            uint32_t off = (uint32_t)(blob.size() / 4);
            size_t dw = (bytes + 15) / 16 * 4;
            size_t at = blob.size();
            blob.resize(at + std::max<size_t>(dw, 4), 0u);
            if (bytes) memcpy(blob.data() + at, data, bytes);
            return off;
        };
        {   // powf's tables lead the blob: kernels that render from an LDS copy of it read them at LDS address 0 (p3d_powf.h)
            static const double log2_tab[16][2] = P3D_POW_LOG2_TAB_INIT;
            static const uint64_t exp2_tab[32] = P3D_POW_EXP2_TAB_INIT;
            static const double coefs[10] = P3D_POW_COEF_INIT;
            static_assert(sizeof log2_tab + sizeof exp2_tab + sizeof coefs == P3D_POW_TAB_BYTES, "powf table layout");
            unsigned char tab[P3D_POW_TAB_BYTES];
            memcpy(tab, log2_tab, sizeof log2_tab);
            memcpy(tab + sizeof log2_tab, exp2_tab, sizeof exp2_tab);
            memcpy(tab + sizeof log2_tab + sizeof exp2_tab, coefs, sizeof coefs);
            if (section(tab, sizeof tab) != 0u) return hip_fail(hipErrorUnknown, "scene blob layout");
        }
        s->off_leaves = section(TL.leaves.data(), TL.leaves.size() * sizeof(LeafRec));
        s->off_spheres = section(spheres.data(), spheres.size() * sizeof(SphereRec));
        s->off_sphere_meta = section(sphere_meta.data(), sphere_meta.size() * sizeof(PrimMeta));
        {   // triangles: 48-byte test records, shading normals out of line (p3d_device_types.h: TriRec)
            const uint32_t tq = s->tri_quads;
            std::vector<uint32_t> test(tris.size() * 4 * tq), nrm(tris.size() * 4);
            for (size_t i = 0; i < tris.size(); i++) {
                memcpy(test.data() + 4 * tq * i, &tris[i], 16 * tq);
                memcpy(nrm.data() + 4 * i, tris[i].n, 12);
            }
            s->off_tris = section(test.data(), test.size() * 4);
            s->off_tri_normals = section(nrm.data(), nrm.size() * 4);
        }
        s->off_boxes = section(boxes.data(), boxes.size() * sizeof(BoxRec));
        s->host_materials = mats;
        s->blob_prunes = s->prunes();
        s->off_mats = section(encoded_materials(mats, s->blob_prunes).data(), mats.size() * sizeof(MaterialRec));
        // the f32 nodes only travel with scenes small enough to be rendered from an LDS copy of the blob
        if (small_scene && blob.size() * 4 + nodes.size() * sizeof(NodePair) <= s->lds_scene_limit) {
            s->off_nodes = section(nodes.data(), nodes.size() * sizeof(NodePair));
            s->lds_capable = true;
        }
        s->blob_quads = (uint32_t)(blob.size() / 4);
        if ((e = s->blob.upload(blob)) != hipSuccess) return hip_fail(e, "upload scene blob");
    }
    {
        QuantisedNodes Q;
        quantise_nodes(nodes, Q);
        if ((e = s->qnodes.upload(Q.nodes)) != hipSuccess) return hip_fail(e, "upload nodes");
        memcpy(s->q_scale, Q.scale, sizeof s->q_scale); memcpy(s->q_base, Q.base, sizeof s->q_base);
    }
    if ((e = s->planes.upload(planes)) != hipSuccess) return hip_fail(e, "upload planes");
    if ((e = s->plane_meta.upload(plane_meta)) != hipSuccess) return hip_fail(e, "upload plane meta");
    if ((e = s->lights.upload(lights)) != hipSuccess) return hip_fail(e, "upload lights");
    s->host_lights = lights;
    grid_prims_from_desc(*d, s->grid_src);
    for (GridPrim& g : s->grid_src) {             // references in the uploaded (leaf-order) numbering
        const uint32_t kind = g.ref >> kRefKindShift, idx = g.ref & kRefIndexMask;
        if (kind == 0u) g.ref = (0u << kRefKindShift) | TL.map_sph[idx];
        else if (kind == 1u) g.ref = (1u << kRefKindShift) | TL.map_tri[idx];
        else if (kind == 2u) g.ref = (2u << kRefKindShift) | TL.map_box[idx];
    }
    {   // the same references, by scene index, are where p3d_scene_update finds a primitive's record
        std::vector<uint32_t> map(s->grid_src.size());
        for (size_t i = 0; i < map.size(); i++) map[i] = s->grid_src[i].ref;
        if ((e = s->prim_map.upload(map)) != hipSuccess) return hip_fail(e, "upload primitive map");
    }
    if ((e = s->d_counters.ensure(sizeof(DeviceCounters))) != hipSuccess) return hip_fail(e, "alloc counters");
    if ((e = hipMemset(s->d_counters.p, 0, sizeof(DeviceCounters))) != hipSuccess) return hip_fail(e, "clear counters");
    memcpy(s->bg, d->background, sizeof s->bg);
    s->n_lights = d->n_lights; s->n_materials = d->n_materials;
    s->stats.n_nodes = bs.n_nodes; s->stats.n_leaves = bs.n_leaves; s->stats.max_depth = bs.max_depth;
    s->stats.n_leaf_refs = bs.n_leaf_refs; s->stats.sah_cost = bs.sah_cost;
    s->stats.n_spheres = (uint32_t)spheres.size(); s->stats.n_triangles = (uint32_t)tris.size();
    s->stats.n_boxes = (uint32_t)boxes.size(); s->stats.n_planes = (uint32_t)planes.size();
    s->stats.n_culled = n_culled;
    s->unit_rays_only = n_culled > 0;
    s->cull_never_hit = opts && opts->cull_never_hit;
    s->stats.device_bytes = s->blob.bytes() + s->qnodes.bytes() + s->planes.bytes() + s->plane_meta.bytes() + s->lights.bytes() + s->prim_map.bytes();
    *out = s.release();
    return P3D_OK;
}

int p3d_scene_destroy(p3d_scene* s) {
    if (!s) return P3D_OK;
    (void)hipSetDevice(s->device);
    // nothing is freed while the handle's own streams may still use it
    if (s->own_stream) (void)hipStreamSynchronize(s->own_stream);
    for (int i = 1; i < kLanes; i++) if (s->lane_stream[i]) (void)hipStreamSynchronize(s->lane_stream[i]);
    delete s;
    return P3D_OK;
}

int p3d_scene_set_skybox(p3d_scene* s, const uint8_t* const faces[6], const uint32_t res_x[6], const uint32_t res_y[6],
                         const uint32_t bytes_per_pixel[6]) {
    if (!s || !faces || !res_x || !res_y || !bytes_per_pixel) return fail(P3D_ERR_ARG, "NULL argument");
    std::vector<uint8_t> all;
    uint32_t off[6];
    for (int i = 0; i < 6; i++) {
        if (!faces[i] || res_x[i] == 0 || res_y[i] == 0 || res_x[i] > 16384 || res_y[i] > 16384 || (bytes_per_pixel[i] != 3 && bytes_per_pixel[i] != 4))
            return fail(P3D_ERR_ARG, "skybox faces must be 1..16384 pixels wide and high, 3 or 4 bytes per pixel");
        const size_t bytes = (size_t)res_x[i] * res_y[i] * bytes_per_pixel[i];
        if (all.size() + bytes > 0xFFFFFFF0ull) return fail(P3D_ERR_LIMIT, "skybox too large");
        off[i] = (uint32_t)all.size();
        all.insert(all.end(), faces[i], faces[i] + bytes);
        all.resize((all.size() + 15) / 16 * 16);
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));              // (frames in flight may still read the old map)
    HIP_TRY(s->sky.upload(all));
    for (int i = 0; i < 6; i++) { s->sky_off[i] = off[i]; s->sky_w[i] = res_x[i]; s->sky_h[i] = res_y[i]; s->sky_bpp[i] = bytes_per_pixel[i]; }
    return P3D_OK;
}

int p3d_scene_get_stats(const p3d_scene* s, p3d_scene_stats* out) {
    if (!s || !out) return fail(P3D_ERR_ARG, "scene/out is NULL");
    *out = s->stats;
    return P3D_OK;
}

int p3d_set_stream(p3d_scene* s, void* hip_stream) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    s->stream = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)s->own_stream;
    return P3D_OK;
}

int p3d_set_tuning(p3d_scene* s, int32_t xcd_chunk, int32_t workspace_mib, int32_t waves_per_simd) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    if (xcd_chunk < 0 || xcd_chunk > (1 << 20)) return fail(P3D_ERR_ARG, "xcd_chunk must be >= 0");
    if (workspace_mib < 0) return fail(P3D_ERR_ARG, "workspace_mib must be >= 0");
    s->pick.invalidate(); s->pick_batch.invalidate();                  // tuning changes what the schedules cost: measure again
    if (xcd_chunk) s->xcd_chunk = xcd_chunk;
    if (workspace_mib) { s->workspace_budget = (size_t)workspace_mib << 20; s->budget_key.invalidate(); }
    if (waves_per_simd >= 0) {
        if (waves_per_simd != 0 && waves_per_simd != 5 && waves_per_simd != 6)
            return fail(P3D_ERR_ARG, "waves_per_simd must be 0 (default), 5 or 6");
        s->occupancy = waves_per_simd;
    }
    return P3D_OK;
}

int p3d_set_primary_tiles(p3d_scene* s, int32_t tiles) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    if (tiles < 0 || tiles > kMaxPrimaryTiles) return fail(P3D_ERR_ARG, "tiles must be 0 (default), 1, 2 or 3");
    s->primary_tiles = tiles ? tiles : kDefaultPrimaryTiles;
    return P3D_OK;
}

int p3d_set_sky_tiles(p3d_scene* s, int32_t on) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    if (on != 0 && on != 1) return fail(P3D_ERR_ARG, "on must be 0 or 1");
    s->sky_tiles = on != 0;
    return P3D_OK;
}

int p3d_set_prune_reflections(p3d_scene* s, int32_t on) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    if (on != 0 && on != 1) return fail(P3D_ERR_ARG, "on must be 0 or 1");
    const bool was = s->prune_reflections;
    s->prune_reflections = on != 0;
    if (s->prunes() == s->blob_prunes) return P3D_OK;
    // the kernels read the switch in the material records: rewrite them behind whatever the stream still holds
    if (stream_capturing(s->stream)) {
        s->prune_reflections = was;
        return fail(P3D_ERR_STATE, "p3d_set_prune_reflections rewrites the scene's materials: not while the stream is being captured");
    }
    hipError_t e = hipSetDevice(s->device);
    // Frames in flight still read the old records: the copy is queued behind them on the scene's stream (no other stream is
    // touched, so a capture elsewhere in the process is left alone), and the call returns when it has been made -- `enc`
    // is pageable and dies here.  A stream the handle was given before (p3d_set_stream) is the caller's to have synchronised,
    // as for every other call; the handle's own stream is waited for when it is not the one in use.
    if (e == hipSuccess && s->stream != (hipStream_t)s->own_stream) e = hipStreamSynchronize(s->own_stream);
    const std::vector<MaterialRec> enc = encoded_materials(s->host_materials, s->prunes());
    if (e == hipSuccess && !enc.empty())
        e = hipMemcpyAsync((uint32_t*)s->blob.p + 4 * (size_t)s->off_mats, enc.data(), enc.size() * sizeof(MaterialRec), hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
        s->prune_reflections = was;
        return fail(P3D_ERR_HIP, std::string("p3d_set_prune_reflections: ") + hipGetErrorString(e));
    }
    s->blob_prunes = s->prunes();
    s->pick.invalidate(); s->pick_batch.invalidate();                  // the switch changes what the schedules cost: measure again
    return P3D_OK;
}

int p3d_get_prune_reflections(const p3d_scene* s, int32_t* on) {
    if (!s || !on) return fail(P3D_ERR_ARG, "NULL argument");
    *on = s->prunes() ? 1 : 0;
    return P3D_OK;
}

}  // extern "C"
