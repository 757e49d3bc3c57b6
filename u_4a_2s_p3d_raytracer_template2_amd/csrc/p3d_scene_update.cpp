// p3d_scene_update.cpp -- p3d_scene_update of include/p3d_hip.h: primitives and lights of a scene handle move, the BVH
// keeps its topology and is refitted on the device (scene_update.hip).  Everything is enqueued on the scene's stream; the
// call waits once, for the root's boxes, which set the quantisation grid the launch parameters carry by value.
#include <cmath>
#include <cstring>

#include "grid_device.h"
#include "p3d_scene_state.h"
#include "scene_flatten.h"
#include "scene_update.h"

using namespace p3d;

namespace {

// what the refit needs next to the scene: allocated, and the parents derived, by the first update of a handle
int prepare_refit(p3d_scene* s, uint32_t n_nodes) {
    if (s->refit.ready) return P3D_OK;
    p3d_scene::Refit& R = s->refit;
    size_t bytes = 0;
    if (!s->lds_capable) { HIP_TRY(R.nodes.ensure((size_t)n_nodes * sizeof(NodePair))); bytes += R.nodes.cap; }
    HIP_TRY(R.parent.ensure((size_t)n_nodes * sizeof(int32_t)));
    HIP_TRY(R.arrived.ensure((size_t)n_nodes * sizeof(uint32_t)));
    HIP_TRY(R.status.ensure(kStatusWords * sizeof(uint32_t)));
    bytes += R.parent.cap + R.arrived.cap + R.status.cap;
    HIP_TRY(launch_refit_prepare(s->qnodes.p, n_nodes, (NodePair*)R.nodes.p, (int32_t*)R.parent.p, s->stream));
    s->stats.device_bytes += bytes;
    R.ready = true;
    return P3D_OK;
}

int ensure_staging(p3d_scene* s, RawBuf& b, size_t bytes) {
    const size_t before = b.cap;
    HIP_TRY(b.ensure(bytes));
    s->stats.device_bytes += b.cap - before;
    return P3D_OK;
}

}  // namespace

extern "C" int p3d_scene_update(p3d_scene* s, const p3d_prim_update* u) {
    if (!s || !u) return fail(P3D_ERR_ARG, "scene/update is NULL");
    if (u->n > 0 && !u->prim_data) return fail(P3D_ERR_ARG, "prim_data is NULL with n > 0");
    if (u->memory != 0 && u->memory != 1) return fail(P3D_ERR_ARG, "p3d_prim_update::memory must be 0 (host) or 1 (device)");
    if (s->cull_never_hit)
        return fail(P3D_ERR_STATE, "scene was built with cull_never_hit: a moved triangle may no longer be one no ray can hit; create a new handle");
    const uint32_t n_prims = (uint32_t)s->prim_map.n;
    const bool host = u->memory == 0;
    if (host) {
        if (!u->index && u->n > n_prims) return fail(P3D_ERR_ARG, "more primitives than the scene has");
        for (uint32_t i = 0; u->index && i < u->n; i++)
            if (u->index[i] >= n_prims) return fail(P3D_ERR_ARG, "primitive index out of range");
    }
    HIP_TRY(hipSetDevice(s->device));
    if (stream_capturing(s->stream))
        return fail(P3D_ERR_STATE, "p3d_scene_update waits on the device and changes launch parameters: not while the stream is being captured");
    const uint32_t n_nodes = (uint32_t)s->qnodes.n;
    uint32_t bad_indices = 0;
    if (u->n > 0) {
        int rc = prepare_refit(s, n_nodes);
        if (rc) return rc;
        // from the first update the host cannot follow on, the device keeps GRID mode's boxes (p3d_scene_build_grid)
        if (!host && (rc = ensure_grid_bounds(s))) return rc;
        const float* d_prims = u->prim_data; const uint32_t* d_index = u->index;
        if (host) {      // one code path: host data is staged and takes the kernel device data takes
            if ((rc = ensure_staging(s, s->refit.stage_prims, (size_t)u->n * 12 * sizeof(float)))) return rc;
            HIP_TRY(hipMemcpyAsync(s->refit.stage_prims.p, u->prim_data, (size_t)u->n * 12 * sizeof(float), hipMemcpyHostToDevice, s->stream));
            d_prims = (const float*)s->refit.stage_prims.p;
            if (u->index) {
                if ((rc = ensure_staging(s, s->refit.stage_index, (size_t)u->n * sizeof(uint32_t)))) return rc;
                HIP_TRY(hipMemcpyAsync(s->refit.stage_index.p, u->index, (size_t)u->n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
                d_index = (const uint32_t*)s->refit.stage_index.p;
            }
        }
        SceneRecords S;
        S.blob = s->blob.p; S.off_leaves = s->off_leaves; S.off_spheres = s->off_spheres; S.off_tris = s->off_tris;
        S.off_tri_normals = s->off_tri_normals; S.off_boxes = s->off_boxes; S.tri_quads = s->tri_quads;
        S.planes = s->planes.p; S.prim_map = s->prim_map.p; S.n_prims = n_prims;
        uint32_t* status = (uint32_t*)s->refit.status.p;
        HIP_TRY(hipMemsetAsync(status, 0, kStatusWords * sizeof(uint32_t), s->stream));
        HIP_TRY(launch_update_records(S, u->n, d_index, d_prims, status, s->grid_bounds.p, s->stream));
        // LDS-capable scenes carry their f32 nodes in the blob: the LDS walk reads them there
        NodePair* nodes = s->lds_capable ? (NodePair*)(s->blob.p + 4 * (size_t)s->off_nodes) : (NodePair*)s->refit.nodes.p;
        HIP_TRY(launch_refit(S, nodes, (const int32_t*)s->refit.parent.p, (uint32_t*)s->refit.arrived.p, n_nodes, status, s->stream));
        uint32_t back[kStatusWords];
        HIP_TRY(hipMemcpyAsync(back, status, sizeof back, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        bad_indices = back[kStatusBadIndex];
        {   // moved geometry may leave the old code grid, and clamped codes would not be conservative: a new grid over
            // the root pair's boxes (= the bounds of all boxes), then every node coded again
            float f[kStatusRootFloats];
            memcpy(f, back, sizeof f);
            double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
            for (int c = 0; c < 2; c++) {
                const float* lo = f + 6 * c; const float* hi = lo + 3;
                if (!(lo[0] <= hi[0])) continue;                   // absent child (NaN bounds)
                for (int a = 0; a < 3; a++) { mn[a] = std::min<double>(mn[a], lo[a]); mx[a] = std::max<double>(mx[a], hi[a]); }
            }
            QuantGrid G;
            quantisation_grid(mn, mx, G.scale, G.base);
            HIP_TRY(launch_requantise(nodes, s->qnodes.p, n_nodes, G, s->stream));
            memcpy(s->q_scale, G.scale, sizeof s->q_scale); memcpy(s->q_base, G.base, sizeof s->q_base);
        }
        // GRID mode: the grid's shape is observable, so it is built again, from the reference's boxes of the new points
        if (s->grid_stale.empty() && !host) s->grid_stale.assign(n_prims, 0);
        if (host) {
            for (uint32_t i = 0; i < u->n; i++) {
                const uint32_t prim = u->index ? u->index[i] : i;
                GridPrim& g = s->grid_src[prim];
                grid_prim_bounds(g.ref >> kRefKindShift, u->prim_data + 12 * (size_t)i, g);
                if (!s->grid_stale.empty() && s->grid_stale[prim]) { s->grid_stale[prim] = 0; s->grid_stale_count--; }
            }
        } else {         // the points stay on the device: remember whose boxes the host no longer knows
            std::vector<uint32_t> idx;
            if (u->index) {
                idx.resize(u->n);
                HIP_TRY(hipMemcpy(idx.data(), u->index, (size_t)u->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            }
            for (uint32_t i = 0; i < u->n; i++) {
                const uint32_t prim = u->index ? idx[i] : i;
                if (prim < n_prims && !s->grid_stale[prim]) { s->grid_stale[prim] = 1; s->grid_stale_count++; }
            }
        }
        if (s->grid_ready) {
            s->stats.device_bytes -= s->grid_cells.bytes() + s->grid_items.bytes();
            s->grid_cells.release(); s->grid_items.release();
            s->grid_ready = false;
        }
    }
    if (u->lights && s->n_lights) {
        for (uint32_t i = 0; i < s->n_lights; i++) {
            const float* l = u->lights + 6 * (size_t)i;
            s->host_lights[i] = LightRec{{l[0], l[1], l[2]}, 0.0f, {l[3], l[4], l[5]}, 0.0f};
        }
        HIP_TRY(hipMemcpyAsync(s->lights.p, s->host_lights.data(), s->n_lights * sizeof(LightRec), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));       // (frames in flight may still read the old sub-lights)
        s->soft_lights.release();                       // the 4x4 grid is built again on next use
    }
    if (bad_indices) return fail(P3D_ERR_ARG, "primitive indices out of range were skipped; the scene and its tree are consistent");
    return P3D_OK;
}
