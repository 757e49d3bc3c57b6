// p3d_host_capi.cpp -- flat C shim over the C++ host layer (p3d_scene.h) so that the Python
// test / bench harness (ctypes) can drive the same loader, camera and sample generator the
// C++ front end uses.  These p3dh_* functions are conveniences ABOVE the drop-in boundary;
// the boundary itself is include/p3d_hip.h.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../bvh_builder.h"
#include "../scene_flatten.h"
#include "../grid_builder.h"
#include "accumulate_host.h"
#include "ao_host.h"
#include "indirect_host.h"
#include "indirect_paths_host.h"
#include "denoise_host.h"
#include "p3d_scene.h"
#include "tile_coverage_host.h"
#include "upsample_host.h"

using namespace p3d_host;

struct p3dh_scene {
    Scene scene;
    Scene::Flat flat;
};

extern "C" {

p3dh_scene* p3dh_scene_load(const char* path) {
    p3dh_scene* h = new p3dh_scene();
    if (!h->scene.load_p3f(path)) { delete h; return nullptr; }
    h->scene.flatten(h->flat);
    return h;
}
void p3dh_scene_free(p3dh_scene* h) { delete h; }

// out[0..7] = n_prims, n_lights, n_materials, res_x, res_y, accel, spp, parse_ok
void p3dh_scene_info(const p3dh_scene* h, int32_t* out) {
    out[0] = (int32_t)h->flat.desc.n_prims; out[1] = (int32_t)h->flat.desc.n_lights;
    out[2] = (int32_t)h->flat.desc.n_materials;
    out[3] = h->scene.GetCamera()->GetResX(); out[4] = h->scene.GetCamera()->GetResY();
    out[5] = (int32_t)h->scene.GetAccelStruct(); out[6] = (int32_t)h->scene.GetSamplesPerPixel();
    out[7] = h->scene.parse_error().empty() ? 1 : 0;
}
void p3dh_scene_set_resolution(p3dh_scene* h, int32_t w, int32_t hh) { h->scene.GetCamera()->SetResolution(w, hh); }
void p3dh_scene_set_eye(p3dh_scene* h, float x, float y, float z) { h->scene.GetCamera()->SetEye(Vector(x, y, z)); }
// the flattened arrays stay owned by the handle
void p3dh_scene_desc(const p3dh_scene* h, p3d_scene_desc* out) { *out = h->flat.desc; }
void p3dh_scene_camera(const p3dh_scene* h, p3d_camera* out) { h->scene.GetCamera()->describe(out); }
void p3dh_primary_ray(const p3dh_scene* h, float px, float py, float* o3, float* d3) {
    Ray r = h->scene.GetCamera()->PrimaryRay(Vector(px, py, 0));
    o3[0] = r.origin.x; o3[1] = r.origin.y; o3[2] = r.origin.z;
    d3[0] = r.direction.x; d3[1] = r.direction.y; d3[2] = r.direction.z;
}
// Camera::SetEye on a COPY of the scene's camera per eye of the reference's orbit (orbit_eyes): n cameras, the scene's own
// camera unchanged.  eyes3 (optional): the n eyes.
void p3dh_orbit_eyes(float ex, float ey, float ez, int32_t n, float step_deg, float d_beta_deg, float* eyes3) {
    std::vector<Vector> e = orbit_eyes(Vector(ex, ey, ez), n, step_deg, d_beta_deg);
    for (int i = 0; i < n; i++) { eyes3[3 * i] = e[i].x; eyes3[3 * i + 1] = e[i].y; eyes3[3 * i + 2] = e[i].z; }
}
void p3dh_scene_orbit_cameras(const p3dh_scene* h, int32_t n, float step_deg, float d_beta_deg, p3d_camera* out) {
    Camera cam = *h->scene.GetCamera();
    std::vector<Vector> e = orbit_eyes(cam.GetEye(), n, step_deg, d_beta_deg);
    for (int i = 0; i < n; i++) { cam.SetEye(e[i]); cam.describe(&out[i]); }
}
void p3dh_generate_samples(uint32_t seed, int32_t res_x, int32_t res_y, int32_t spp, float aperture, float* out) {
    generate_samples(seed, res_x, res_y, spp, aperture, out);
}

// traceRays() of the host layer on n rays (origin3 / dir3: n x 3 floats); every output plane may be NULL.  Returns its status.
int p3dh_trace_rays(const p3dh_scene* h, uint32_t n, const float* origin3, const float* dir3, int32_t max_depth, int32_t accel,
                    int32_t soft_shadow, int32_t device, float* colors3, int32_t* hit_id, float* t, float* normal3) {
    std::vector<Ray> rays(n);
    for (uint32_t i = 0; i < n; i++) {
        rays[i].origin = Vector(origin3[3 * i], origin3[3 * i + 1], origin3[3 * i + 2]);
        rays[i].direction = Vector(dir3[3 * i], dir3[3 * i + 1], dir3[3 * i + 2]);
    }
    RenderOptions opt;
    opt.max_depth = max_depth; opt.accel = accel; opt.SOFT_SHADOW = soft_shadow != 0; opt.device = device;
    TraceResult res;
    const int rc = traceRays(h->scene, opt, rays, res, nullptr);
    if (rc) return rc;
    if (colors3) memcpy(colors3, res.colors.data(), (size_t)n * 12);
    if (hit_id) memcpy(hit_id, res.hit_id.data(), (size_t)n * 4);
    if (t) memcpy(t, res.t.data(), (size_t)n * 4);
    if (normal3) memcpy(normal3, res.normal.data(), (size_t)n * 12);
    return rc;
}

// occluded() of the host layer on n segments (origin3 / dir3: n x 3 floats) into out[n].  Returns its status.
int p3dh_occluded(const p3dh_scene* h, uint32_t n, const float* origin3, const float* dir3, int32_t accel, int32_t device, uint8_t* out) {
    std::vector<Ray> segments(n);
    for (uint32_t i = 0; i < n; i++) {
        segments[i].origin = Vector(origin3[3 * i], origin3[3 * i + 1], origin3[3 * i + 2]);
        segments[i].direction = Vector(dir3[3 * i], dir3[3 * i + 1], dir3[3 * i + 2]);
    }
    RenderOptions opt;
    opt.accel = accel; opt.device = device;
    std::vector<uint8_t> res;
    const int rc = occluded(h->scene, opt, segments, res, nullptr);
    if (rc) return rc;
    if (out && n) memcpy(out, res.data(), n);
    return rc;
}

// denoise() of the host layer (denoise_host.cpp): p3d_denoise's result on host planes, every bit.  out_rgb32f / out_rgb8
// may each be NULL.  The caller keeps params inside the ranges p3d_denoise accepts.
void p3dh_denoise(const p3d_denoise_params* params, const float* rgb32f, const float* depth, const float* normal, const float* albedo,
                  float* out_rgb32f, uint8_t* out_rgb8) {
    denoise(*params, rgb32f, depth, normal, albedo, out_rgb32f, out_rgb8);
}

// denoise_variance() of the host layer (denoise_host.cpp): p3d_denoise_variance's result on host planes, every bit.
// out_rgb32f / out_rgb8 / out_variance may each be NULL.  The caller keeps params inside the ranges the entry accepts.
void p3dh_denoise_variance(const p3d_denoise_params* params, const float* rgb32f, const float* depth, const float* normal,
                           const float* albedo, const float* variance, float* out_rgb32f, uint8_t* out_rgb8, float* out_variance) {
    denoise_variance(*params, rgb32f, depth, normal, albedo, variance, out_rgb32f, out_rgb8, out_variance);
}

// upsample() of the host layer (upsample_host.cpp): p3d_upsample's result on host planes, every bit.  out_plane / out_fallback
// may each be NULL.  The caller keeps params inside the ranges p3d_upsample accepts.
void p3dh_upsample(const p3d_upsample_params* params, const float* low, const float* low_depth, const float* low_normal, const float* depth,
                   const float* normal, float* out_plane, uint8_t* out_fallback) {
    upsample(*params, low, low_depth, low_normal, depth, normal, out_plane, out_fallback);
}

// ao_segments() / ao_resolve() of the host layer (ao_host.cpp): steps 1 to 6 and step 8 of p3d_ambient_occlusion's definition
// on host planes, every bit.  One frame, the frame-th of a batch: origin_out / dir_out [res_y][res_x][samples][3], valid_out
// [res_y][res_x].  The caller keeps params inside the ranges p3d_ambient_occlusion accepts.
void p3dh_ao_segments(const p3d_ao_params* params, const p3d_camera* cam, int32_t frame, int32_t res_x, int32_t res_y, const float* depth,
                      const float* normal, float* origin_out, float* dir_out, uint8_t* valid_out) {
    ao_segments(*params, *cam, frame, res_x, res_y, depth, normal, origin_out, dir_out, valid_out);
}
void p3dh_ao_resolve(int32_t samples, uint64_t n_pixels, const int32_t* occluded, const float* rgb32f_in, float* ao_out, float* rgb32f_out) {
    ao_resolve(samples, (size_t)n_pixels, occluded, rgb32f_in, ao_out, rgb32f_out);
}

// indirect_resolve() of the host layer (indirect_host.cpp): steps 8 and 9 of p3d_indirect_diffuse's definition on host planes,
// every bit.  radiance [n_pixels][samples][3], valid [n_pixels]; albedo, rgb32f_in, indirect_out and rgb32f_out may each be
// NULL.  The rays are p3dh_ao_segments' at radius 1.  The caller keeps samples inside what p3d_indirect_diffuse accepts.
void p3dh_indirect_resolve(int32_t samples, uint64_t n_pixels, const float* radiance, const uint8_t* valid, const float* albedo,
                           const float* rgb32f_in, float* indirect_out, float* rgb32f_out) {
    indirect_resolve(samples, (size_t)n_pixels, radiance, valid, albedo, rgb32f_in, indirect_out, rgb32f_out);
}

// path_next() / path_add() of the host layer (indirect_paths_host.cpp): steps 4 and 3 of p3d_indirect_paths' definition for m
// paths that just traced ray b, every bit.  The arrays are indirect_paths_host.h's; vertex 0 is p3dh_ao_segments' at radius 1
// and step 5 is p3dh_indirect_resolve.  The caller keeps b in 0 .. 6 and hit_id inside the scene.
void p3dh_path_next(uint64_t m, int32_t b, float bias, const float* origin, const float* dir, const float* t, const float* normal,
                    const int32_t* hit_id, const uint32_t* prim_material, const float* materials, const uint32_t* pk0, const uint32_t* sample,
                    float* throughput, float* origin_out, float* dir_out, uint8_t* alive_out) {
    path_next((size_t)m, b, bias, origin, dir, t, normal, hit_id, prim_material, materials, pk0, sample, throughput, origin_out, dir_out, alive_out);
}
void p3dh_path_add(uint64_t m, int32_t b, const float* throughput, const float* radiance, const uint8_t* alive, float* sum) {
    path_add((size_t)m, b, throughput, radiance, alive, sum);
}

// accumulate() of the host layer (accumulate_host.cpp): p3d_accumulate's result on host planes, every bit.  history may be
// NULL; out_rgb32f / out_length may each be NULL.  The caller keeps params inside the ranges p3d_accumulate accepts.
void p3dh_accumulate(const p3d_accumulate_params* params, const p3d_accumulate_frames* frames, const p3d_accumulate_history* history,
                     float* out_rgb32f, float* out_length) {
    accumulate(*params, *frames, history, out_rgb32f, out_length);
}

// accumulate_moving() of the host layer: p3d_accumulate_moving's result on host planes and host geometry, every bit.  history
// may be NULL; the three outputs may each be NULL.  The caller keeps the arguments inside what p3d_accumulate_moving accepts.
void p3dh_accumulate_moving(const p3d_accumulate_params* params, const p3d_accumulate_frames* frames, const p3d_accumulate_history* history,
                            const p3d_accumulate_motion* motion, float* out_rgb32f, float* out_length, float* out_prev_xy) {
    accumulate_moving(*params, *frames, history, *motion, out_rgb32f, out_length, out_prev_xy);
}

// accumulate_variance() of the host layer: p3d_accumulate_variance's result on host planes and host geometry, every bit.
// history (with history_moments) and motion may be NULL; the five outputs may each be NULL; out_rgb32f must not be the
// frames' colour.  The caller keeps the arguments inside what p3d_accumulate_variance accepts.
void p3dh_accumulate_variance(const p3d_accumulate_params* params, const p3d_accumulate_variance_params* variance_params,
                              const p3d_accumulate_frames* frames, const p3d_accumulate_history* history, const float* history_moments,
                              const p3d_accumulate_motion* motion, float* out_rgb32f, float* out_length, float* out_moments,
                              float* out_variance, float* out_prev_xy) {
    accumulate_variance(*params, *variance_params, *frames, history, history_moments, motion, out_rgb32f, out_length, out_moments,
                        out_variance, out_prev_xy);
}

// tile_coverage() of the host layer (tile_coverage_host.cpp): the level-1 launch's tile coverage mask for cam's frame over a
// scene description, the statements of csrc/p3d_tile_coverage.h.  active_out [tiles_y][tiles_x] bytes; returns 1 when every
// tile was marked because a primitive asked for it.
int32_t p3dh_tile_coverage(const p3d_camera* cam, int32_t tile_h, int32_t row_block, int32_t rank, int32_t world, const p3d_scene_desc* desc,
                           uint8_t* active_out) {
    return tile_coverage(*cam, tile_h, row_block, rank, world, desc->n_prims, desc->prim_type, desc->prim_data, active_out);
}

// ---- host-only BVH build, for tests that run without a GPU
struct p3dh_bvh {
    std::vector<p3d::NodePair> nodes;
    std::vector<uint32_t> refs;
    std::vector<p3d::BuildPrim> prims;   // padded bounds, in the builder's final order
    p3d::BvhStats stats;
};
// saveImgFile() replacement, exposed for the CPU-side tests
int p3dh_save_png(const char* path, const uint8_t* img_Data, int32_t w, int32_t h) { return save_png(path, img_Data, w, h); }

p3dh_bvh* p3dh_bvh_build(const p3d_scene_desc* d, uint32_t leaf_max) {
    p3d::FlatScene F;
    if (!p3d::flatten_scene(*d, F).empty()) return nullptr;
    p3dh_bvh* b = new p3dh_bvh();
    b->prims = F.build_prims;
    p3d::BvhOptions o;
    if (leaf_max) o.leaf_max = leaf_max;
    p3d::build_bvh(b->prims, o, b->nodes, b->refs, b->stats);
    return b;
}
void p3dh_bvh_free(p3dh_bvh* b) { delete b; }
// out[0..4] = n_nodes, n_leaf_refs, n_leaves, max_depth, n_prims
void p3dh_bvh_info(const p3dh_bvh* b, uint32_t* out) {
    out[0] = (uint32_t)b->nodes.size(); out[1] = (uint32_t)b->refs.size(); out[2] = b->stats.n_leaves;
    out[3] = b->stats.max_depth; out[4] = (uint32_t)b->prims.size();
}
// nodes16: 16 dwords per node exactly as uploaded; refs: leaf reference list
void p3dh_bvh_dump(const p3dh_bvh* b, uint32_t* nodes16, uint32_t* refs) {
    memcpy(nodes16, b->nodes.data(), b->nodes.size() * sizeof(p3d::NodePair));
    memcpy(refs, b->refs.data(), b->refs.size() * sizeof(uint32_t));
}

// the 32-byte node pairs kernels that read the scene from HBM walk (csrc/scene_flatten.cpp: quantise_nodes):
// qnodes8 = 8 dwords per node, scale3 / base3 = the de-quantisation constants (plane = base + code * scale)
void p3dh_bvh_quantise(const p3dh_bvh* b, uint32_t* qnodes8, float* scale3, float* base3) {
    p3d::QuantisedNodes Q;
    p3d::quantise_nodes(b->nodes, Q);
    memcpy(qnodes8, Q.nodes.data(), Q.nodes.size() * sizeof(p3d::QNode));
    memcpy(scale3, Q.scale, sizeof Q.scale); memcpy(base3, Q.base, sizeof Q.base);
}

// ---- the build primitives flatten_scene hands either BVH builder for a scene (padded bounds and leaf references, scene
// order of the bounded primitives); returns their number, or -1.  Arrays may be NULL to ask for the number only.
int64_t p3dh_build_prims(const p3d_scene_desc* d, float* lo3, float* hi3, uint32_t* ref, uint64_t cap) {
    p3d::FlatScene F;
    if (!p3d::flatten_scene(*d, F).empty()) return -1;
    for (size_t i = 0; lo3 && hi3 && ref && i < F.build_prims.size() && i < cap; i++) {
        memcpy(lo3 + 3 * i, F.build_prims[i].lo, 12); memcpy(hi3 + 3 * i, F.build_prims[i].hi, 12);
        ref[i] = F.build_prims[i].ref;
    }
    return (int64_t)F.build_prims.size();
}

// ---- the triangle normals the device shades with (computed on the host by flatten_scene), scene order of the
// triangles; returns their number.  For the CPU-side parity test against the reference's known answers.
int64_t p3dh_triangle_normals(const p3d_scene_desc* d, float* out3, uint64_t cap) {
    p3d::FlatScene F;
    if (!p3d::flatten_scene(*d, F).empty()) return -1;
    for (size_t i = 0; i < F.tris.size() && i < cap; i++) memcpy(out3 + 3 * i, F.tris[i].n, 12);
    return (int64_t)F.tris.size();
}

// ---- host-only grid build (the reference's Grid::Build layout, csrc/grid_builder.cpp), for tests without a GPU
// dims[3]; counts: cells' populations (nx*ny*nz) or NULL; returns the number of cells, or -1
int64_t p3dh_grid_build(const p3d_scene_desc* d, int32_t* dims, uint32_t* counts, uint64_t counts_cap) {
    std::vector<p3d::GridPrim> prims;
    p3d::grid_prims_from_desc(*d, prims);
    p3d::GridHost g;
    if (!p3d::build_grid(prims, g)) return -1;
    dims[0] = g.n[0]; dims[1] = g.n[1]; dims[2] = g.n[2];
    const size_t cells = g.cell_start.size() - 1;
    if (counts) for (size_t c = 0; c < cells && c < counts_cap; c++) counts[c] = g.cell_start[c + 1] - g.cell_start[c];
    return (int64_t)cells;
}


// ---- the whole of build_grid()'s output, for the device build to be compared with: over a scene description (d != NULL), or
// over n boxes lo3 / hi3 [n*3] with the references ref[n] they are listed under, as p3d_debug_grid_build takes them.
// dims3, mn3, mx3, *n_items; cell_start / items (may be NULL): the first cell_cap / item_cap words.  Returns the number of
// cells, or -1 when the formula asks for more than 2^31 of them.
int64_t p3dh_grid_dump(const p3d_scene_desc* d, uint32_t n, const float* lo3, const float* hi3, const uint32_t* ref, int32_t* dims3,
                       float* mn3, float* mx3, uint64_t* n_items, uint32_t* cell_start, uint64_t cell_cap, uint32_t* items,
                       uint64_t item_cap) {
    std::vector<p3d::GridPrim> prims;
    if (d) p3d::grid_prims_from_desc(*d, prims);
    else {
        prims.resize(n);
        for (size_t i = 0; i < n; i++) { memcpy(prims[i].lo, lo3 + 3 * i, 12); memcpy(prims[i].hi, hi3 + 3 * i, 12); prims[i].ref = ref[i]; }
    }
    p3d::GridHost g;
    if (!p3d::build_grid(prims, g)) return -1;
    for (int a = 0; a < 3; a++) { dims3[a] = g.n[a]; mn3[a] = g.mn[a]; mx3[a] = g.mx[a]; }
    *n_items = g.items.size();
    if (cell_start) memcpy(cell_start, g.cell_start.data(), std::min<size_t>(cell_cap, g.cell_start.size()) * 4);
    if (items) memcpy(items, g.items.data(), std::min<size_t>(item_cap, g.items.size()) * 4);
    return (int64_t)g.cell_start.size() - 1;
}

}  // extern "C"
