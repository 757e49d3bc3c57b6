// p3d_capi_misc.cpp -- the small entries of include/p3d_hip.h: errors, device queries, synchronisation, counters,
// profile and timers, de-interleaving, device memory for callers, and the debug entries that run one device function
// (those of the image-space entries: p3d_debug_planes.cpp).
#include <cstring>

#include "grid_device.h"
#include "p3d_debug_run.h"

using namespace p3d;

namespace {
thread_local std::string g_err;
}

extern "C" int p3d_internal_set_error(int code, const char* msg) { g_err = msg ? msg : ""; return code; }
// device and stream a scene is bound to (for p3d_comm.cpp)
extern "C" int p3d_internal_scene_binding(p3d_scene* s, int* device, void** stream) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    *device = s->device; *stream = (void*)s->stream;
    return P3D_OK;
}

extern "C" {

int p3d_abi_version(void) { return P3D_ABI_VERSION; }
const char* p3d_last_error(void) { return g_err.c_str(); }

int p3d_device_count(int* count) {
    if (!count) return fail(P3D_ERR_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(P3D_ERR_NO_DEVICE, hipGetErrorString(e)); }
    *count = n;
    return P3D_OK;
}

int p3d_local_rows(int32_t res_y, int32_t row_block, int32_t world) {
    if (row_block <= 0) row_block = 16;
    if (world <= 0) world = 1;
    int nblocks = (res_y + row_block - 1) / row_block;
    return ((nblocks + world - 1) / world) * row_block;
}

int p3d_sync(p3d_scene* s) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return P3D_OK;
}

int p3d_get_counters(p3d_scene* s, p3d_counters* out) {
    if (!s || !out) return fail(P3D_ERR_ARG, "scene/out is NULL");
    if (!s->counters_valid) return fail(P3D_ERR_STATE, "no render with P3D_FLAG_COUNTERS yet");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    DeviceCounters c;
    HIP_TRY(hipMemcpy(&c, s->d_counters.p, sizeof c, hipMemcpyDeviceToHost));
    out->closest_queries = c.closest_queries; out->shadow_queries = c.shadow_queries;
    out->box_tests = c.box_tests; out->sphere_tests = c.sphere_tests; out->tri_tests = c.tri_tests;
    out->aabox_tests = c.aabox_tests; out->plane_tests = c.plane_tests; out->pixels = c.pixels;
    return P3D_OK;
}

int p3d_debug_set_stamps(p3d_scene* s, void* device_buffer) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    if (device_buffer && !kernels_have_stamps())
        return fail(P3D_ERR_STATE, "this build has no stamp hooks: use the diagnostic build (make -C csrc stamps, libp3d_hip_stamps.so)");
    s->dbg_stamps = (unsigned long long*)device_buffer;
    return P3D_OK;
}

int p3d_debug_set_stamp_level(p3d_scene* s, int32_t level) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    if (level < 1 || level > kMaxDepth) return fail(P3D_ERR_ARG, "level must be in 1..16");
    s->dbg_stamp_level = level;
    return P3D_OK;
}

int p3d_get_profile(p3d_scene* s, float* frame_ms, float* kernel_ms) {
    if (!s || !frame_ms || !kernel_ms) return fail(P3D_ERR_ARG, "NULL argument");
    if (!s->profile_valid) return fail(P3D_ERR_STATE, "no render with P3D_FLAG_PROFILE yet");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipEventSynchronize(s->ev_prof[1]));
    HIP_TRY(hipEventElapsedTime(frame_ms, s->ev_prof[0], s->ev_prof[1]));
    HIP_TRY(hipEventElapsedTime(kernel_ms, s->ev_prof[2], s->ev_prof[3]));
    return P3D_OK;
}

int p3d_scene_last_builder(const p3d_scene* s, int32_t* builder) {
    if (!s || !builder) return fail(P3D_ERR_ARG, "NULL argument");
    *builder = s->builder;
    return P3D_OK;
}

int p3d_last_schedule(p3d_scene* s, int32_t* schedule) {
    if (!s || !schedule) return fail(P3D_ERR_ARG, "NULL argument");
    if (s->last_schedule < 0) return fail(P3D_ERR_STATE, "no render yet");
    *schedule = s->last_schedule;
    return P3D_OK;
}

int p3d_last_primary_tiles(p3d_scene* s, int32_t* tiles) {
    if (!s || !tiles) return fail(P3D_ERR_ARG, "NULL argument");
    if (s->last_schedule < 0) return fail(P3D_ERR_STATE, "no render yet");
    *tiles = s->last_primary_tiles;
    return P3D_OK;
}

// What the pre-pass of the most recent frame marked is on the device: it is read back here, after the stream has passed, and
// nowhere on a frame's own path.
int p3d_last_sky_tiles(p3d_scene* s, int32_t* used, int32_t* empty_tiles) {
    if (!s || !used || !empty_tiles) return fail(P3D_ERR_ARG, "NULL argument");
    if (s->last_schedule < 0) return fail(P3D_ERR_STATE, "no render yet");
    *used = 0; *empty_tiles = 0;
    if (!s->last_sky.on) return P3D_OK;
    if (stream_capturing(s->stream)) return fail(P3D_ERR_STATE, "p3d_last_sky_tiles waits for the stream: not while it is being captured");
    HIP_TRY(hipSetDevice(s->device));
    const CoverTiles& g = s->last_sky.tiles;
    std::vector<uint32_t> status((size_t)g.tiles_y);
    const uint32_t* d_status = (const uint32_t*)s->sky_mask.p + (size_t)g.tiles_y * s->last_sky.row_words;
    HIP_TRY(hipMemcpyAsync(status.data(), d_status, status.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    int64_t tiles = 0, active = 0;
    for (int32_t ty = 0; ty < g.tiles_y; ty++) {
        if (status[(size_t)ty] & kCoverAllFlag) return P3D_OK;            // a primitive asked for every tile: the frame ran as without a mask
        if (cover_tile_image_row(g, ty) >= g.res_y) continue;               // rows the compact buffer pads the image with
        tiles += g.tiles_x; active += status[(size_t)ty];
    }
    *used = 1; *empty_tiles = (int32_t)(tiles - active);
    return P3D_OK;
}

// The shard counters the level launches of a wavefront pass keep stay on the device until the next pass's level-1 launch
// clears them (LaunchParams::wf_alt): they are read back here, after the stream has passed, and nowhere on a frame's own path.
int p3d_last_level_rays(p3d_scene* s, uint32_t* counts, int32_t n) {
    if (!s || !counts) return fail(P3D_ERR_ARG, "NULL argument");
    if (n < 1 || n > kMaxDepth) return fail(P3D_ERR_ARG, "n must be in 1..16");
    if (!s->last_wf.valid) return fail(P3D_ERR_STATE, "the handle's most recent frame did not run the wavefront schedule (or there is none yet)");
    if (s->last_wf.passes > (size_t)s->last_wf.lanes)
        return fail(P3D_ERR_STATE, "the frame ran several passes over the same counters (sample passes or bands): only its last pass is on the device");
    if (stream_capturing(s->stream)) return fail(P3D_ERR_STATE, "p3d_last_level_rays waits for the stream: not while it is being captured");
    HIP_TRY(hipSetDevice(s->device));
    for (int32_t i = 0; i < n; i++) counts[i] = 0u;
    std::vector<uint32_t> w(kCountBufferWords);
    for (size_t ln = 0; ln < s->last_wf.passes; ln++) {          // (the joined lanes' launches are in front of the stream's tail)
        HIP_TRY(hipMemcpyAsync(w.data(), s->ws[ln].counts.p, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        const uint32_t par = w[kCountWords + 4 * kShards + 32] & 1u;     // the set this pass's launches used (wf_ctrl[32])
        for (int l = 2; l <= s->last_wf.D && l <= n; l++) {
            const uint32_t* q = l == 2 ? w.data() + kCountWords + (size_t)(par * 2u) * kShards : w.data() + (size_t)l * kShards;
            for (int sh = 0; sh < kShards; sh++) counts[l - 1] += q[sh];
        }
    }
    counts[0] = (uint32_t)std::min<uint64_t>(s->last_wf.level1, 0xFFFFFFFFull);
    return P3D_OK;
}

int p3d_timer_begin(p3d_scene* s) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipEventRecord(s->ev0, s->stream));
    s->timer_open = true;
    return P3D_OK;
}

int p3d_timer_end(p3d_scene* s, float* ms) {
    if (!s || !ms) return fail(P3D_ERR_ARG, "scene/ms is NULL");
    if (!s->timer_open) return fail(P3D_ERR_STATE, "p3d_timer_begin was not called");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipEventRecord(s->ev1, s->stream));
    HIP_TRY(hipEventSynchronize(s->ev1));
    HIP_TRY(hipEventElapsedTime(ms, s->ev0, s->ev1));
    s->timer_open = false;
    return P3D_OK;
}

int p3d_deinterleave_frames(p3d_scene* s, const void* gathered, void* frames, int32_t res_x, int32_t res_y,
                            int32_t row_block, int32_t world, int32_t bpp, uint64_t rank_stride_bytes,
                            int32_t n_frames, uint64_t tile_stride_bytes, uint64_t frame_stride_bytes) {
    if (!s || !gathered || !frames) return fail(P3D_ERR_ARG, "NULL argument");
    if (res_x <= 0 || res_y <= 0 || world <= 0 || n_frames <= 0) return fail(P3D_ERR_ARG, "bad sizes");
    if (row_block <= 0) row_block = 16;
    if (bpp != 3 && bpp != 4 && bpp != 12) return fail(P3D_ERR_ARG, "bytes_per_pixel must be 3, 4 or 12");
    HIP_TRY(hipSetDevice(s->device));
    const size_t tile = (size_t)p3d_local_rows(res_y, row_block, world) * res_x * bpp;
    const size_t in_stride = tile_stride_bytes ? (size_t)tile_stride_bytes : tile;
    const size_t stride = rank_stride_bytes ? (size_t)rank_stride_bytes : in_stride * n_frames;
    const size_t out_stride = frame_stride_bytes ? (size_t)frame_stride_bytes : (size_t)res_y * res_x * bpp;
    HIP_TRY(launch_deinterleave(gathered, frames, res_x, res_y, row_block, world, stride, bpp, n_frames, in_stride,
                                out_stride, s->stream));
    return P3D_OK;
}

int p3d_deinterleave(p3d_scene* s, const void* gathered, void* frame, int32_t res_x, int32_t res_y,
                     int32_t row_block, int32_t world, int32_t bpp, uint64_t rank_stride_bytes) {
    return p3d_deinterleave_frames(s, gathered, frame, res_x, res_y, row_block, world, bpp, rank_stride_bytes, 1, 0, 0);
}

int p3d_device_alloc(p3d_scene* s, uint64_t bytes, void** out) {
    if (!s || !out) return fail(P3D_ERR_ARG, "scene/out is NULL");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMalloc(out, bytes ? (size_t)bytes : 1));
    return P3D_OK;
}
int p3d_device_free(p3d_scene* s, void* ptr) {
    if (!s) return fail(P3D_ERR_ARG, "scene is NULL");
    HIP_TRY(hipSetDevice(s->device));
    if (ptr) HIP_TRY(hipFree(ptr));
    return P3D_OK;
}
int p3d_upload(p3d_scene* s, void* device_dst, const void* host_src, uint64_t bytes) {
    if (!s || !device_dst || !host_src) return fail(P3D_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpyAsync(device_dst, host_src, (size_t)bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return P3D_OK;
}
int p3d_download(p3d_scene* s, void* host_dst, const void* device_src, uint64_t bytes) {
    if (!s || !host_dst || !device_src) return fail(P3D_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpyAsync(host_dst, device_src, (size_t)bytes, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return P3D_OK;
}

}  // extern "C"

namespace {

typedef hipError_t (*RcpCheckLaunch)(uint32_t, uint64_t, unsigned long long*, uint32_t*, hipStream_t);
int debug_check_reciprocal(const char* entry, RcpCheckLaunch launch, int device, uint32_t first_bits, uint64_t count,
                           uint64_t* n_bad, uint32_t* first_bad) {
    if (!n_bad || !first_bad) return fail(P3D_ERR_ARG, "NULL argument");
    *n_bad = 0; *first_bad = 0xFFFFFFFFu;
    if (count == 0) return P3D_OK;
    if (count > (1ull << 32)) return fail(P3D_ERR_ARG, "count exceeds the 2^32 bit patterns");
    unsigned long long r[2] = {0ull, 0xFFFFFFFFull};      // [0] mismatches, [1] (low word) first mismatching pattern
    DebugArg a[1] = {{r, r, sizeof r}};
    int rc = debug_run(entry, device, a, [&] {
        return launch(first_bits, count, a[0].as<unsigned long long>(), (uint32_t*)(a[0].as<unsigned long long>() + 1), nullptr);
    });
    if (rc) return rc;
    *n_bad = r[0]; *first_bad = (uint32_t)r[1];
    return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_debug_intersect(int device, uint32_t n, const uint32_t* type, const float* prim12, const float* origin,
                        const float* dir, int32_t* hit, float* t, float* normal) {
    if (!type || !prim12 || !origin || !dir || !hit || !t || !normal) return fail(P3D_ERR_ARG, "NULL argument");
    if (n == 0) return P3D_OK;
    const size_t N = n;
    DebugArg a[7] = {{type, nullptr, N * 4}, {prim12, nullptr, N * 48}, {origin, nullptr, N * 12}, {dir, nullptr, N * 12},
                     {nullptr, hit, N * 4}, {nullptr, t, N * 4}, {nullptr, normal, N * 12}};
    return debug_run("p3d_debug_intersect", device, a, [&] {
        return launch_debug_intersect(n, a[0].as<uint32_t>(), a[1].as<float>(), a[2].as<float>(), a[3].as<float>(), a[4].as<int32_t>(),
                                      a[5].as<float>(), a[6].as<float>(), nullptr);
    });
}

int p3d_debug_check_rcp(int device, uint32_t first_bits, uint64_t count, uint64_t* n_bad, uint32_t* first_bad) {
    return debug_check_reciprocal("p3d_debug_check_rcp", launch_debug_check_rcp, device, first_bits, count, n_bad, first_bad);
}
int p3d_debug_check_rcp_len(int device, uint32_t first_bits, uint64_t count, uint64_t* n_bad, uint32_t* first_bad) {
    return debug_check_reciprocal("p3d_debug_check_rcp_len", launch_debug_check_rcp_len, device, first_bits, count, n_bad, first_bad);
}

int p3d_debug_powf(int device, uint32_t n, const float* x, const float* y, float* out) {
    if (!x || !y || !out) return fail(P3D_ERR_ARG, "NULL argument");
    if (n == 0) return P3D_OK;
    const size_t N = n;
    DebugArg a[3] = {{x, nullptr, N * 4}, {y, nullptr, N * 4}, {nullptr, out, N * 4}};
    return debug_run("p3d_debug_powf", device, a, [&] { return launch_debug_powf(n, a[0].as<float>(), a[1].as<float>(), a[2].as<float>(), nullptr); });
}

int p3d_debug_pow(int device, uint32_t n, const double* x, const double* y, double* out) {
    if (!x || !y || !out) return fail(P3D_ERR_ARG, "NULL argument");
    if (n == 0) return P3D_OK;
    const size_t N = n;
    DebugArg a[3] = {{x, nullptr, N * 8}, {y, nullptr, N * 8}, {nullptr, out, N * 8}};
    return debug_run("p3d_debug_pow", device, a, [&] { return launch_debug_pow(n, a[0].as<double>(), a[1].as<double>(), a[2].as<double>(), nullptr); });
}

int p3d_debug_schlick_kr(int device, uint32_t n, const float* ior_1, const float* new_ior, const float* cos_theta_i, float* out) {
    if (!ior_1 || !new_ior || !cos_theta_i || !out) return fail(P3D_ERR_ARG, "NULL argument");
    if (n == 0) return P3D_OK;
    const size_t N = n;
    DebugArg a[4] = {{ior_1, nullptr, N * 4}, {new_ior, nullptr, N * 4}, {cos_theta_i, nullptr, N * 4}, {nullptr, out, N * 4}};
    return debug_run("p3d_debug_schlick_kr", device, a, [&] {
        return launch_debug_schlick_kr(n, a[0].as<float>(), a[1].as<float>(), a[2].as<float>(), a[3].as<float>(), nullptr);
    });
}

static int debug_bvh_build(const char* what, uint32_t builder, int device, uint32_t n, const float* lo3, const float* hi3, const uint32_t* ref,
                           uint32_t* nodes16, uint32_t* leaf_refs, uint32_t* stats4, float* sah_cost, PlocInfo* info) {
    if (!lo3 || !hi3 || !ref || !nodes16 || !leaf_refs || !stats4 || !sah_cost) return fail(P3D_ERR_ARG, "NULL argument");
    if (n < 4) return fail(P3D_ERR_ARG, "the device builder needs at least 4 primitives (two leaves)");
    std::vector<BuildPrim> prims(n);
    for (uint32_t i = 0; i < n; i++) {
        memcpy(prims[i].lo, lo3 + 3 * (size_t)i, 12); memcpy(prims[i].hi, hi3 + 3 * (size_t)i, 12);
        prims[i].ref = ref[i]; prims[i].scene_id = i;
    }
    const size_t n_nodes = (n + 1) / 2 - 1;
    BvhStats bs;
    DebugArg a[2] = {{nullptr, nodes16, n_nodes * sizeof(NodePair)}, {nullptr, leaf_refs, (size_t)n * 4}};
    int rc = debug_run(what, device, a, [&] {
        return build_bvh_device(builder, prims, BvhOptions(), a[0].as<NodePair>(), a[1].as<uint32_t>(), bs, info, nullptr);
    });
    if (rc) return rc;
    stats4[0] = bs.n_nodes; stats4[1] = bs.n_leaves; stats4[2] = bs.n_leaf_refs; stats4[3] = bs.max_depth;
    *sah_cost = bs.sah_cost;
    return P3D_OK;
}

int p3d_debug_lbvh_build(int device, uint32_t n, const float* lo3, const float* hi3, const uint32_t* ref, uint32_t* nodes16,
                         uint32_t* leaf_refs, uint32_t* stats4, float* sah_cost) {
    return debug_bvh_build("p3d_debug_lbvh_build", 1u, device, n, lo3, hi3, ref, nodes16, leaf_refs, stats4, sah_cost, nullptr);
}

int p3d_debug_ploc_build(int device, uint32_t n, const float* lo3, const float* hi3, const uint32_t* ref, uint32_t* nodes16,
                         uint32_t* leaf_refs, uint32_t* stats4, float* sah_cost, int32_t* rounds, int32_t* fell_back) {
    if (!rounds || !fell_back) return fail(P3D_ERR_ARG, "NULL argument");
    PlocInfo info;
    int rc = debug_bvh_build("p3d_debug_ploc_build", 2u, device, n, lo3, hi3, ref, nodes16, leaf_refs, stats4, sah_cost, &info);
    if (rc) return rc;
    *rounds = info.rounds; *fell_back = info.fell_back;
    return P3D_OK;
}

int p3d_debug_grid_build(int device, uint32_t n, const float* lo3, const float* hi3, const uint32_t* ref, int32_t* dims3,
                         float* mn3, float* mx3, uint64_t* n_cells, uint64_t* n_items, uint32_t* cell_start, uint64_t cell_cap,
                         uint32_t* items, uint64_t item_cap) {
    if (!dims3 || !mn3 || !mx3 || !n_cells || !n_items || (n > 0 && (!lo3 || !hi3 || !ref))) return fail(P3D_ERR_ARG, "NULL argument");
    std::vector<float> rows(6 * (size_t)n);
    for (size_t i = 0; i < n; i++) { memcpy(&rows[6 * i], lo3 + 3 * i, 12); memcpy(&rows[6 * i + 3], hi3 + 3 * i, 12); }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(P3D_ERR_NO_DEVICE, "no HIP device visible");
    DevBuf<float> d_rows; DevBuf<uint32_t> d_ref, cells, refs;           // freed on every path
    GridDeviceOut G;
    GridDeviceLimit limit = kGridFits;
    const bool sizes_only = !cell_start || !items;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = d_rows.upload(rows);
    if (e == hipSuccess) e = d_ref.upload(std::vector<uint32_t>(ref, ref + n));
    if (e == hipSuccess) e = build_grid_device(d_rows.p, d_ref.p, n, sizes_only, nullptr, G, &limit);
    cells.p = G.cell_start; refs.p = G.items;
    if (e == hipSuccess && limit == kGridFits && !sizes_only) {
        e = hipMemcpy(cell_start, G.cell_start, (size_t)std::min<uint64_t>(cell_cap, G.n_cells + 1) * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && std::min<uint64_t>(item_cap, G.n_items) > 0)
            e = hipMemcpy(items, G.items, (size_t)std::min<uint64_t>(item_cap, G.n_items) * 4, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return fail(P3D_ERR_HIP, std::string("p3d_debug_grid_build: ") + hipGetErrorString(e));
    for (int a = 0; a < 3; a++) { dims3[a] = G.n[a]; mn3[a] = G.mn[a]; mx3[a] = G.mx[a]; }
    *n_cells = G.n_cells; *n_items = G.n_items;
    if (limit == kGridTooManyCells) return fail(P3D_ERR_LIMIT, "the reference's grid formula asks for more than 2^31 cells");
    if (limit == kGridTooManyItems) return fail(P3D_ERR_LIMIT, "the grid's cells hold more than 2^32 - 1 primitive references");
    return P3D_OK;
}

int p3d_debug_rand(int device, uint32_t seed, uint64_t first, uint32_t n, uint32_t* out) {
    if (!out) return fail(P3D_ERR_ARG, "NULL argument");
    if (n == 0) return P3D_OK;
    DebugArg a[1] = {{nullptr, out, (size_t)n * 4}};
    return debug_run("p3d_debug_rand", device, a, [&] { return launch_debug_rand(seed, first, n, a[0].as<uint32_t>(), nullptr); });
}

int p3d_debug_sample_stream(int device, uint32_t seed, int32_t res_x, int32_t res_y, int32_t spp, float aperture, uint64_t pairs_per_pass,
                            float* out, int32_t* passes) {
    if (!out || !passes) return fail(P3D_ERR_ARG, "NULL argument");
    if (res_x < 1 || res_y < 1 || spp < 1) return fail(P3D_ERR_ARG, "res_x, res_y and spp must be at least 1");
    const uint64_t pixels = (uint64_t)res_x * (uint64_t)res_y, per_pixel = (uint64_t)spp * (uint64_t)spp;
    if (pixels > kMaxStackedPixels || per_pixel > kMaxStackedPixels || pixels * per_pixel > kMaxStackedPixels)
        return fail(P3D_ERR_LIMIT, "res_x * res_y * spp * spp does not fit 31 bits");
    SampleStreamScratch scratch;             // freed on every path
    DebugArg a[1] = {{nullptr, out, (size_t)(pixels * per_pixel) * 4 * sizeof(float)}};
    return debug_run("p3d_debug_sample_stream", device, a, [&] {
        return generate_sample_stream(scratch, seed, res_x, res_y, spp, aperture, a[0].as<float>(), pairs_per_pass, passes, nullptr);
    });
}

}  // extern "C"
