// p3d_scene_state.h -- the scene handle behind the C-ABI of include/p3d_hip.h, shared by the files that implement it
// (p3d_scene_create.cpp, p3d_scene_update.cpp, p3d_scene_rebuild.cpp, p3d_scene_build_grid.cpp, p3d_render.cpp, p3d_generate_samples.cpp, p3d_denoise.cpp, p3d_accumulate.cpp, p3d_upsample.cpp, p3d_capi_misc.cpp, p3d_debug_planes.cpp; p3d_ambient_occlusion and p3d_indirect_diffuse live in p3d_render.cpp).  Internal: not installed with include/.
// Every device resource in it is owned by a member that frees it: deleting a p3d_scene releases all of them.
#ifndef P3D_SCENE_STATE_H
#define P3D_SCENE_STATE_H

#include "p3d_hip.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "grid_builder.h"
#include "p3d_device_types.h"
#include "p3d_frame_config.h"
#include "p3d_launch.h"
#include "p3d_tile_coverage.h"
#include "sample_stream.h"

extern "C" int p3d_internal_set_error(int code, const char* msg);   // p3d_capi_misc.cpp: the thread's p3d_last_error()

#pragma GCC visibility push(hidden)
namespace p3d {

static inline int fail(int code, const std::string& msg) { return p3d_internal_set_error(code, msg.c_str()); }

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(P3D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

constexpr size_t kMaxLdsBytes = 160 * 1024;   // gfx950: 160 KiB per CU
constexpr int kMaxDepth = 16;
constexpr size_t kLdsSceneLimit = 24 * 1024;
#ifndef P3D_HBM_STACK_DWORDS
#define P3D_HBM_STACK_DWORDS 64u      // per entry per wave: RefStack 64 (4-byte entries; p3d_traverse.h), SlimStack 96
#endif
constexpr uint32_t kHbmStackDwordsPerEntry = P3D_HBM_STACK_DWORDS;
// 4-byte slots (node references only, p3d_traverse.h) for both scene placements
#ifndef P3D_LDS_STACK_DWORDS
#define P3D_LDS_STACK_DWORDS 64u      // RefStack: 4-byte slots (WideStack: 128)
#endif
constexpr int kLanes = 4;                             // concurrent sample passes of one frame
constexpr unsigned kPersistentWavesNarrow = 256 * 16 * 4;   // ... of HBM-resident scenes (narrow waves, 4 per SIMD)
constexpr int kShards = 64;   // queue shards; spreads the slot-allocation atomics. == the wave size: the deeper-level
                              // kernel holds one shard's count per lane (wf_secondary_kernel)
// counter buffer of a workspace: [level][shard] ray counts, node counts (all cleared by the first launch of a pass),
// then the two alternating level-1 sets and the parity words (LaunchParams::wf_alt)
constexpr size_t kCountWords = (size_t)2 * (kMaxDepth + 2) * kShards;
constexpr size_t kCountBufferWords = kCountWords + 4 * kShards + 64;
constexpr uint64_t kMaxStackedPixels = 0x7FFFFFFFull;   // pixel links are 31 bits (NodeRec / RayRec link, kLinkRefr)
constexpr int kTileOrderPeriod = 64;

// Device memory, freed with its owner.  Move-only.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    ~DevBuf() { release(); }
    hipError_t upload(const std::vector<T>& h) {
        release();
        n = h.size();
        size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) return e;
        if (n) e = hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    size_t bytes() const { return std::max<size_t>(n, 1) * sizeof(T); }
};

struct RawBuf {
    void* p = nullptr;
    size_t cap = 0;
    RawBuf() = default;
    RawBuf(RawBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    RawBuf& operator=(RawBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~RawBuf() { release(); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// A stream / an event of the handle's own, made with kFlags and destroyed with its owner.
template <unsigned kFlags>
struct OwnedStream {
    hipStream_t h = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream() { if (h) (void)hipStreamDestroy(h); }
    hipError_t create() { return hipStreamCreateWithFlags(&h, kFlags); }
    operator hipStream_t() const { return h; }
};
template <unsigned kFlags>
struct OwnedEvent {
    hipEvent_t h = nullptr;
    OwnedEvent() = default;
    OwnedEvent(const OwnedEvent&) = delete;
    OwnedEvent& operator=(const OwnedEvent&) = delete;
    ~OwnedEvent() { if (h) (void)hipEventDestroy(h); }
    hipError_t create() { return hipEventCreateWithFlags(&h, kFlags); }
    operator hipEvent_t() const { return h; }
};
using LaneStream = OwnedStream<hipStreamNonBlocking>;
using TimingEvent = OwnedEvent<hipEventDefault>;
using OrderEvent = OwnedEvent<hipEventDisableTiming>;

// Whether `stream` is being captured into a graph: what waits for the stream or allocates is refused then.
inline bool stream_capturing(hipStream_t stream) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cap);
    return cap != hipStreamCaptureStatusNone;
}

}  // namespace p3d

// Members are destroyed in reverse order of declaration: the streams come first, so they outlive the buffers and events
// used on them.  p3d_scene_destroy() waits for the streams before it deletes the handle.
struct p3d_scene {
    int device = 0;
    p3d::LaneStream own_stream;
    hipStream_t stream = nullptr;         // own_stream, or the caller's (p3d_set_stream): never destroyed here
    p3d::LaneStream lane_stream[p3d::kLanes];   // [0] stays empty: lane 0 is `stream`
    p3d::OrderEvent ev_fork, ev_join[p3d::kLanes];
    p3d::DevBuf<uint32_t> blob;              // powf tables (32 quads) | leaf records | spheres | sphere meta | tris | boxes | materials [| f32 nodes: LDS scenes]
    p3d::DevBuf<p3d::QNode> qnodes;          // 32-byte node pairs: what kernels that read the scene from HBM walk
    float q_scale[3] = {1, 1, 1}, q_base[3] = {0, 0, 0};
    uint32_t blob_quads = 0;
    uint32_t off_nodes = 0, off_leaves = 0, off_spheres = 0, off_sphere_meta = 0, off_tris = 0, off_tri_normals = 0, off_boxes = 0, off_mats = 0;
    p3d::DevBuf<p3d::PlaneRec> planes;
    p3d::DevBuf<p3d::PrimMeta> plane_meta;
    p3d::DevBuf<p3d::LightRec> lights;
    // GRID mode (accel 1): the reference's uniform grid, built from grid_src on the first GRID frame (and on the first
    // one after a p3d_scene_update, which refreshes grid_src: one entry per primitive, in scene order, kept)
    std::vector<p3d::GridPrim> grid_src;
    p3d::DevBuf<uint32_t> grid_cells, grid_items;
    p3d::GridHost grid_info; bool grid_ready = false;
    // p3d_scene_update: where each primitive's record sits (scene index -> kind << 30 | index in the kind's leaf-ordered
    // array; planes index their own), and what the refit needs next to the scene, allocated by the first update.
    // p3d_scene_rebuild replaces the map with the new tree's, and the refit state with that tree's f32 pairs and parents
    p3d::DevBuf<uint32_t> prim_map;
    struct Refit {
        p3d::RawBuf nodes;                   // f32 node pairs of a scene that carries quantised ones only (else: the blob's)
        p3d::RawBuf parent, arrived, status; // per node pair: parent, arrival counter; root boxes + bad-index count
        p3d::RawBuf stage_prims, stage_index;   // host-memory updates pass through these
        bool ready = false;
    } refit;
    // primitives whose grid_src entry predates an update from device memory: GRID mode is refused while there are any
    std::vector<uint8_t> grid_stale; size_t grid_stale_count = 0;
    // p3d_scene_build_grid: GRID mode's box of every primitive ([n_prims][6], scene order), made of grid_src by the first
    // update from device memory or the first device build (grid_device.h: ensure_grid_bounds) and kept current by every
    // update from then on (update_records_kernel); empty until then
    p3d::DevBuf<float> grid_bounds;
    p3d::DevBuf<p3d::LightRec> soft_lights;     // 16 sub-lights per light, built on first use (SOFT_SHADOW, spp == 0)
    p3d::DevBuf<uint8_t> sky;                   // cube map of P3D_FEATURE_SKYBOX: the six faces back to back
    uint32_t sky_off[6] = {0, 0, 0, 0, 0, 0}, sky_w[6] = {0, 0, 0, 0, 0, 0}, sky_h[6] = {0, 0, 0, 0, 0, 0}, sky_bpp[6] = {0, 0, 0, 0, 0, 0};
    std::vector<p3d::LightRec> host_lights;
    size_t lds_scene_limit = p3d::kLdsSceneLimit;  // blobs up to this size are rendered from an LDS copy
    bool lds_capable = false;            // ... and then carry the f32 nodes the LDS walk reads
    int last_schedule = -1;
    int32_t builder = 0;                 // whose tree the handle walks: 0 host SAH, 1 device LBVH, 2 device clustering (p3d_scene_last_builder)
    bool unit_rays_only = false;         // built with cull_never_hit: cannot serve un-normalised (NONE-mode) shadow rays
    bool cull_never_hit = false;         // ... the option itself, whether or not it found a triangle to leave out: ray streams are refused
    uint32_t packet_node_limit = 64;     // trees up to this many node pairs use the wave-wide walk
    float bg[3] = {0, 0, 0};
    uint32_t n_lights = 0, n_materials = 0;
    p3d_scene_stats stats{};
    p3d::RawBuf fb_rgb8, fb_rgb32f, fb_hit, samples;
    p3d::RawBuf fb_depth, fb_normal, fb_albedo;   // host-memory AOV planes of p3d_render_aov are staged here, like hit_id in fb_hit
    p3d::RawBuf ray_tab; int tab_res_x = 0, tab_res_y = 0;   // cached per-column / per-row ray factors
    // Wavefront workspaces: ray queues (levels 2..D), parked nodes (levels 1..D-1), counters.
    // A frame of several sample passes (spp > 0) runs up to kLanes passes at a
    // time, each on its own stream with its own queues: the latency-bound deep levels and launch tails
    // of one pass fill with another pass's work, like independent frames do.  Lane 0 is the scene's stream.
    struct Workspace {
        p3d::RawBuf rays[p3d::kMaxDepth + 2], nodes[p3d::kMaxDepth + 2], counts;   // counts: cleared by a kernel in front of every pass
        p3d::RawBuf rng[p3d::kMaxDepth + 2];     // random-stream keys of the queued rays (stochastic features)
        size_t held() const {
            size_t b = 0;
            for (auto& q : rays) b += q.cap;
            for (auto& q : nodes) b += q.cap;
            for (auto& q : rng) b += q.cap;
            return b;
        }
    } ws[p3d::kLanes];
    p3d::RawBuf wf_planes;                   // [sample][local px][3] clamped sample colours (spp > 0)
    // tile schedule: (resident workgroups) x (one 16x16 tile's worst-case queues), and the tile counter + exit
    // ticket the kernel re-arms itself (zeroed once, at allocation)
    p3d::RawBuf tile_ws, tile_ctrl;
    // "heaviest tile first" for scenes read from HBM: per-tile durations written by the tile kernel, and the order made of
    // them after the first frame of a configuration and every kTileOrderPeriod frames from then on (all on the frame's stream)
    struct TileOrder {
        p3d::RawBuf cost, sorted, iota, order, temp;   // sized for key's tile count
        size_t temp_bytes = 0;
        p3d::Keyed<p3d::TileOrderKey> key;
        bool valid = false;          // `order` holds an order for `key`
        int frames = 0;              // frames rendered since it was made
    } tile_lpt, wave_lpt;            // 16x16 tiles of the tile schedule / 16x4 wave tiles of the tree and wavefront level-1 launches
    TileOrder tile_lpt_batch, wave_lpt_batch;   // ... of frame batches (p3d_render_frames), keyed on n and the tile count too
    bool tile_lpt_enabled = true;
    // cached occupancy queries ([without / with AOV planes][private / shared walk]), keyed by the build they were made for
    // (walk -1: none yet): alternating p3d_render and p3d_render_aov asks for neither again
    struct { p3d::KernelVariant v = {false, false, -1}; size_t lds = 0; int blocks = 0; } tile_occ[2][2];
    struct { p3d::KernelVariant v = {false, false, -1}; uint32_t stack = 0; unsigned waves = 0; } wf_occ;   // ... of the deeper-level kernel
    // upper limit of the workspace one frame may allocate (wavefront schedule: worst-case level queues of a band
    // of tile rows; tile schedule: one slot per resident workgroup).  64 GiB holds BASELINE config 4's wavefront
    // queues (4096^2, depth 6: 58 GB worst case) in one band: 10.7 -> 9.3 ms against 8 GiB.
    size_t workspace_budget = (size_t)64 << 30;
    // what of that budget this device can actually give: re-read (hipMemGetInfo) whenever the budget or the frame
    // configuration changes, so that several scene handles, or a framework holding most of the HBM, shrink the
    // bands / fall back to another schedule instead of failing in hipMalloc
    size_t budget_avail = 0; p3d::Keyed<p3d::BudgetKey> budget_key;
    // Ray streams (p3d_trace_rays) keep their state apart from the frames': staging for host rays and host outputs (counted
    // in device_bytes as it grows), and their own reading of the budget.  Nothing above is keyed on, or changed by, a stream (the workspaces ws[0] are scratch that
    // only grows; the occupancy cache wf_occ is keyed by the build it describes).
    struct RayStream {
        p3d::RawBuf origin, dir, rgb32f, hit_id, t, normal;
        p3d::RawBuf occluded;                // p3d_occluded stages host segments in origin / dir and host answers here
        size_t budget_avail = 0; p3d::Keyed<p3d::RayStreamKey> key;
    } rays;
    // p3d_generate_samples: jump tables and the summaries of the pass in flight (counted in device_bytes as they grow)
    p3d::SampleStreamScratch sample_stream;
    // p3d_denoise: the two colour buffers the passes alternate between, and the staging of host planes (all counted in
    // device_bytes as they grow).  p3d_denoise_variance: the same, the scratch with the variance behind the colour.
    struct Denoise {
        p3d::RawBuf scratch[2];
        p3d::RawBuf in_rgb32f, in_depth, in_normal, in_albedo, out_rgb32f, out_rgb8;
        p3d::RawBuf in_variance, out_variance;       // p3d_denoise_variance: the host variance planes
    } denoise;
    // p3d_accumulate: the staging of host planes (frames, history, outputs) and the two frames of an output plane the
    // caller does not want but the next frame reads (all counted in device_bytes as they grow).  No history is kept.
    struct Accumulate {
        p3d::RawBuf in_rgb32f, in_depth, in_normal, in_hit_id;
        p3d::RawBuf hist_rgb32f, hist_depth, hist_normal, hist_length, hist_hit_id;
        p3d::RawBuf out_rgb32f, out_length, spare_rgb32f, spare_length;
        p3d::RawBuf motion_type, motion_data, motion_hist, out_prev_xy;      // p3d_accumulate_moving: host geometry and the host prev_xy plane
        p3d::RawBuf hist_moments, out_moments, out_variance, spare_moments;  // p3d_accumulate_variance: the host planes it adds, and the moments the caller does not want
    } accumulate;
    // p3d_ambient_occlusion: the staging of host planes and the frames' cameras (FrameCam records, written on the stream
    // by every call: launch_frame_cams); all counted in device_bytes as they grow.  Apart from the frames' frame_cams.
    struct AmbientOcclusion {
        p3d::RawBuf in_depth, in_normal, in_rgb32f, out_ao, out_rgb32f, cams;
    } ao;
    // p3d_indirect_diffuse: the same for its planes; all counted in device_bytes as they grow.
    struct IndirectDiffuse {
        p3d::RawBuf in_depth, in_normal, in_albedo, in_rgb32f, out_indirect, out_rgb32f, cams;
    } indirect;
    // p3d_upsample: the staging of host planes (counted in device_bytes as they grow).  The filter itself needs no scratch.
    struct Upsample {
        p3d::RawBuf in_low, in_low_depth, in_low_normal, in_depth, in_normal, out_plane, out_fallback;
    } upsample;
    p3d::RawBuf d_counters;             // one DeviceCounters
    bool counters_valid = false;
    p3d::TimingEvent ev0, ev1;
    p3d::TimingEvent ev_prof[4];         // frame begin/end, dominant kernel begin/end
    p3d::SchedulePick pick, pick_batch;  // one frame (p3d_render) / frame batches (p3d_render_frames: n is in the key)
    // p3d_tune_schedule(): a candidate forced for the frames it times, the winner to adopt at the next frame, and what the
    // most recent frame's measured choice had to choose from (0: the choice is made by rule or by a flag)
    int tune_force = -1, tune_commit = -1, tune_candidates = 0;
    uint32_t tune_avail = 0;
    p3d::TimingEvent ev_pick[2], ev_pick_batch[2];
    // per-frame cameras of a batch (FrameCam records), written on the frame's stream by every batch (launch_frame_cams)
    p3d::RawBuf frame_cams;
    bool profile_valid = false;
    bool timer_open = false;
    int xcd_chunk = 1;
    int frame_streams = 1;               // bands of a one-sample frame run concurrently on this many streams (experiment knob)
    int resolve_blocks_per_shard = 16;   // a resolve launch is latency-bound: few nodes per thread, many threads
    int fused_resolve_shard_px = 8192;   // frames with at most this many pixels per shard resolve all levels in one launch
    bool pair_mode = true;               // the last level combines sibling rays with their parent (LaunchParams::wf_pair_in)
    uint32_t dbg_skip = 0;               // diagnostic builds only (LaunchParams::dbg_skip)
    unsigned long long* dbg_stamps = nullptr; int dbg_stamp_level = 1;   // the caller's buffer (p3d_debug_set_stamps)
    int occupancy = 0;     // 0 = compiler default register budget, else 5 / 6 / 8 waves per SIMD
    int primary_tiles = p3d::kDefaultPrimaryTiles;   // 16x16 tiles a workgroup of the level-1 launch runs (p3d_set_primary_tiles)
    int last_primary_tiles = 1;                      // ... and what the most recent render's level-1 launch ran with
    // The tile coverage mask of a frame (p3d_tile_coverage.h, p3d_set_sky_tiles): [tiles_y][row_words] mask words, then
    // [tiles_y] status words, written by a pre-pass on the frame's stream.  last_sky: the geometry of the most recent
    // render's mask (on = it had one); what the device marked is read back only when p3d_last_sky_tiles() asks.
    bool sky_tiles = p3d::kDefaultSkyTiles;
    p3d::RawBuf sky_mask;
    struct { bool on = false; p3d::CoverTiles tiles{}; uint32_t row_words = 0; } last_sky;
    // p3d_set_prune_reflections: what the caller asked for, and whether the scene as created lets it apply (finite_scene:
    // every material, light, background and flattened normal component is finite).  Frames prune when both hold.
    // The kernels learn it from the material records (p3d_shade.h: shade_hit): host_materials is the caller's materials,
    // blob_prunes says which encoding of them the scene blob holds (p3d_scene_create.cpp: encoded_materials).
    bool prune_reflections = p3d::kDefaultPruneReflections;
    bool finite_scene = true;
    bool prunes() const { return prune_reflections && finite_scene; }
    std::vector<p3d::MaterialRec> host_materials;
    bool blob_prunes = false;
    // p3d_last_level_rays: the most recent wavefront-schedule frame (or ray stream) of the handle -- its depth, its level-1
    // rays and how many passes it ran on how many lanes (every lane's counters keep its last pass).  valid = false before the
    // first one and after a tile or tree frame.
    struct { bool valid = false; int D = 0, lanes = 0; size_t passes = 0; uint64_t level1 = 0; } last_wf;
    uint32_t tri_quads = 3;    // 16-byte quads per triangle test record (3; 4 = round 2's 64-byte stride, P3D_TRI_STRIDE=64)
    bool verbose = false;      // P3D_VERBOSE=1: launch geometry on stderr (diagnostic)
    int share_min_idle = 16;   // work-sharing walk of scenes read from HBM: idle lanes before a steal round (0 or > 64: private walks)
};
#pragma GCC visibility pop

#endif
