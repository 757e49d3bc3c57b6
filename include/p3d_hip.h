/*
 * p3d_hip.h -- C-ABI of the MI355X-native Whitted renderer (libp3d_hip.so).
 *
 * The reference (P3D_RayTracer_Template2, RT/ = /root/reference/P3D_RayTracer_Template2/)
 * has no plugin/FFI surface: its hot path is one function, renderScene() (RT/main.cpp:732),
 * reached through globals.  This header is the boundary a maintainer binds instead of that
 * loop: plain pointers and sizes only, no C++ or torch types.  Each entry point names the
 * reference code it replaces.  INTEGRATION.md shows the reference-side call sites.
 *
 * Conventions
 *   - every function returns 0 on success or a negative p3d_status; p3d_last_error()
 *     describes the failure (the reference prints and exit()s, RT/main.cpp:827; the library
 *     never exits the process);
 *   - the caller owns every host buffer; the library owns device memory behind p3d_scene;
 *   - a p3d_scene is bound to one HIP device and must not be used from two threads at once;
 *   - render calls are asynchronous on the scene's HIP stream; p3d_sync() or a host-memory
 *     download waits for them.
 */
#ifndef P3D_HIP_H
#define P3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_ABI_VERSION 4

typedef enum p3d_status {
    P3D_OK = 0,
    P3D_ERR_ARG = -1,        /* bad argument / inconsistent sizes                       */
    P3D_ERR_HIP = -2,        /* a HIP runtime call failed                               */
    P3D_ERR_NO_DEVICE = -3,  /* no usable gfx950 device                                 */
    P3D_ERR_LIMIT = -4,      /* scene exceeds a kernel limit (LDS stack, depth)         */
    P3D_ERR_STATE = -5,      /* call made in the wrong state                            */
    P3D_ERR_COMM = -6        /* an RCCL call failed                                     */
} p3d_status;

/* primitive kinds, RT/scene.h:67-145 */
enum { P3D_SPHERE = 0, P3D_TRIANGLE = 1, P3D_BOX = 2, P3D_PLANE = 3 };

/* accelerator enum of RT/scene.h:18; selects the SHADOW-RAY semantics:
 * NONE = un-normalised direction, no distance bound; GRID/BVH = normalised, t < |L|.
 * Closest hits are always "nearest, lowest scene index on ties" (SURVEY Q1). */
enum { P3D_ACCEL_NONE = 0, P3D_ACCEL_GRID = 1, P3D_ACCEL_BVH = 2 };

/* Flattened scene in SCENE ORDER (the order Scene::addObject saw, RT/scene.cpp:302).
 * prim_data holds 12 floats per primitive:
 *   sphere   c.x c.y c.z r                    (RT/scene.h:116-131)
 *   triangle P0 P1 P2                         (RT/scene.cpp:10)
 *   box      min max                          (RT/scene.cpp:188)
 *   plane    PN.x PN.y PN.z D                 (unit normal and offset, RT/scene.cpp:95-115)
 * materials hold 12 floats: diffuse rgb, Kd, specular rgb, Ks, shine, T, ior, reflection
 * (RT/scene.h:23-55; reflection == Ks for loader-made materials, RT/scene.h:31).
 * lights hold 6 floats: position xyz, colour rgb (RT/scene.h:57-65). */
typedef struct p3d_scene_desc {
    uint32_t        n_prims;
    const uint32_t* prim_type;
    const float*    prim_data;
    const uint32_t* prim_material;
    uint32_t        n_materials;
    const float*    materials;
    uint32_t        n_lights;
    const float*    lights;
    float           background[3];   /* Scene::GetBackgroundColor, RT/scene.h:155 */
} p3d_scene_desc;

/* BVH construction knobs (replaces BVH::Build, RT/bvh.cpp:28-158; the tree need not match
 * the reference's because its closest-hit result is discarded). */
typedef struct p3d_build_opts {
    uint32_t leaf_max;        /* max primitives per leaf, 1..8; 0 = default (4)          */
    uint32_t sah_bins;        /* 0 = default (16)                                       */
    uint32_t builder;         /* 0 = binned SAH on the host (default); 1 = linear BVH built on the
                                 device (Morton sort + Karras hierarchy + refit): a tree of lower
                                 quality in a fraction of the time, for scene-reload loops and
                                 scenes of millions of primitives. 2 = built on the device by local
                                 clustering over builder 1's sorted leaves (csrc/bvh_ploc.hip): a tree
                                 near the SAH tree's cost, at builder 1's node and leaf counts; when the
                                 clustering does not finish in 95 rounds the tree is builder 1's
                                 (p3d_scene_last_builder tells). Above 2: P3D_ERR_ARG. Scenes of fewer
                                 than 64 bounded primitives are built on the host whatever this says.
                                 Same images either way.                                       */
    uint32_t cull_never_hit;  /* 1 = leave out of the BVH every triangle the reference's own test can
                                 never accept: Triangle::intercepts rejects |det| < 1e-3
                                 (RT/scene.cpp:66-67) and |det| <= |d| * |e1 x e2|, so a
                                 triangle with sqrt(2) * |e1 x e2| below that threshold is invisible to
                                 every ray whose direction is at most sqrt(2) long -- all closest-hit
                                 rays (the odd refraction ray of SURVEY Q6 reaches sqrt(2)) and the
                                 normalised shadow rays of GRID / BVH mode. NONE-mode shadow rays are
                                 not normalised, so p3d_render() rejects accel NONE on such a scene.
                                 Same images, same ray counts, fewer box / triangle tests. Default 0:
                                 every primitive is traversed, like in the reference.            */
} p3d_build_opts;

/* The values Camera::Camera derives (RT/camera.h:35-73); PrimaryRay (RT/camera.h:91-127)
 * is evaluated on the device from these. */
typedef struct p3d_camera {
    float   eye[3], u[3], v[3], n[3];
    float   w, h, plane_dist;
    float   aperture;        /* lens aperture in world units, RT/camera.h:65            */
    float   focal_ratio;
    int32_t res_x, res_y;
} p3d_camera;

typedef struct p3d_render_params {
    int32_t  max_depth;      /* MAX_DEPTH, RT/main.cpp:34                                */
    int32_t  accel;          /* P3D_ACCEL_*: shadow-ray semantics, RT/main.cpp:476-510  */
    int32_t  spp;            /* 0 = Whitted one sample at pixel centre; n = n*n samples
                                with thin lens, summed and divided by 16   */
    const float* samples;    /* spp>0: HOST array [res_y][res_x][spp*spp][4] =
                                pixel sample x, y, lens x, lens y in reference RNG order
                                (RT/main.cpp:776-801); uploaded by the call.  p3d_generate_samples
                                makes the same array on the device (P3D_FLAG_DEVICE_SAMPLES) */
    /* image-space sharding: this device renders the row blocks b with
     * b % world == rank, row_block rows each, into a COMPACT buffer of
     * p3d_local_rows() rows.  world = 1 renders the whole frame. */
    int32_t  row_block;      /* rows per block, multiple of 16; 0 = default (16)         */
    int32_t  rank, world;
    uint32_t flags;          /* P3D_FLAG_*                                              */
    uint32_t features;       /* P3D_FEATURE_*: the reference's distribution-ray-tracing switches */
    uint32_t seed;           /* seed of the device random streams those features draw from       */
} p3d_render_params;

/* SOFT_SHADOW / FUZZY_REFLECTION of RT/main.cpp:41,43 (compile-time false there).
 * SOFT_SHADOW: every light becomes the reference's 0.5 x 0.5 area light -- with spp == 0 its
 * deterministic 4x4 grid of sub-lights of colour/16 (RT/main.cpp:601-618, bit-faithful), with
 * spp > 0 one jittered position per pixel sample in that sample's stratum (RT/main.cpp:620-624).
 * FUZZY_REFLECTION: mirror directions perturbed inside a sphere of radius 0.3 (RT/main.cpp:651-660).
 * The jitter and the fuzz draw from counter-based device random streams keyed by (seed, pixel, sample,
 * tree node): the reference's serial rand() stream is not reproducible in parallel, so these two are
 * statistically, not bitwise, equal to it. They need the wavefront schedule (P3D_FLAG_TREE_KERNEL is
 * rejected). DEPTH_OF_FIELD is implied by spp > 0 as in the reference (RT/main.cpp:943-944);
 * MOTION_BLUR only stamps rays with a time no object reads, so it has no switch. */
#define P3D_FEATURE_SOFT_SHADOW 1u
#define P3D_FEATURE_FUZZY_REFLECTION 2u
/* A ray that hits nothing returns Scene::GetSkyboxColor(ray) (RT/scene.cpp:383-461) from the cube map given to
 * p3d_scene_set_skybox() instead of the background colour.  The reference holds this function and the `env` loader
 * command (RT/scene.cpp:652-658) but never calls the former -- its rayTracing() returns bgColor on a miss
 * (RT/main.cpp:582) -- so this switch is what the function is evidently there for, off by default.
 * The lookup itself is bit-exact against the reference's object code (tests/test_oracle_vs_ref.py).  Like the other
 * features it needs the tile or the wavefront schedule. */
#define P3D_FEATURE_SKYBOX 4u
/* SCHLICK_APPROX of RT/main.cpp:99 (false there): the Fresnel weight of a transmissive hit becomes Schlick's
 * approximation KR = rI + (1 - rI) * pow(1 - cos_theta_i, 5), rI = ((ior_1 - newIor) / (ior_1 + newIor))^2
 * (RT/main.cpp:699-702), instead of the default 1 / 2 * (R0 + R1) -- an integer 1 / 2, so 0: with the switch
 * glass shows its reflection.  Under total internal reflection KR stays 0 (RT/main.cpp:710).  No random draws: the
 * frames equal the reference's in every float bit -- the device runs glibc's double pow algorithm (csrc/p3d_pow.h) and
 * g++'s operation order -- on all three schedules, and combine with every other switch, samples and sharding. */
#define P3D_FEATURE_SCHLICK 8u

#define P3D_FLAG_COUNTERS 1u     /* accumulate p3d_counters on the device (slower kernels)  */
/* Kernel schedules: three ways to run the same per-node code, bit-identical frames.  Which one p3d_render() uses
 * when none is forced (p3d_last_schedule() reports it):
 *   - scenes whose flattened records fit 24 KiB are rendered from an LDS copy, and go BY RULE: one-sample frames
 *     (spp == 0) the wavefront schedule, sample loops (spp > 0) the tile schedule;
 *   - every other scene is read from HBM / L2 and the choice is MEASURED per configuration (resolution, depth, accel,
 *     spp, rank / world, flags): the first six frames of a configuration run the wavefront, tree and tile schedules
 *     twice each (first run untimed: code-object load, workspace allocation; a schedule whose workspace does not fit
 *     is skipped), the fastest one stays.  During those frames p3d_render() WAITS on a HIP event for the previous
 *     frame's timing even when p3d_outputs::memory == 1, i.e. it is not asynchronous; a frame issued while the stream
 *     is being captured measures nothing and uses the choice already made (the tile schedule if there is none yet).
 * A schedule whose workspace does not fit the budget falls back tile -> wavefront (in bands) -> tree.
 * One scene handle carries ONE frame at a time per stream: its workspace and the parity words of its queues are
 * ordered by the stream only, so a caller must not issue frames of one handle on two streams concurrently (use one
 * handle per stream, as bench.py does).  At most one of the three forcing flags may be set. */
#define P3D_FLAG_TILE_KERNEL 64u /* ONE launch per frame: persistent 256-thread workgroups draw 16x16-pixel tiles and
                                    run a tile's whole ray tree level by level among themselves (queues in a
                                    private workspace slot, counters in LDS, no global atomics between levels)  */
#define P3D_FLAG_WAVEFRONT 32u   /* one launch per tree level over the whole frame + resolve launches          */
#define P3D_FLAG_DEVICE_SAMPLES 128u /* p3d_render_params::samples is a DEVICE pointer on the scene's device (same
                                    layout): the caller uploaded the sample array once instead of per call    */
#define P3D_FLAG_PROFILE 16u     /* bracket the frame and its dominant kernel (the level-1 /
                                    tree launch) with HIP events for p3d_get_profile()           */
#define P3D_FLAG_PRIVATE_WALK 8u /* scenes read from HBM: every lane walks the BVH for its own ray only.  Without it the
                                    lanes of a wave may SHARE their walks -- idle lanes take over pending subtrees of busy
                                    ones, results merged by minimum over (t, scene id) / OR: same hits, same bits -- and
                                    whether they do is part of the measured schedule choice                              */
#define P3D_FLAG_PACKET_WALK 256u /* wave-wide (packet) BVH walk for trees of up to 64 node pairs: node and primitive
                                    records fetched once per wave, a node visited when any lane's slab test passes.
                                    Same results as the default per-lane walk; measured slower since the leaves
                                    became typed runs (0.137 vs 0.133 ms on BASELINE config 2)                       */
#define P3D_FLAG_NO_LDS_SCENE 4u /* read the scene from HBM/L2 even when it would fit in LDS    */
#define P3D_FLAG_TREE_KERNEL 2u  /* one launch, each lane walks its pixel's whole tree with a post-order frame
                                    stack (LDS, or private memory for scenes read from HBM); also the last
                                    fallback when neither the tile nor the wavefront workspace fits the budget */

/* Work counters in the unit of SURVEY §8d (one ray = one closest-hit or shadow query). */
typedef struct p3d_counters {
    uint64_t closest_queries;
    uint64_t shadow_queries;
    uint64_t box_tests;      /* node AABB slab tests (32 algorithmic bytes each)         */
    uint64_t sphere_tests;   /* 16 B each                                               */
    uint64_t tri_tests;      /* 48 B each                                               */
    uint64_t aabox_tests;    /* 32 B each                                               */
    uint64_t plane_tests;    /* 16 B each                                               */
    uint64_t pixels;
} p3d_counters;

/* Output planes. Pointers may be NULL. memory: 0 = host pointers (the call copies and
 * returns after the frame is complete), 1 = device pointers on the scene's device (the
 * call only enqueues the kernel). A plane holds res_y rows when world == 1 and
 * p3d_local_rows() rows (this rank's compact shard) when world > 1. Layout follows img_Data / colors of RT/main.cpp:70-76:
 * row 0 is the BOTTOM row; rgb8 is 3 bytes per pixel, rgb32f 3 floats per pixel (clamped
 * colour before quantisation), hit_id the scene index of the primary hit or -1. */
typedef struct p3d_outputs {
    uint8_t* rgb8;
    float*   rgb32f;
    int32_t* hit_id;
    int32_t  memory;
} p3d_outputs;

typedef struct p3d_scene p3d_scene;

typedef struct p3d_scene_stats {
    uint32_t n_nodes, n_leaves, max_depth, n_leaf_refs;
    uint32_t n_spheres, n_triangles, n_boxes, n_planes, n_culled;
    uint64_t device_bytes;
    float    sah_cost;
} p3d_scene_stats;

int         p3d_abi_version(void);
const char* p3d_last_error(void);
int         p3d_device_count(int* count);

/* Replaces init_scene()'s accelerator set-up (RT/main.cpp:912-936) and BVH::Build
 * (RT/bvh.cpp:28): flattens nothing (the caller did), builds the BVH on the host, uploads
 * scene + BVH to `device`. opts may be NULL.  The uniform grid of GRID mode (Grid::Build, RT/grid.cpp:30) is
 * built and uploaded by the first p3d_render() with accel == P3D_ACCEL_GRID -- a one-off synchronous cost of that
 * frame; such a frame is refused (P3D_ERR_STATE) while the stream is being captured. */
int p3d_scene_create(const p3d_scene_desc* desc, const p3d_build_opts* opts, int device,
                     p3d_scene** out);
int p3d_scene_destroy(p3d_scene* scene);
/* Replaces Scene::LoadSkybox (RT/scene.cpp:333-381; DevIL image loading stays with the caller): the six faces in the
 * reference's order right, left, top, bottom, front, back, each res_x[i] x res_y[i] pixels of bytes_per_pixel[i] (3 or
 * 4) bytes, rows bottom-up (the reference loads them with a lower-left origin).  HOST pointers; copied to the device. */
int p3d_scene_set_skybox(p3d_scene* scene, const uint8_t* const faces[6], const uint32_t res_x[6], const uint32_t res_y[6],
                         const uint32_t bytes_per_pixel[6]);
int p3d_scene_get_stats(const p3d_scene* scene, p3d_scene_stats* out);

/* Primitives to move, and optionally the lights, of an existing scene handle. */
typedef struct p3d_prim_update {
    uint32_t        n;          /* primitives to replace; 0 is allowed                                   */
    const uint32_t* index;      /* [n] scene indices (p3d_scene_desc order); NULL = primitives 0..n-1    */
    const float*    prim_data;  /* [n][12], the form p3d_scene_desc::prim_data has for that primitive's kind */
    int32_t         memory;     /* 0 host, 1 device pointers on the scene's device (index and prim_data)  */
    const float*    lights;     /* NULL, or [n_lights][6] position + colour of ALL lights: HOST memory always */
} p3d_prim_update;
/* What a render loop with moving spheres, triangles, boxes, planes or lights calls instead of destroying the handle and
 * creating a new one per frame (the reference has no such loop: its scene is loaded once, RT/main.cpp:912-936).  The new
 * records are written on the device and the BVH is REFITTED there: same topology, new boxes.
 *  - equality of frames: after the call every entry -- p3d_render, p3d_render_frames, p3d_trace_rays; every accel mode,
 *    schedule, flag and feature; LDS and HBM placement, sharding, samples -- produces what a handle created from the
 *    updated description produces, in every bit (a closest hit is "nearest, lowest scene index on ties" whatever the
 *    tree).
 *  - what may change: geometry, and the lights' positions and colours.  Kind, material, primitive count, material table,
 *    number of lights and background stay what they were at creation.
 *  - tree quality: the tree keeps the topology it was built with, so its quality degrades as primitives move away from
 *    where they were; frames stay equal and get slower.  p3d_scene_rebuild (below) is the remedy.  The statistics keep
 *    creation's sah_cost; device_bytes grows by what the first update allocates (f32 nodes of scenes read from HBM, one
 *    parent and one counter word per node pair, staging for host-memory updates).  The first update from DEVICE memory also
 *    allocates GRID mode's box of every primitive, 24 bytes each (what p3d_scene_build_grid builds from); every update
 *    after it, from either memory, keeps those boxes current in the kernel that writes the records.
 *  - ordering: runs after everything already enqueued on the scene's stream, and returns when scene and tree are
 *    consistent; it waits on the device (the root's boxes come back to set the quantisation grid).
 *  - stream capture: refused with P3D_ERR_STATE while the stream is being captured.  A graph captured BEFORE an update
 *    must be captured again: the quantisation grid of scenes read from HBM travels in the launch parameters by value.
 *  - P3D_ERR_ARG: NULL scene or update; n > 0 with a NULL prim_data; memory outside 0 and 1; for host memory an index
 *    >= the primitive count (with a NULL index: n above it), checked before anything is changed.  For device memory such
 *    entries are skipped on the device: the call leaves a consistent tree and THEN returns P3D_ERR_ARG.  With duplicate
 *    indices, which of their values holds is unspecified; results for non-finite data are unspecified.
 *  - a handle created with cull_never_hit is refused with P3D_ERR_STATE: a moved triangle may no longer be one the
 *    reference can never hit.
 *  - GRID mode: the uniform grid's shape is observable (RT/grid.cpp:265-309), so the update drops the built grid and the
 *    next GRID frame builds it again from the new points, under the rule of the first GRID frame (p3d_scene_create).
 *    The host needs the points for that: after an update from DEVICE memory, GRID-mode frames and ray streams are refused
 *    with P3D_ERR_STATE until updates from host memory have covered those primitives, or call p3d_scene_build_grid (below),
 *    which builds the grid on the device.  BVH and NONE mode have no such limit.
 *  - lights: all of them are replaced; the 4x4 sub-lights of P3D_FEATURE_SOFT_SHADOW follow on next use.
 *  - the handle's other state stays: the measured schedule choice, the learned tile orders (predictions, never results),
 *    p3d_last_schedule() and the ray-stream state.  A frame after an update measures nothing again. */
int p3d_scene_update(p3d_scene* scene, const p3d_prim_update* update);

/* What p3d_scene_rebuild did, and the tree the handle walks after it. */
typedef struct p3d_rebuild_info {
    uint32_t rebuilt;          /* 1 = the handle walks a new tree; 0 = nothing was changed (see below) */
    uint32_t n_nodes, n_leaves, max_depth;   /* of the tree the handle walks after the call */
    float    sah_cost_before;  /* SAH cost of the tree as it stood (refitted boxes), creation's units */
    float    sah_cost_after;   /* == p3d_scene_stats::sah_cost after the call */
} p3d_rebuild_info;
/* The other half of "refit while the frame time holds, rebuild when it no longer does": the tree of a live handle is built
 * again, on the device, from the primitive records the handle holds there -- no host copy of the geometry is needed (updates
 * may have come from device memory) and no new handle is made.  info may be NULL.
 *  - equality of frames: after the call every entry -- p3d_render, p3d_render_frames, p3d_render_aov, p3d_trace_rays; every
 *    accel mode, schedule, flag and feature; sharding, samples -- produces, in every bit, what it produced before the call,
 *    and hence what a handle freshly created from the current geometry produces (a closest hit is "nearest, lowest scene
 *    index on ties" whatever the tree).  Only speed changes.
 *  - which tree: the device builder's (Morton sort, leaves of two, Karras hierarchy: p3d_build_opts::builder == 1) over the
 *    padded bounds of the records as they are now, the primitives enumerated in scene order with the planes left out, so
 *    that ties between equal Morton keys break the way they do at creation.  A handle created with the host SAH builder may
 *    be rebuilt too: it trades the SAH tree's quality for a tree that fits the moved geometry.
 *  - what is kept: the measured schedule choice, the learned tile orders (predictions, never results), p3d_last_schedule(),
 *    the ray-stream state, the stream, tuning, the skybox, the lights, the materials, and which primitives' points the host
 *    lacks for GRID mode (p3d_scene_update from device memory).
 *  - what changes: the order of the records inside the handle (leaf order of the new tree), the map from scene index to
 *    record, leaf records, node arrays and the quantisation grid; of p3d_scene_stats n_nodes, n_leaves, n_leaf_refs,
 *    max_depth, sah_cost and device_bytes; the refit state (the next p3d_scene_update climbs the new topology).  A built
 *    uniform grid is dropped, as by an update: the next GRID frame builds it again (after updates from device memory it is
 *    refused as before the rebuild: cover those primitives from host memory, or call p3d_scene_build_grid).
 *  - ordering: runs after everything already enqueued on the scene's stream, waits on the device and returns when the handle
 *    is consistent; what the handle held before is freed only after that wait.
 *  - stream capture: refused with P3D_ERR_STATE while the stream is being captured.  A graph captured BEFORE a rebuild must be
 *    captured again: the scene's addresses and the quantisation grid travel in the launch parameters by value.
 *  - a handle created with cull_never_hit is refused with P3D_ERR_STATE, as by p3d_scene_update.  P3D_ERR_ARG: NULL scene.
 *    P3D_ERR_HIP when device memory runs out: every allocation is made before anything of the handle changes, so the handle
 *    is then what it was.
 *  - handles left alone: scenes served from an LDS copy, and scenes with fewer than 64 bounded primitives (which creation
 *    builds on the host whatever the builder asked for), keep their tree: P3D_OK, rebuilt == 0, statistics unchanged,
 *    sah_cost_before == sah_cost_after == the current cost.  Their tree is a few hundred node pairs walked from LDS; their
 *    layout carries a record per leaf and the f32 nodes, and growing it could push the scene out of LDS and change which
 *    kernels serve it. */
int p3d_scene_rebuild(p3d_scene* scene, p3d_rebuild_info* info);
/* p3d_scene_rebuild with the device builder named: builder == 1 is p3d_scene_rebuild exactly (which is a call of this entry);
 * builder == 2 builds the clustered tree of p3d_build_opts::builder == 2 over the same sorted leaves.  Anything else is
 * P3D_ERR_ARG: builder 0 needs the host's geometry.  Every rule above carries over -- equal frames, what is kept and what
 * changes, the refusals, every allocation before any change, the handles left alone (rebuilt == 0) -- with one difference:
 * builder 2 waits on the device once per clustering round (about 50 to 60 short waits on a real scene, 95 at the most)
 * instead of twice in all.  When the clustering does not finish in 95 rounds the tree is builder 1's; rebuilt is 1 then too
 * and p3d_scene_last_builder answers 1. */
int p3d_scene_rebuild_with(p3d_scene* scene, uint32_t builder, p3d_rebuild_info* info);
/* The builder whose tree the handle walks now: 0 = host SAH (also every scene under 64 bounded primitives), 1 = device LBVH
 * (also a builder-2 request that fell back), 2 = the clustered tree.  A handle a rebuild left alone keeps its value.
 * P3D_ERR_ARG: NULL argument. */
int p3d_scene_last_builder(const p3d_scene* scene, int32_t* builder);
/* SAH cost of the tree the handle walks NOW, in the unit of p3d_scene_stats::sah_cost: per node pair 1.2 x the area of its
 * own box (the union of its two child boxes), per leaf the primitive count x the area of the leaf's box, both over the root's
 * area.  After updates it tells what the refitted boxes cost; p3d_scene_stats keeps the cost of the last build.  One
 * reduction over the f32 node pairs (float sums in no fixed order: equal to a few ulps per thousand nodes between calls); a
 * handle read from HBM that was never updated nor rebuilt has no such pairs and has not moved: it answers creation's
 * sah_cost.  Synchronous; refused with P3D_ERR_STATE while the stream is being captured.  P3D_ERR_ARG: NULL scene or sah_cost. */
int p3d_scene_tree_cost(p3d_scene* scene, float* sah_cost);

/* What p3d_scene_build_grid did, and the grid the handle holds after it. */
typedef struct p3d_grid_info {
    uint32_t built;            /* 1 = this call built the grid; 0 = the handle already had one (nothing done) */
    int32_t  n[3];             /* cells per axis, Grid::Build's nx ny nz */
    float    mn[3], mx[3];     /* the grid's box (scene bounds -/+ EPSILON) */
    uint64_t n_cells, n_items; /* cells, and primitive references over all cells */
} p3d_grid_info;
/* GRID mode's half of "move on the device, never go back to the host": the reference's uniform grid (Grid::Build,
 * RT/grid.cpp:30-98) is built on the device from what the handle holds there.  Opt-in: without this call the grid is built
 * lazily on the host by the first GRID call, with the refusals described under p3d_scene_update.  info may be NULL.
 *  - resulting state: the handle has the grid the host build would make of the current geometry -- the same cells per axis,
 *    the same box, and the same two arrays in every word (the grid's shape is observable: hits are accepted per cell,
 *    RT/grid.cpp:265-309), its items references in the handle's current numbering, in scene order inside every cell.  GRID-mode
 *    p3d_render, p3d_render_frames, p3d_render_aov, p3d_trace_rays and p3d_occluded then run, also while primitives updated
 *    from device memory are still unknown to the host.  A handle that already has a grid (built lazily, or by an earlier
 *    call) is left alone: P3D_OK, built == 0, info describes the grid it has.
 *  - the host's knowledge is NOT refreshed: the next p3d_scene_update or p3d_scene_rebuild drops the grid as it always does,
 *    and the lazy path refuses again as before; calling p3d_scene_build_grid again is the remedy.
 *  - where the boxes come from: the reference's per-primitive grid boxes (RT/scene.cpp:26-39, 180-196) cannot be recovered from
 *    the device records (a triangle is kept as p0, e1, e2, and p0 + (p1 - p0) is not p1 in float), so the handle keeps them in
 *    an array of its own, 24 bytes per primitive, in scene order: made of the creation-time description at the first update
 *    from device memory or the first call of this entry, whichever comes first, and kept current by every update after that.
 *  - ordering: synchronous.  Runs after everything already enqueued on the scene's stream and waits for it, then for the
 *    bounds of all boxes, for the item total and for the finished arrays.
 *  - stream capture: refused with P3D_ERR_STATE while the stream is being captured.  A GRID frame issued AFTER the call can be
 *    captured: it finds the grid built.
 *  - P3D_ERR_ARG: NULL scene.  P3D_ERR_STATE: a handle created with cull_never_hit, as for GRID frames.  P3D_ERR_LIMIT, before
 *    either grid array is allocated: the reference's formula asks for more than 2^31 - 1 cells (the host build's rule), or the
 *    references over all cells do not fit 32 bits.  P3D_ERR_HIP when device memory runs out: the handle keeps the grid state
 *    it had (no grid); the box array, if this call made it, stays and is counted.
 *  - what is kept: everything else -- the measured schedule choice, the learned tile orders, p3d_last_schedule(), the
 *    ray-stream state, the refit state and the tree.
 *  - memory: p3d_scene_stats::device_bytes grows by the two grid arrays (4 bytes per cell plus 4, 4 bytes per reference) and,
 *    once, by the box array (24 bytes per primitive); an update or rebuild gives the grid arrays back, so update / build
 *    rounds settle.  Sort and scan temporaries and the (cell, primitive) pairs are freed before the call returns and are not
 *    counted. */
int p3d_scene_build_grid(p3d_scene* scene, p3d_grid_info* info);

/* Rows of the compact per-rank tile buffer: ceil(n_row_blocks / world) * row_block, the
 * same on every rank so that the gather moves equal-sized buffers (rows past the image are
 * never written). */
int p3d_local_rows(int32_t res_y, int32_t row_block, int32_t world);

/* Replaces renderScene() (RT/main.cpp:732-832) incl. Camera::PrimaryRay, rayTracing(),
 * processLight() and every intercepts() beneath them. */
int p3d_render(p3d_scene* scene, const p3d_camera* cam, const p3d_render_params* params,
               const p3d_outputs* out);
/* Renders n frames of one configuration, frame f seen through cams[f], in the same launches.  Frame f equals what
 * p3d_render(scene, &cams[f], params', out_f) would produce, in every bit, where params' = *params except
 * seed = params->seed + f and samples = frame f's sample array.
 *  - cams: a HOST array of n >= 1 cameras sharing res_x and res_y (else P3D_ERR_ARG); eye, basis, w / h, plane_dist,
 *    aperture and focal_ratio may differ per frame.
 *  - outputs: every plane holds the n frames back to back, frame f starting f * rows * res_x pixels in, where rows is
 *    what p3d_render uses: res_y when world == 1, p3d_local_rows() when world > 1.  Host or device memory as in
 *    p3d_render; NULL planes are allowed.  Sharded batches stitch with p3d_deinterleave_frames (tile_stride_bytes =
 *    rows * res_x * bpp).
 *  - samples (spp > 0): n sample arrays back to back, on the host or (P3D_FLAG_DEVICE_SAMPLES) on the device.
 *  - random streams: frame f is keyed with seed + f.
 *  - every feature, flag, accel mode, rank / world and row_block of p3d_render is accepted.  Counters are the sum over
 *    the batch; the profile brackets the whole batch.  Batches keep their own measured schedule choice and tile order
 *    (keyed on n), so alternating with p3d_render on one handle re-measures neither.
 *  - a batch whose stacked pixel count n * p3d_local_rows() * res_x does not fit 31 bits is refused with P3D_ERR_LIMIT
 *    before anything is allocated.
 *  - under a stream capture it behaves like p3d_render: the per-frame cameras are written by launches of the captured
 *    stream itself, so a replay renders the cameras it was captured with. */
int p3d_render_frames(p3d_scene* scene, const p3d_camera* cams, int32_t n, const p3d_render_params* params,
                      const p3d_outputs* out);

/* What a frame knows about its primary hits besides their colour: the planes a denoiser, a depth compositor, an edge-aware
 * upsampler, picking with a hit point or reprojection between cameras read. */
typedef struct p3d_aov_outputs {   /* every plane may be NULL; memory as p3d_outputs::memory of the same call */
    float* depth;    /* [rows][res_x]    the intersector's t of the primary hit; +inf on a miss           */
    float* normal;   /* [rows][res_x][3] getNormal(hit point).normalize() of that hit; 0,0,0 on a miss    */
    float* albedo;   /* [rows][res_x][3] diffuse rgb of the hit primitive's material; 0,0,0 on a miss     */
} p3d_aov_outputs;
/* p3d_render_frames(scene, cams, n, params, out) in every bit of rgb8, rgb32f and hit_id, with the AOV planes written by
 * the same launches, where the closest hit of the primary ray is still in registers (the reference has no such output: its
 * rayTracing() keeps t, the normal and the material to itself, RT/main.cpp:575-589).  n == 1 is one frame, as p3d_render.
 * With aov == NULL, or all three planes NULL, the call is p3d_render_frames exactly.
 *  - which hit: the one hit_id describes -- the primary ray's closest hit, of sample 0 when spp > 0.  depth and normal are
 *    the bits p3d_trace_rays returns as t and normal for that same primary ray.
 *  - depth: no image convention -- no clamp, no quantisation; in units of the primary ray's direction as PrimaryRay builds
 *    it (RT/camera.h:91-127), so the hit point is origin + depth * direction.
 *  - albedo: floats 0..2 of the hit's material record as p3d_scene_desc::materials gave them, not multiplied by Kd.
 *  - layout: that of rgb32f and hit_id -- bottom row first, rows = res_y, or p3d_local_rows() when world > 1; frame f of a
 *    batch starts f * rows * res_x pixels in; rows past the image (the padding of a shard's last row block) are not
 *    written into device-memory planes, and hold unspecified values in host-memory planes, which are copied back whole from
 *    the handle's staging buffers -- as for rgb8, rgb32f and hit_id.  Sharded planes stitch with
 *    p3d_deinterleave[_frames]: bytes_per_pixel 4 for depth, 12 for normal and albedo.
 *  - every schedule, accel mode, feature, flag, sample count, sharding and workspace budget (banded frames) that
 *    p3d_render_frames accepts is accepted, with the same refusals; a NULL out is P3D_ERR_ARG as there (the planes are in
 *    the memory out->memory names).  A frame with planes runs builds of the level-1, tile and tree kernels that hold the
 *    writes; a frame without runs the kernels it ran before this entry existed.  The multi-tile level-1 kernels
 *    (p3d_set_primary_tiles) have no such build: a frame with planes runs one tile per workgroup, and
 *    p3d_last_primary_tiles() says so.
 *  - host memory (out->memory == 0): the planes are staged in device buffers the handle owns and copied back before the
 *    call returns.
 *  - handle state: the planes are part of no cache key.  A call with them shares the measured schedule choice, the learned
 *    tile orders and the workspaces of the same configuration without them; alternating the two re-measures nothing.
 *    The choice is measured by the frames WITHOUT planes only: a call with planes uses the choice already made (the tile
 *    schedule while there is none), times no candidate and leaves the measurement where it was.
 *  - after p3d_scene_update the planes follow the moved geometry like everything else. */
int p3d_render_aov(p3d_scene* scene, const p3d_camera* cams, int32_t n, const p3d_render_params* params,
                   const p3d_outputs* out, const p3d_aov_outputs* aov);
/* Replaces the sample draws of renderScene() (set_rand_seed, RT/main.cpp:747; pixel jitter :781-782;
 * sampleUnitDisk() * aperture, :723-730, :790) for one frame: writes [res_y][res_x][spp*spp][4] floats,
 * every bit what generate_samples(seed, res_x, res_y, spp, aperture, out) of the host layer writes with
 * this machine's C library -- the serial srand() / rand() stream, produced in parallel on the device
 * (csrc/p3d_rand.h, csrc/sample_stream.hip): a new seed, a render-again loop or a frame batch no longer
 * pays a host thread and an upload per frame.
 *  - output: memory == 1: a device pointer on the scene's device; the array is exactly what
 *    P3D_FLAG_DEVICE_SAMPLES reads.  A batch for p3d_render_frames is n calls at out + f * per_frame
 *    floats (per_frame = res_x * res_y * spp * spp * 4) with the caller's seeds and apertures; the host
 *    layer uses seed + f and cams[f].aperture.  memory == 0: the array is staged in the handle's sample
 *    buffer (where p3d_render stages a host sample array) and copied back.
 *  - exactness: how many draws a frame consumes depends on the draws (rejection sampling), so the call
 *    provisions a pass from the expected consumption and reads back the count of completed samples;
 *    while that count is short it continues the stream where the pass stopped -- position, machine
 *    state and sample index carry over.  Every seed gives the whole array; no sample is approximated.
 *  - synchronous, like p3d_scene_update: it runs after everything already enqueued on the scene's
 *    stream and WAITS for its own passes (one wait in all but astronomically rare cases), so the array
 *    is complete on return, in either memory.
 *  - stream capture: refused with P3D_ERR_STATE while the stream is being captured.
 *  - P3D_ERR_ARG: NULL scene or out; res_x, res_y or spp < 1; memory outside 0 and 1.  P3D_ERR_LIMIT,
 *    before anything is allocated, when res_x * res_y * spp * spp does not fit 31 bits.
 *  - scratch: jump tables (34 KiB) and 8 bytes per 496 pairs of draws of a pass plus 16 per 63488 --
 *    2.5 MB for 4096 x 4096 at 2 x 2 -- never the draws themselves; owned by the handle, counted in
 *    p3d_scene_stats::device_bytes when allocated, kept for the next call.
 *  - handle state: nothing else changes -- the measured schedule choice, the learned tile orders,
 *    p3d_last_schedule() and the ray-stream state are what they were. */
int p3d_generate_samples(p3d_scene* scene, uint32_t seed, int32_t res_x, int32_t res_y, int32_t spp,
                         float aperture, float* out, int32_t memory /* 0 host, 1 device */);

/* A stream of rays the caller supplies, and what comes back for each.  Ray i is (origin[i], dir[i]); its results sit at
 * index i of every plane -- no image conventions: no clamp, no quantisation, no bottom-up rows, no "/ 16". */
typedef struct p3d_rays {
    uint32_t     n;         /* number of rays; 0 is allowed and does nothing             */
    const float* origin;    /* [n][3]                                                    */
    const float* dir;       /* [n][3], used as given: NOT normalised (as rayTracing())   */
    int32_t      memory;    /* 0 host, 1 device pointers on the scene's device           */
} p3d_rays;

typedef struct p3d_ray_outputs {  /* every plane may be NULL */
    float*   rgb32f;   /* [n][3] what rayTracing(ray, 1, 1.0) returns: UNCLAMPED            */
    int32_t* hit_id;   /* [n] scene index of the closest hit, -1 on a miss                  */
    float*   t;        /* [n] the intersector's t of that hit (units of |dir|); +inf on a miss */
    float*   normal;   /* [n][3] getNormal(hit point).normalize() of that hit; 0,0,0 on a miss */
    int32_t  memory;   /* as p3d_outputs::memory: 0 = copy back and return when done, 1 = enqueue only */
} p3d_ray_outputs;

/* Replaces a caller's own loop around rayTracing(ray, 1, 1.0) (RT/main.cpp:530-721, with processLight() and every
 * intercepts() beneath it): ray i is traced as rayTracing(Ray(origin[i], dir[i]), 1, 1.0) -- depth 1, outside ior 1.0 --
 * for cameras the reference does not have, picking, probes and visibility queries.
 *  - params: max_depth, accel, flags and features are read.  accel selects the shadow-ray semantics exactly as
 *    for frames; closest hits are "nearest, lowest scene index on ties" (SURVEY Q1), as for frames.
 *  - asynchronous on the scene's stream like p3d_render; with p3d_ray_outputs::memory == 0 it copies and waits (and with
 *    p3d_rays::memory == 0 it uploads the rays first).  Under a stream capture it behaves like p3d_render: the lazy grid
 *    build of the first GRID-mode call is refused while capturing.
 *  - flags: P3D_FLAG_NO_LDS_SCENE and P3D_FLAG_PRIVATE_WALK are honoured; P3D_FLAG_WAVEFRONT is accepted and does nothing
 *    (ray streams run the wavefront schedule only).  Every other flag -- tile and tree forcing, counters, profile, packet
 *    walk, device samples -- is refused with P3D_ERR_ARG.
 *  - features: 0 and P3D_FEATURE_SOFT_SHADOW.  A stream has no sample index, so soft shadows are always the deterministic
 *    4x4 sub-light grid of RT/main.cpp:601-618.  Schlick, fuzzy reflection and the skybox are refused with P3D_ERR_ARG.
 *  - P3D_ERR_ARG also for: spp != 0, samples != NULL, world > 1 or rank != 0, a NULL origin or dir with n > 0, max_depth
 *    outside 1..16.
 *  - a scene created with cull_never_hit is refused with P3D_ERR_STATE: that shortcut rests on |dir| <= sqrt(2), which a
 *    caller's ray does not promise.
 *  - a ray with a NaN or an infinity in its origin or direction, or whose largest direction component lies outside
 *    [2^-60, 2^60], is tested against every primitive, as the reference's loop over the scene does (accel NONE and BVH;
 *    in GRID mode the reference converts such a ray's cell coordinate to int, which is undefined, and so are the results).
 *  - the staging of host-memory rays and planes is owned by the handle, counted in p3d_scene_stats::device_bytes as it
 *    grows and kept for the next call.
 *  - the workspace obeys the p3d_set_tuning() budget: streams that need more run in bands of rays, the way frames run in
 *    bands of rows.  A stream of 2^31 rays or more is refused with P3D_ERR_LIMIT before anything is allocated.
 *  - the handle's frame state is not touched: the measured schedule choice, the learned tile orders, p3d_last_schedule()
 *    and p3d_last_primary_tiles() are what they were, and a frame rendered after a stream is, in bits and in schedule,
 *    the frame it would have been without it. */
int p3d_trace_rays(p3d_scene* scene, const p3d_rays* rays, const p3d_render_params* params,
                   const p3d_ray_outputs* out);
/* Where the answers of p3d_occluded go. */
typedef struct p3d_occlusion_outputs {
    uint8_t* occluded;   /* [n] 1 = the shadow query answers "in shadow", 0 = not; may be NULL (the call then only validates) */
    int32_t  memory;     /* as p3d_ray_outputs::memory: 0 = copy back and return when done, 1 = enqueue only */
} p3d_occlusion_outputs;

/* Replaces the shadow query of processLight() (RT/main.cpp:476-510) -- the other traversal of both accelerators,
 * BVH::Traverse(Ray&) (RT/bvh.cpp:348) and Grid::Traverse(Ray&) (RT/grid.cpp:313) -- for segments the caller supplies: line
 * of sight, light baking, ambient occlusion, portal and audio probes.  Segment i is Ray(origin[i], dir[i]) of `segments`,
 * the "Ray(precise_hit_point, L)" processLight() builds: it ends at origin + dir.  occluded[i] is what the switch on
 * Accel_Struct would set insideShadow to for that ray:
 *    P3D_ACCEL_NONE  true if any primitive's intercepts() accepts the ray: the direction is used as given and there is NO
 *                    distance bound -- a primitive beyond the segment's end occludes it
 *    P3D_ACCEL_BVH   length = |dir|, the direction is normalised, true if a primitive is hit with t < length.  (The
 *                    reference's own tree answers false for a segment that starts exactly ON a primitive's bounding box and
 *                    does not enter it -- its box test rejects the node although intercepts() accepts the primitive at
 *                    t = 0.  The answer here is the primitive's: true.  tests/test_gpu_edge_rays.py keeps such segments.)
 *    P3D_ACCEL_GRID  the same bound over the reference's own grid, with its rule that a ray for which Init_Traverse fails
 *                    -- one that misses the grid's box -- is IN SHADOW (RT/grid.cpp:327-328).  The grid is built by the
 *                    first GRID call of a scene, this entry's included, under the rules of the first GRID frame: refused
 *                    with P3D_ERR_STATE while the stream is being captured and after updates from device memory (update
 *                    those primitives from host memory, or call p3d_scene_build_grid first: a handle that has a built
 *                    grid is served).
 *   There is no L.N > 0 test: that test decides whether processLight() asks at all, and every segment here is asked.
 *   Planes: the reference's accelerators bound a plane as [-1, 1]^3, and so do the tree and the grid here.
 *   In BVH and GRID mode a plane occludes only where the walk reaches that box: a segment that crosses the plane away
 *   from it is reported NOT occluded, as the reference's shadow rays are.  NONE mode tests every plane as it is.
 *  - params: only accel and flags are read.  P3D_FLAG_NO_LDS_SCENE and P3D_FLAG_PRIVATE_WALK are honoured, P3D_FLAG_WAVEFRONT
 *    is accepted and does nothing; every other flag is P3D_ERR_ARG.  features != 0, spp != 0, samples != NULL, world > 1
 *    and rank != 0 are P3D_ERR_ARG.  max_depth is not read.
 *  - P3D_ERR_ARG also for a NULL scene, segments, params or out, a NULL origin or dir with n > 0, and a memory field
 *    outside 0 and 1.
 *  - n >= 2^31 is P3D_ERR_LIMIT before anything is allocated; n == 0 does nothing and returns P3D_OK.
 *  - a scene created with cull_never_hit is served in accel BVH, whose rays are unit length; NONE and GRID are
 *    P3D_ERR_STATE (on the option itself, whatever it culled).
 *  - asynchronous on the scene's stream; with p3d_occlusion_outputs::memory == 0 it copies back and waits, and with
 *    p3d_rays::memory == 0 it uploads the segments first, through staging the handle owns (shared with p3d_trace_rays;
 *    counted in p3d_scene_stats::device_bytes as either entry grows it, and kept for the next call).
 *  - one launch, no ray queues and no workspace: the p3d_set_tuning() budget does not apply.
 *  - non-finite inputs, a zero-length dir and a dir whose largest component lies outside [2^-60, 2^60] are tested against
 *    every primitive in NONE and BVH mode (the rules above, no tree in between); in GRID mode the reference converts such a
 *    segment's cell coordinate to int, which is undefined, and so are the results (the call still returns).
 *  - the handle's frame state is not touched: the measured schedule choice, the learned tile orders, p3d_last_schedule(),
 *    p3d_last_primary_tiles() and the ray-stream state are what they were.
 *  - after p3d_scene_update or p3d_scene_rebuild the answers follow the moved geometry, like everything else. */
int p3d_occluded(p3d_scene* scene, const p3d_rays* segments, const p3d_render_params* params,
                 const p3d_occlusion_outputs* out);

/* The consumer of p3d_render_aov's planes: an edge-stopping filter for frames that are noisy by design -- jittered soft
 * shadows, fuzzy reflections, the thin lens at low spp. */
typedef struct p3d_denoise_params {
    int32_t res_x, res_y, n_frames;          /* n_frames >= 1: planes hold the frames back to back, as p3d_render_aov writes them */
    int32_t iterations;                      /* 0..6 */
    float   sigma_depth, sigma_albedo, sigma_color;
    int32_t normal_power_log2;               /* 0..8 */
} p3d_denoise_params;
typedef struct p3d_denoise_inputs { const float *rgb32f, *depth, *normal, *albedo; int32_t memory; } p3d_denoise_inputs;
/* An a-trous edge-avoiding wavelet filter (Dammertz et al. 2010) over the colour of n_frames frames, guided by their depth,
 * normal and albedo planes.  The reference has no denoiser; the result is DEFINED here, in float32 IEEE-754 basic
 * operations in a fixed order (no fused multiply-add, correctly rounded division, no exp and no pow), and the device, the
 * host layer (p3dh_denoise) and tests/denoise_reference.py agree on it in every bit.
 *  - the filter: pass i (0 <= i < iterations) has step s = 2^i, reads the previous pass's colour (pass 0 the input) and the
 *    unchanged depth Z, normal N and albedo A.  With k1 = {0.375, 0.25, 0.0625}, inv_a = 1 / sigma_albedo and, when
 *    sigma_color > 0, inv_c = 1 / (sigma_color * 2^-i):
 *      a pixel is VALID when its Z is finite and > 0.  A centre p that is not (a miss: +inf; t == 0; NaN) is copied.
 *      Else inv_z = 1 / (sigma_depth * Z_p), lum(c) = (0.2126 c.r + 0.7152 c.g) + 0.0722 c.b, and the taps
 *      q = (x + dx s, y + dy s) run dy = -2..2 (outer), dx = -2..2 (inner); a tap outside the frame or not valid
 *      contributes nothing; for the others
 *        h  = k1[|dx|] * k1[|dy|]
 *        wz = tz * tz,  tz = max(0, 1 - |Z_q - Z_p| * inv_z)
 *        wn = max(0, (N_p.x N_q.x + N_p.y N_q.y) + N_p.z N_q.z), then wn = wn * wn, normal_power_log2 times
 *        wa = ta * ta,  ta = max(0, 1 - ((|A_q.r - A_p.r| + |A_q.g - A_p.g|) + |A_q.b - A_p.b|) * inv_a)
 *        wc = tc * tc,  tc = max(0, 1 - |lum(C_q) - lum(C_p)| * inv_c)      (sigma_color > 0 only)
 *        w  = ((h * wz) * wn) * wa, then w = w * wc;  sum += w * C_q per channel (a product, then a sum);  sw += w
 *      out_p = sw > 0 ? sum / sw per channel : in_p.  max(0, v) is v > 0 ? v : 0.
 *    rgb32f receives the last pass's colour (the input when iterations == 0) and rgb8 its u8fromfloat(clamp01()), the
 *    quantisation of a frame (RT/maths.h:113-117).  NaN colours give unspecified results.  Frames of a batch are filtered
 *    independently: no tap crosses from one into the next.
 *  - planes: res_y rows of res_x pixels, bottom row first, frame f starting f * res_x * res_y pixels in -- what
 *    p3d_render_aov writes with world == 1.  Every input plane is needed.  out->rgb32f and out->rgb8 may each be NULL;
 *    out->hit_id must be NULL.  in->memory and out->memory are 0 (host) or 1 (device), independently; host planes are
 *    staged in buffers the handle owns and copied back before the call returns, as in p3d_trace_rays.
 *  - ordering: with all planes in device memory the call only enqueues on the scene's stream: one launch per pass, all
 *    frames in it (iterations == 0: one copy-and-quantise launch).  With a plane in host memory on EITHER side the call
 *    waits for the stream before it returns -- host inputs with device outputs too, so the caller's host planes have
 *    been read (pinned ones included) when it returns, as in p3d_accumulate and p3d_ambient_occlusion.
 *  - aliasing: out->rgb32f == in->rgb32f in device memory is allowed for every iterations.  No pass writes a buffer it
 *    reads: the colour alternates between two scratch buffers of the handle and the last pass writes the destination (a
 *    single in-place pass reads a copy).  Partial overlap is unspecified.
 *  - handle-owned memory: the scratch (12 bytes per pixel each, as many as the pass count needs) and the staging of
 *    host planes are counted in p3d_scene_stats::device_bytes as they grow, kept for the next call and freed with the handle.
 *  - stream capture: a call that has to allocate while the stream is being captured is refused with P3D_ERR_STATE, and
 *    so is one with a plane in host memory (it would have to wait); the capture survives.  After a call of the same
 *    shape made before the capture, the captured call is accepted and the graph replays.
 *  - P3D_ERR_ARG: a NULL scene, params or in; any NULL input plane; a NULL out; a non-NULL out->hit_id; res_x, res_y or
 *    n_frames below 1; iterations outside 0..6; normal_power_log2 outside 0..8; sigma_depth or sigma_albedo not finite or
 *    not positive; sigma_color not finite or negative (0 switches the colour stop off); a memory field outside 0 and 1.
 *    P3D_ERR_LIMIT, before anything is allocated, when n_frames * res_x * res_y does not fit 31 bits.
 *  - shards: the compact shards of world > 1 are not frames -- their rows are not neighbours in the image.  Stitch them with
 *    p3d_deinterleave[_frames] first and denoise the result.
 *  - handle state: nothing of the handle's frame state changes -- the measured schedule choice, the learned tile orders,
 *    p3d_last_schedule(), p3d_last_primary_tiles() and the ray-stream state are what they were. */
int p3d_denoise(p3d_scene* scene, const p3d_denoise_params* params, const p3d_denoise_inputs* in, const p3d_outputs* out);

/* p3d_denoise steered by a variance plane (SVGF, Schied et al. 2017): the colour stop of a pixel is as wide as the standard
 * deviation of its luminance says it is still noisy, and closes where the pixel has converged.  The variance is any
 * non-negative estimate of the luminance's variance per pixel -- over the frames a pixel has accumulated, or over its
 * neighbours. */
typedef struct p3d_denoise_variance_inputs { const float *rgb32f, *depth, *normal, *albedo, *variance; int32_t memory; } p3d_denoise_variance_inputs;
typedef struct p3d_denoise_variance_outputs { uint8_t* rgb8; float* rgb32f; float* variance; int32_t memory; } p3d_denoise_variance_outputs;
/* The result is DEFINED, as p3d_denoise's is: float32 IEEE-754 basic operations in a fixed order (no fused multiply-add,
 * correctly rounded division and square root, no exp and no pow); the device, the host layer (p3dh_denoise_variance) and
 * tests/denoise_variance_reference.py agree on it in every bit.
 *  - params: p3d_denoise's, with one difference: sigma_color must be finite and > 0.  It is the width of the colour stop in
 *    standard deviations of the luminance, not an absolute luminance, and it is NOT halved per pass.
 *  - planes: p3d_denoise's, and the variance V: [n_frames][res_y][res_x] floats, one per pixel.  in->variance is needed;
 *    out->rgb8, out->rgb32f and out->variance may each be NULL.
 *  - the filter: pass i (0 <= i < iterations) has step s = 2^i and reads the colour C and the variance V of the previous
 *    pass (pass 0 the inputs).  Everything of p3d_denoise's definition holds -- validity, k1, inv_a, inv_z, lum, the 25 taps
 *    dy outer and dx inner, h, wz, wn, wa -- with these changes for a VALID centre p:
 *      the prefiltered variance: the taps (x + dx, y + dy), dy = -1..1 (outer), dx = -1..1 (inner), at stride 1 whatever
 *        s, with k = k2[|dx|] * k2[|dy|], k2 = {0.5, 0.25}; a tap outside the frame or not valid contributes nothing; for
 *        the others sg += k * V_q (a product, then a sum), sk += k.  g = sg / sk, then g = g > 0 ? g : 0.
 *      inv_c = 1 / (sigma_color * sqrt(g) + 0x1p-20f): a product, a sum, a division.  It is always finite, and a pixel with
 *        no variance stops at a luminance difference of 2^-20.
 *      wc = tc * tc,  tc = max(0, 1 - |lum(C_q) - lum(C_p)| * inv_c), always
 *      w  = ((h * wz) * wn) * wa, then w = w * wc;  sum += w * C_q per channel;  sw += w;  sv += (w * w) * V_q, in this
 *        order.
 *      out_p = sw > 0 ? sum / sw per channel : C_p;  V_out = sw > 0 ? sv / (sw * sw) : V_p.
 *    A centre that is not valid keeps its colour and its variance.  rgb32f receives the last pass's colour, rgb8 its
 *    quantisation and variance the last pass's variance; iterations == 0 copies and quantises the colour and copies the
 *    variance.  NaN or negative variances (and NaN colours) give unspecified results for the pixels that read them.
 *  - aliasing: out->rgb32f == in->rgb32f and out->variance == in->variance in device memory are allowed, each or both,
 *    for every iterations (no pass writes a buffer it reads, as in p3d_denoise).  P3D_ERR_ARG when an output plane is any
 *    other input plane, or two output planes are one plane.
 *  - handle-owned memory: p3d_denoise's scratch buffers grow to carry the variance beside the colour (16 bytes per pixel
 *    each, as many as p3d_denoise's pass count needs); they and the staging of host planes (p3d_denoise's, and the two
 *    variance planes) are counted in p3d_scene_stats::device_bytes as they grow, kept for the next call and freed with
 *    the handle.
 *  - memory, ordering (the wait with a host plane on either side included), stream capture, the 31-bit limit, shards and
 *    "no frame state touched": as p3d_denoise.
 *  - P3D_ERR_ARG: p3d_denoise's refusals; a NULL in->variance; sigma_color == 0; the aliases above. */
int p3d_denoise_variance(p3d_scene* scene, const p3d_denoise_params* params, const p3d_denoise_variance_inputs* in,
                         const p3d_denoise_variance_outputs* out);

/* The temporal half of that pipeline: frames of a SEQUENCE from a moving camera (p3d_render_frames, p3d_render --orbit,
 * the render-again loop after SetEye, RT/main.cpp:740) are blended with what the previous frame accumulated at the same
 * surface point, found by reprojecting the pixel's primary hit into the previous camera. */
typedef struct p3d_accumulate_params {
    int32_t res_x, res_y, n_frames;   /* n_frames >= 1: a SEQUENCE, planes back to back as p3d_render_aov writes them (world == 1) */
    float   depth_tolerance;          /* finite, > 0: relative */
    float   normal_min;               /* in [-1, 1] */
    float   max_history;              /* finite, >= 1: cap of the history length, i.e. floor of the blend weight 1 / length */
} p3d_accumulate_params;
typedef struct p3d_accumulate_frames {  /* the frames to accumulate */
    const float *rgb32f, *depth, *normal;   /* needed */
    const int32_t* hit_id;                  /* may be NULL */
    const p3d_camera* cams;                 /* HOST array of n_frames cameras, always; res_x / res_y must equal params' */
    int32_t memory;                         /* 0 host, 1 device: the planes */
} p3d_accumulate_frames;
typedef struct p3d_accumulate_history { /* what frame 0 looks back at; the whole struct may be NULL = frame 0 has no history */
    const float *rgb32f, *depth, *normal, *length;   /* one frame each; all needed */
    const int32_t* hit_id;                            /* may be NULL */
    const p3d_camera* cam;                            /* HOST, the camera those planes were seen through */
    int32_t memory;
} p3d_accumulate_history;
typedef struct p3d_accumulate_outputs { float* rgb32f; float* length; int32_t memory; } p3d_accumulate_outputs;  /* either may be NULL, not both */
/* Temporal reprojection of history over the AOV planes of a sequence.  The reference has nothing like it; the result is
 * DEFINED here, in float32 IEEE-754 basic operations in a fixed order (no fused multiply-add, correctly rounded division
 * and square root), and the device, the host layer (p3dh_accumulate) and tests/accumulate_reference.py agree on it in
 * every bit.
 *  - history across the sequence: frame 0 looks back at `history` (at nothing when it is NULL); frame f > 0 looks back at
 *    frame f-1: its OUTPUT colour and length, its INPUT depth, normal and hit_id, and cams[f-1].  A caller running frame by
 *    frame feeds the previous call's outputs (and the previous frame's depth, normal, hit_id and camera) back as `history`
 *    and gets the bits of the whole sequence in one call.  The handle keeps no history: the entry is a pure function of
 *    its arguments.
 *  - the definition, for pixel (x, y) of frame f with colour C, depth Z, normal N and hit id I; primed values belong to the
 *    frame it looks back at, seen through the camera eye', u', v', n', w', h', plane_dist'.  A depth is VALID when it is
 *    finite and > 0 (the denoiser's rule).  "No history" means out = C and length = 1.
 *      0. the frame has nothing to look back at, or Z is not valid: no history.
 *      1. d = the direction of Camera::PrimaryRay((x + 0.5, y + 0.5)) of cams[f] (RT/camera.h:91-108) -- the bits of the
 *         spp == 0 frame kernels: fx = ((float)x + 0.5) / (float)res_x - 0.5, fy likewise,
 *         D = ((u * w) * fx + (v * h) * fy) + n * -plane_dist per component, l = 1 / sqrt((D.x^2 + D.y^2) + D.z^2),
 *         d = D * l.  P = eye + d * Z, per component a product and then a sum.
 *      2. q = P - eye';  a = (q.x u'.x + q.y u'.y) + q.z u'.z, b the same with v', c = -((q.x n'.x + q.y n'.y) + q.z n'.z).
 *         !(c > 0): no history.  s = c / plane_dist', fx' = a / (w' * s), fy' = b / (h' * s),
 *         px = (fx' + 0.5) * (float)res_x - 0.5, py = (fy' + 0.5) * (float)res_y - 0.5.
 *         !(px > -1 && px < (float)res_x && py > -1 && py < (float)res_y): no history (this also catches NaN).
 *         x0 = floor(px), tx = px - x0, y0 = floor(py), ty = py - y0.
 *         dist = sqrt((q.x^2 + q.y^2) + q.z^2), lim = depth_tolerance * dist.
 *      3. the taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), in this order, with the weights (1-tx)*(1-ty),
 *         tx*(1-ty), (1-tx)*ty, tx*ty.  A tap contributes when it is inside the frame, Z' is valid, |Z' - dist| <= lim,
 *         (N.x N'.x + N.y N'.y) + N.z N'.z >= normal_min and, when both hit_id planes exist, I' == I.  For each of them,
 *         with weight wgt and history length L':  sum += wgt * C' per channel, sl += wgt * L', sw += wgt.
 *      4. !(sw > 0): no history.  Else H = sum / sw, hl = sl / sw, len = hl + 1, len = max_history if len > max_history,
 *         alpha = 1 / len, out = H + (C - H) * alpha per channel, length = len.
 *    NaN colours give unspecified results.
 *  - depth counts from the ray's origin.  For one-sample pinhole frames (spp == 0) the planes are exact geometry along
 *    exactly the ray of step 1.  For spp > 0 the planes describe sample 0's jittered lens ray; the pinhole ray through the
 *    pixel centre then approximates it within a pixel (and within the aperture).  The definition does not change.
 *  - planes: res_y rows of res_x pixels, bottom row first, frame f starting f * res_x * res_y pixels in: rgb32f and normal
 *    3 floats per pixel, depth and length 1 float, hit_id 1 int32.  `length` is the history length: 1 where no history was
 *    taken, else up to max_history.  The compact shards of world > 1 are not frames: stitch them first
 *    (p3d_deinterleave[_frames]).
 *  - memory: frames->memory, history->memory and out->memory are 0 (host) or 1 (device), independently.  Host planes are
 *    staged in buffers the handle owns (counted in p3d_scene_stats::device_bytes as they grow, kept for the next call,
 *    freed with the handle); the call copies back and waits.  With everything in device memory the call only enqueues on
 *    the scene's stream: one launch per frame, in stream order; both cameras travel in the launch arguments by value, so
 *    a captured graph replays the cameras it was captured with.  An output plane that is NULL while n_frames > 1 is kept
 *    in two frame-sized buffers of the handle, since the next frame reads it.
 *  - aliasing: out->rgb32f == frames->rgb32f is allowed (a pixel reads only its own current colour before it writes).
 *    An output plane equal to any plane of `history`, to frames->depth, frames->normal or frames->hit_id, to the other
 *    output plane, or out->length == frames->rgb32f: P3D_ERR_ARG.  Partial overlap is unspecified.
 *  - stream capture: a call that has to allocate while the stream is being captured, or that has a plane in host memory,
 *    is refused with P3D_ERR_STATE; the capture survives.  After a call of the same shape made before the capture, the
 *    captured call is accepted and the graph replays.
 *  - P3D_ERR_ARG: a NULL scene, params, frames or out; a NULL frames->rgb32f, depth, normal or cams; a non-NULL history
 *    with a NULL rgb32f, depth, normal, length or cam; both output planes NULL; res_x, res_y or n_frames below 1; a camera
 *    whose res_x / res_y differ from params'; depth_tolerance not finite or not positive; normal_min outside [-1, 1] (or
 *    NaN); max_history not finite or below 1; a memory field outside 0 and 1; the aliases above.  P3D_ERR_LIMIT, before
 *    anything is allocated, when n_frames * res_x * res_y does not fit 31 bits.
 *  - handle state: nothing of the handle's frame state changes -- the measured schedule choice, the learned tile orders,
 *    p3d_last_schedule(), p3d_last_primary_tiles() and the ray-stream state are what they were.
 *  - after p3d_scene_update THIS entry still sees a static world: the hit_id, depth and normal tests drop what moved, or,
 *    under a small motion, pass on the wrong surface point.  p3d_accumulate_moving (below) is the entry for sequences whose
 *    primitives move: it reprojects through the primitive records of the two frames. */
int p3d_accumulate(p3d_scene* scene, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                   const p3d_accumulate_history* history, const p3d_accumulate_outputs* out);

/* The same accumulation for a sequence whose primitives move between frames (p3d_scene_update): the geometry every frame
 * was rendered with, in the form p3d_scene_update was given it. */
typedef struct p3d_accumulate_motion {
    uint32_t        n_prims;             /* >= 1 */
    const uint32_t* prim_type;           /* [n_prims] P3D_SPHERE.. as in p3d_scene_desc */
    const float*    prim_data;           /* [n_frames][n_prims][12]: the geometry frame f was rendered with,
                                            in p3d_scene_desc::prim_data form (what p3d_scene_update was given) */
    const float*    history_prim_data;   /* [n_prims][12]: the geometry the history was rendered with; needed iff history != NULL */
    int32_t         memory;              /* 0 host, 1 device: all three arrays */
} p3d_accumulate_motion;
typedef struct p3d_accumulate_moving_outputs { float* rgb32f; float* length; float* prev_xy; int32_t memory; } p3d_accumulate_moving_outputs;  /* not all NULL */
/* p3d_accumulate with the hit point moved back onto where the same surface point of the same primitive was in the frame
 * looked back at.  DEFINED here like p3d_accumulate: float32 IEEE-754 basic operations in the stated order, no fused
 * multiply-add, correctly rounded division and square root; the device, the host layer (p3dh_accumulate_moving) and
 * tests/accumulate_moving_reference.py agree on it in every bit.  Like p3d_accumulate it is a pure function of its
 * arguments: the handle keeps no previous geometry and no history, it lends its stream and its staging buffers.
 *  - the definition: steps 0, 1, 3 and 4 are p3d_accumulate's.  Step 2 starts from q = P_prev - eye' instead of
 *    q = P - eye'; everything after that line is unchanged, the depth test of step 3 included -- dist = |q| is then the
 *    PREVIOUS depth of the surface point, which is what Z' has to be compared with.
 *  - P_prev, for the pixel's hit id I (frames->hit_id is needed here: the motion is looked up by it; history->hit_id may
 *    still be NULL, which only switches the id test of step 3 off).  a = the record prim_data[f][I]; b = the record of the
 *    frame looked back at, prim_data[f-1][I], or history_prim_data[I] for frame 0; k = prim_type[I];
 *    dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z.
 *      static rule: if I < 0, or I >= n_prims, or the kind's meaningful floats of a and b are equal as 32-bit words (4 for a
 *         sphere, 9 for a triangle, 6 for a box, 4 for a plane and for any kind above 3 that reaches the device), then
 *         P_prev = P exactly.  With unchanged geometry the entry therefore returns the bits of p3d_accumulate, and ids
 *         outside the primitives read nothing.
 *      sphere   c, r -> c', r':  s = r' / r;  P_prev = c' + (P - c) * s per component, a product and then a sum.
 *      triangle P0 P1 P2 -> P0' P1' P2':  e1 = P1 - P0, e2 = P2 - P0, w = P - P0;  d11 = dot(e1, e1), d12 = dot(e1, e2),
 *         d22 = dot(e2, e2), w1 = dot(w, e1), w2 = dot(w, e2);  den = d11 * d22 - d12 * d12;
 *         beta = (d22 * w1 - d12 * w2) / den, gamma = (d11 * w2 - d12 * w1) / den;  e1' = P1' - P0', e2' = P2' - P0';
 *         P_prev = (P0' + e1' * beta) + e2' * gamma per component.
 *      box      mn, mx -> mn', mx', per axis:  e = mx - mn;  t = e != 0 ? (P - mn) / e : 0;  P_prev = mn' + (mx' - mn') * t.
 *      plane (and any kind above 3): a changed record has no point correspondence: no history.
 *    Degenerate records (r == 0, den == 0) give an infinite or NaN P_prev; the !(c > 0) and window tests of step 2 turn that
 *    into "no history", there is no test of its own.  The normal test of step 3 compares the CURRENT normal N with N': a
 *    primitive that turns by more than acos(normal_min) per frame loses its history.
 *  - out->prev_xy (optional): 2 floats per pixel, frames back to back: (px, py) of step 2 whenever the window test of step 2
 *    passed -- whether or not a tap then contributed -- and two quiet NaNs (0x7FC00000) otherwise: a frame with nothing to
 *    look back at, Z not valid, a changed plane, !(c > 0), a position outside the window.  It is the screen-space motion
 *    vector (previous position; subtract the pixel's own x, y) that temporal anti-aliasing and motion blur need.
 *  - planes, memory, the launches (one per frame in stream order, cameras by value), the spare planes, stream capture, the
 *    shards of world > 1 and the handle's untouched frame state: as p3d_accumulate.  motion->memory is independent of the
 *    other memory fields; host geometry is staged in buffers the handle owns (counted in device_bytes) like host planes,
 *    and like them refuses a captured stream.  Device arrays need only the alignment of their floats.
 *  - aliasing: out->rgb32f == frames->rgb32f is allowed.  Any other output plane equal to a plane of the frames or of the
 *    history, to an array of the motion or to another output plane -- prev_xy included --: P3D_ERR_ARG.
 *  - P3D_ERR_ARG: everything p3d_accumulate refuses (with "every output plane NULL" for its "both"); a NULL motion, prim_type
 *    or prim_data; n_prims == 0; a history with a NULL history_prim_data; a NULL frames->hit_id; motion->memory outside 0
 *    and 1; for host memory a prim_type above 3.  P3D_ERR_LIMIT, before anything is allocated, when
 *    n_frames * res_x * res_y or n_frames * n_prims * 12 does not fit 31 bits. */
int p3d_accumulate_moving(p3d_scene* scene, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                          const p3d_accumulate_history* history, const p3d_accumulate_motion* motion,
                          const p3d_accumulate_moving_outputs* out);

/* The temporal half of variance-guided denoising (SVGF, Schied et al. 2017): p3d_accumulate, or with a motion
 * p3d_accumulate_moving, that also carries the first two moments of every pixel's luminance over the frames it has
 * accumulated, and the variance they give -- the plane that steers p3d_denoise_variance. */
typedef struct p3d_accumulate_variance_params {
    float   min_temporal;        /* finite, >= 1: a pixel whose history is shorter takes the spatial estimate (1: none does) */
    int32_t radius;              /* 1..3: the spatial estimate looks at (2 radius + 1)^2 pixels */
    float   sigma_depth;         /* finite, > 0: p3d_denoise's depth stop, for the spatial estimate */
    int32_t normal_power_log2;   /* 0..8: p3d_denoise's normal stop, for the spatial estimate */
} p3d_accumulate_variance_params;
typedef struct p3d_accumulate_variance_outputs {   /* each may be NULL, not all */
    float* rgb32f; float* length;
    float* moments;              /* [n_frames][res_y][res_x][2] */
    float* variance;             /* [n_frames][res_y][res_x] */
    float* prev_xy;              /* with a motion only */
    int32_t memory;
} p3d_accumulate_variance_outputs;
/* DEFINED like its siblings: float32 IEEE-754 basic operations in the stated order, no fused multiply-add, correctly
 * rounded division and square root; the device, the host layer (p3dh_accumulate_variance) and
 * tests/accumulate_variance_reference.py agree on it in every bit.  A pure function of its arguments, as they are.
 *  - arguments: params, frames and history as p3d_accumulate reads them.  motion NULL: a static world, step 2 of
 *    p3d_accumulate; else step 2 of p3d_accumulate_moving, with everything that entry asks of motion and frames->hit_id.
 *    history_moments: one frame of [res_y][res_x][2] floats in history->memory, the `moments` output of the frame the
 *    history describes; needed exactly when history is given.
 *  - rgb32f, length and prev_xy are, in every bit, what p3d_accumulate (motion NULL) or p3d_accumulate_moving (motion
 *    given) returns for the same arguments.  prev_xy without a motion: P3D_ERR_ARG.
 *  - moments, for a pixel with current colour C: l = lum(C) = (0.2126 C.r + 0.7152 C.g) + 0.0722 C.b, m = (l, l * l).
 *    In step 3 every tap that contributes also adds, after sl and before sw, sm1 += wgt * M'.x and sm2 += wgt * M'.y, M' the
 *    moments of the frame looked back at (frame f-1's OUTPUT moments; history_moments for frame 0).  In step 4
 *    Hm = sm / sw per component and out_m = Hm + (m - Hm) * alpha with the colour's alpha.  "No history" in all its forms:
 *    out_m = m.
 *  - variance: vt = out_m.y - out_m.x * out_m.x, then vt = vt > 0 ? vt : 0.  A pixel whose Z is not valid gets 0.  A pixel
 *    whose Z is valid and whose output length is < min_temporal gets a spatial estimate from the frame's INPUT colour:
 *      inv_z = 1 / (sigma_depth * Z_p); the taps q = (x + dx, y + dy) run dy = -radius..radius (outer), dx likewise
 *      (inner); a tap outside the frame or with a Z that is not valid contributes nothing; for the others
 *        wz = tz * tz,  tz = max(0, 1 - |Z_q - Z_p| * inv_z)
 *        wn = max(0, (N_p.x N_q.x + N_p.y N_q.y) + N_p.z N_q.z), then wn = wn * wn, normal_power_log2 times
 *        w = wz * wn,  lq = lum(C_q);  s1 += w * lq;  s2 += w * (lq * lq);  sw += w        (products, then sums)
 *      sw > 0: a = s1 / sw, b = s2 / sw, variance = max(0, b - a * a).  Else variance = vt.
 *    Every other pixel gets vt.  Lengths are >= 1, so min_temporal == 1 switches the estimate off.  The estimate is not
 *    fed back: the next frame looks back at the moments only.
 *  - an output plane the caller does not want but a later launch reads -- colour, length or moments while n_frames > 1, the
 *    length the spatial estimate reads -- is kept in spare planes of the handle (counted in device_bytes as they grow).
 *  - launches: per frame p3d_accumulate[_moving]'s launch with the moments in it, and behind it, when min_temporal > 1
 *    and out->variance is wanted, the launch of the spatial estimate; cameras by value, in stream order.
 *  - aliasing: out->rgb32f == frames->rgb32f is allowed (with a spatial estimate the colour is then blended into a spare
 *    plane of the handle and copied over the frame once the estimate has read it).  P3D_ERR_ARG for everything the
 *    siblings refuse, and for out->moments or out->variance equal to any plane of the frames or of the history,
 *    history_moments, an array of the motion or another output plane, and for any output plane equal to history_moments.
 *  - planes, memory (history_moments lies where history->memory says), stream capture, the 31-bit limit, the shards of
 *    world > 1 and the handle's untouched frame state: as p3d_accumulate.
 *  - P3D_ERR_ARG besides: a NULL variance_params; history without history_moments or the reverse; min_temporal not finite
 *    or below 1; radius outside 1..3; sigma_depth not finite or not positive; normal_power_log2 outside 0..8; every output
 *    plane NULL. */
int p3d_accumulate_variance(p3d_scene* scene, const p3d_accumulate_params* params, const p3d_accumulate_variance_params* variance_params,
                            const p3d_accumulate_frames* frames, const p3d_accumulate_history* history, const float* history_moments,
                            const p3d_accumulate_motion* motion, const p3d_accumulate_variance_outputs* out);

/* Ambient occlusion over the planes of p3d_render_aov: hemisphere any-hit queries fused per pixel.  What a caller of
 * p3d_occluded would build as res_x * res_y * samples segments, upload and count is made in the lanes of one launch from
 * the depth and normal planes; the segments never exist in memory. */
typedef struct p3d_ao_params {
    int32_t  samples;    /* 1, 2, 4, 8, 16, 32 or 64 segments per pixel */
    float    radius;     /* finite, > 0: the segments' length */
    float    bias;       /* finite, >= 0: the origin is moved this far along the normal that faces the eye */
    uint32_t seed;       /* frame f keys its random streams with seed + f */
} p3d_ao_params;
typedef struct p3d_ao_inputs {
    const float *depth, *normal;   /* needed */
    const float* rgb32f;           /* may be NULL */
    int32_t memory;                /* 0 host, 1 device */
} p3d_ao_inputs;
typedef struct p3d_ao_outputs { float* ao; float* rgb32f; int32_t memory; } p3d_ao_outputs;   /* either may be NULL, not both */
/* The reference has no ambient occlusion; the result is DEFINED here, in float32 IEEE-754 basic operations in a fixed
 * order (no fused multiply-add, correctly rounded division and square root), and the device, the host layer
 * (p3dh_ao_segments, p3dh_ao_resolve) and tests/ao_reference.py agree on it in every bit.  One part is anchored to what the
 * reference pins: whether a sample counts as occluded is what p3d_occluded answers for its segment.
 *  - planes: res_y rows of res_x pixels, bottom row first, n frames back to back, as p3d_render_aov writes them with
 *    world == 1: depth and ao 1 float per pixel, normal and rgb32f 3.  Frame f is seen through cams[f] (HOST array of n
 *    cameras); all cameras share res_x / res_y.
 *  - the definition, for pixel (x, y) of frame f with depth Z and normal N.  normalized(a) is the project's:
 *    l = 1 / sqrt((a.x^2 + a.y^2) + a.z^2), a * l per component.  rng_mix(a, b) is, in uint32 arithmetic,
 *    h = (a ^ 0x9E3779B9) * 0x85EBCA6B + b; h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16; and
 *    rng_u01(key, k) = (float)(rng_mix(key, k) >> 8) * 2^-24 (the random streams of the frames' stochastic features).
 *      1. validity: Z is VALID when it is finite and > 0 (the denoiser's rule).  Otherwise the pixel has no query and ao = 1.
 *      2. hit point: d = the direction of Camera::PrimaryRay((x + 0.5, y + 0.5)) of cams[f], exactly as step 1 of
 *         p3d_accumulate forms it; P = eye + d * Z, per component a product and then a sum.
 *      3. face-forward: Ns = -N if (N.x d.x + N.y d.y) + N.z d.z > 0, else N.  The origin is O = P + Ns * bias, per
 *         component a product and then a sum.
 *      4. keys: pk = rng_mix(seed + f, y * res_x + x); sample s = 0 .. samples - 1 has the key k = rng_mix(pk, s).  The
 *         keys do not depend on `samples`: sample s is the same segment at every sample count.
 *      5. a uniform point on the sphere by rejection: tries j = 0 .. 31 draw c_i = 2 * rng_u01(k, 3 j + i) - 1 for
 *         i = 0, 1, 2; q = (c_0^2 + c_1^2) + c_2^2.  The first try with q <= 1 && q >= 2^-20 is accepted and
 *         v = normalized(c).  If none of the 32 tries is accepted, v = Ns (the rule bounds the loop).
 *      6. cosine-weighted direction: w = Ns + v; if !((w.x^2 + w.y^2) + w.z^2 >= 2^-20) then w = Ns.
 *         L = normalized(w) * radius.
 *      7. the query: sample s is occluded iff p3d_occluded answers 1 for the segment (O, L) under params->accel -- NONE
 *         mode's "no distance bound", GRID's "misses the grid's box = in shadow" and the accelerators' plane rule included.
 *      8. with occ the number of occluded samples, ao = (float)(samples - occ) / (float)samples.  out->rgb32f is ao * c per
 *         channel of in->rgb32f when that is given, else (ao, ao, ao) -- a plane p3d_denoise takes as its colour.
 *    A normal that is not unit length, zero or not finite goes through the same operations; step 7's answer for a segment
 *    that is not finite is p3d_occluded's.
 *  - params: only accel and flags are read, with p3d_occluded's rules: P3D_FLAG_NO_LDS_SCENE and P3D_FLAG_PRIVATE_WALK are
 *    honoured, P3D_FLAG_WAVEFRONT is accepted and does nothing; every other flag is P3D_ERR_ARG, and so are features != 0,
 *    spp != 0, samples != NULL, world > 1 and rank != 0.  The GRID-mode lazy build and the cull_never_hit refusals
 *    (P3D_ERR_STATE) are p3d_occluded's.
 *  - P3D_ERR_ARG also for a NULL scene, cams, params, ao, in or out; n < 1; cameras whose res_x / res_y are below 1 or
 *    differ; ao->samples not one of 1, 2, 4, 8, 16, 32, 64; radius or bias not finite, radius <= 0, bias < 0; a NULL depth or
 *    normal; both output planes NULL; an output plane that is an input plane or the other output plane; a memory field
 *    outside 0 and 1.  P3D_ERR_LIMIT, before anything is allocated, when n * res_y * res_x * samples does not fit 31 bits.
 *  - memory: in->memory and out->memory are 0 (host) or 1 (device), independently.  Host planes are staged in buffers the
 *    handle owns (counted in p3d_scene_stats::device_bytes as they grow, kept for the next call, freed with the handle);
 *    the call copies back and waits.  With everything in device memory the call only enqueues on the scene's stream: one
 *    small launch that writes the n cameras into a buffer of the handle (they travel in that launch's arguments, so a
 *    captured graph replays the cameras it was captured with) and ONE launch for all n frames.
 *  - stream capture: a call that has to allocate while the stream is being captured, or that has a plane in host memory,
 *    is refused with P3D_ERR_STATE; the capture survives.  After a call of the same shape made before the capture, the
 *    captured call is accepted and the graph replays.
 *  - handle state: nothing of the handle's frame state changes -- the measured schedule choice, the learned tile orders,
 *    p3d_last_schedule(), p3d_last_primary_tiles() and the ray-stream state are what they were.
 *  - after p3d_scene_update or p3d_scene_rebuild the queries follow the moved geometry; the planes are the caller's.
 *  - on every refusal the outputs are untouched. */
int p3d_ambient_occlusion(p3d_scene* scene, const p3d_camera* cams, int32_t n, const p3d_render_params* params,
                          const p3d_ao_params* ao, const p3d_ao_inputs* in, const p3d_ao_outputs* out);

/* One bounce of diffuse indirect light over the planes of p3d_render_aov (a final gather, "colour bleeding"): per pixel,
 * `samples` cosine-weighted rays from the primary hit, each returning the direct-lit colour of what it hits, and their
 * mean.  What a caller of p3d_trace_rays would build as res_x * res_y * samples rays, upload, trace at max_depth 1 and
 * reduce is made, traced and summed in the lanes of one launch; neither the rays nor their colours exist in memory. */
typedef struct p3d_indirect_params {
    int32_t  samples;    /* 1, 2, 4, 8, 16, 32 or 64 rays per pixel */
    float    bias;       /* finite, >= 0: the origin is moved this far along the normal that faces the eye */
    uint32_t seed;       /* frame f keys its random streams with seed + f */
} p3d_indirect_params;
typedef struct p3d_indirect_inputs {
    const float *depth, *normal;      /* needed */
    const float *albedo, *rgb32f;     /* may be NULL */
    int32_t memory;                   /* 0 host, 1 device */
} p3d_indirect_inputs;
typedef struct p3d_indirect_outputs { float* indirect; float* rgb32f; int32_t memory; } p3d_indirect_outputs;   /* either may be NULL, not both */
/* The reference has no indirect light (Whitted's recursion has no such term); the result is DEFINED here, in float32
 * IEEE-754 basic operations in a fixed order (no fused multiply-add), and the device, the host layer (p3dh_ao_segments,
 * p3dh_indirect_resolve) and tests/indirect_reference.py agree on it in every bit.  One part is anchored to what the
 * reference pins: a sample's radiance is what p3d_trace_rays returns for its ray.
 *  - planes: as p3d_ambient_occlusion's: depth 1 float per pixel; normal, albedo, rgb32f and indirect 3.  Frame f is seen
 *    through cams[f] (HOST array of n cameras); all cameras share res_x / res_y.
 *  - the definition, for pixel (x, y) of frame f with depth Z and normal N:
 *      1. - 6. steps 1 to 6 of p3d_ambient_occlusion with radius = 1: validity of Z (otherwise the pixel has no query), the
 *         hit point P through cams[f], the face-forward normal Ns, the origin O = P + Ns * bias, the keys
 *         pk = rng_mix(seed + f, y * res_x + x) and k = rng_mix(pk, s), the rejection draw, and D = normalized(w) --
 *         normalized(w) * 1.0f in every bit.  The ray of sample s is the segment p3dh_ao_segments makes at radius 1, and the
 *         same ray at every sample count.
 *      7. radiance: r_s is the rgb32f p3d_trace_rays returns for Ray(O, D) with max_depth = 1, features = 0 and
 *         params->accel: at a hit the clamped direct lighting of the hit point -- the reference's depth >= MAX_DEPTH return,
 *         processLight with its shadow queries under the mode's shadow semantics --, at a miss the scene's background.
 *      8. the sum is a balanced tree in sample order, per channel: t_0[s] = r_s, t_(j+1)[i] = t_j[2 i] + t_j[2 i + 1], and
 *         m = t_(log2 samples)[0] * (1.0f / samples).
 *      9. out->indirect = m.  out->rgb32f = c + a * m per channel, a product and then a sum, with a = in->albedo (1 when
 *         that is NULL) and c = in->rgb32f; without in->rgb32f the value is a * m alone.  A pixel without a query gets
 *         indirect = 0 and rgb32f = c (0 without in->rgb32f).
 *    A normal that is not unit length, zero or not finite goes through the same operations; step 7's answer for a ray that
 *    is not finite is p3d_trace_rays'.
 *  - params: only accel and flags are read, with p3d_trace_rays' rules: P3D_FLAG_NO_LDS_SCENE and P3D_FLAG_PRIVATE_WALK are
 *    honoured, P3D_FLAG_WAVEFRONT is accepted and does nothing; every other flag is P3D_ERR_ARG, and so are features != 0,
 *    spp != 0, samples != NULL, world > 1 and rank != 0.  max_depth is not read.  The GRID-mode lazy build and the
 *    refusal of a handle built with cull_never_hit (P3D_ERR_STATE, in every accel) are p3d_trace_rays'.
 *  - P3D_ERR_ARG also for a NULL scene, cams, params, indirect, in or out; n < 1; cameras whose res_x / res_y are below 1 or
 *    differ; indirect->samples not one of 1, 2, 4, 8, 16, 32, 64; bias not finite or < 0; a NULL depth or normal; both output
 *    planes NULL; an output plane that is an input plane or the other output plane; a memory field outside 0 and 1.
 *    P3D_ERR_LIMIT, before anything is allocated, when n * res_y * res_x * samples does not fit 31 bits.
 *  - memory, staging, stream capture, handle state, scene motion: as p3d_ambient_occlusion, with staging buffers of its
 *    own.  With everything in device memory the call is the small camera launch and ONE launch for all n frames: no ray
 *    queues, no workspace.
 *  - on every refusal the outputs are untouched. */
int p3d_indirect_diffuse(p3d_scene* scene, const p3d_camera* cams, int32_t n, const p3d_render_params* params,
                         const p3d_indirect_params* indirect, const p3d_indirect_inputs* in, const p3d_indirect_outputs* out);

/* Several bounces of diffuse indirect light over the same planes: per pixel `samples` paths of at most `bounces` rays, a path
 * per lane.  Ray 0 of a path is the ray p3d_indirect_diffuse traces for that sample; at every hit the path goes on in a
 * cosine-weighted direction, its throughput multiplied by the albedo of what it hit, and every ray adds the direct-lit
 * colour of what it hits times the throughput.  What a caller would build as `bounces` rounds of p3d_trace_rays with kernels
 * of their own in between -- 24 bytes of ray and 12 of colour per sample per round -- is a loop in the lanes of one launch. */
typedef struct p3d_path_params {
    int32_t  samples;   /* 1, 2, 4, 8, 16, 32 or 64 paths per pixel */
    int32_t  bounces;   /* 1 .. 8: rays per path at most */
    float    bias;      /* finite, >= 0: every vertex's origin is moved this far along the normal that faces the incoming ray */
    uint32_t seed;      /* frame f keys its random streams with seed + f */
} p3d_path_params;
/* The result is DEFINED here like p3d_indirect_diffuse's, in float32 IEEE-754 basic operations in the stated order (no fused
 * multiply-add), and the device, the host layer (p3dh_ao_segments, p3dh_path_next, p3dh_path_add, p3dh_indirect_resolve) and
 * tests/path_reference.py agree on it in every bit.  Every ray's answer is anchored to what p3d_trace_rays returns for it.
 *  - planes, cameras, inputs and outputs: p3d_indirect_diffuse's.
 *  - the definition, for pixel (x, y) of frame f and sample s = 0 .. samples - 1:
 *      1. vertex 0: steps 1 to 6 of p3d_indirect_diffuse give the pixel's validity (an invalid depth: no path), O_0, Ns_0,
 *         pk_0 = rng_mix(seed + f, y * res_x + x) and D_0: ray 0 of the path is the ray p3d_indirect_diffuse traces for
 *         sample s.
 *      2. trace: for b = 0 .. bounces - 1 while the path is alive, (r_b, hit_b, t_b, N_b) is what p3d_trace_rays answers as
 *         rgb32f, hit_id, t and normal for Ray(O_b, D_b) with max_depth = 1, features = 0 and params->accel: r_b is the
 *         clamped direct lighting of the hit with its shadow queries, or the background on a miss; N_b is
 *         getNormal(O_b + D_b * t_b).normalize().
 *      3. sum: R = r_0; for b >= 1, per channel, R = R + T_b * r_b, a product and then a sum.  A path that misses at
 *         bounce b (hit_b < 0) ends after adding that term.
 *      4. next vertex, when hit_b >= 0 and b + 1 < bounces:
 *           P = O_b + D_b * t_b, per component a product and then a sum;
 *           a = floats 0..2 of the hit's material record: the albedo p3d_render_aov defines, not multiplied by Kd;
 *           T_(b+1) = a for b = 0, else T_b * a per channel;
 *           Ns = -N_b if (N_b.x D_b.x + N_b.y D_b.y) + N_b.z D_b.z > 0, else N_b;
 *           O_(b+1) = P + Ns * bias, per component a product and then a sum;
 *           pk_(b+1) = rng_mix(pk_0, 0x80000000 + (b + 1));
 *           D_(b+1) = steps 5 and 6 of p3d_ambient_occlusion at radius 1 from Ns with the key rng_mix(pk_(b+1), s).
 *         The keys do not depend on `samples` or `bounces`: sample s is the same path at every sample count, and a path of
 *         fewer bounces is a prefix of a path of more.
 *      5. resolve: steps 8 and 9 of p3d_indirect_diffuse on the per-sample R: the balanced tree in sample order, times
 *         1.0f / samples, out->indirect = m and out->rgb32f = c + a * m.  A pixel without a path gets what it gets there.
 *    Normals that are not unit length, zero or not finite, and glass or mirror materials, go through the same operations.
 *    There is no Russian roulette and no specular path segment.  With bounces == 1 every output bit is
 *    p3d_indirect_diffuse's.
 *  - params, P3D_ERR_ARG, P3D_ERR_LIMIT (still on n * res_y * res_x * samples), P3D_ERR_STATE, memory, stream capture,
 *    handle state, scene motion and refusals: as p3d_indirect_diffuse, with `paths` in the place of `indirect`; in addition
 *    paths->bounces outside 1 .. 8 is P3D_ERR_ARG.  The staging buffers and the camera buffer are p3d_indirect_diffuse's:
 *    calls of the two entries on planes of one size share them.  With everything in device memory the call is the small
 *    camera launch and ONE launch for all n frames and all bounces. */
int p3d_indirect_paths(p3d_scene* scene, const p3d_camera* cams, int32_t n, const p3d_render_params* params,
                       const p3d_path_params* paths, const p3d_indirect_inputs* in, const p3d_indirect_outputs* out);

/* The edge-aware upsampler of p3d_render_aov's planes: a low-frequency signal (ambient occlusion, a soft shadow, a fuzzy
 * reflection) computed at 1 / factor of the resolution is brought up to the full frame along the full frame's depth and
 * normal (joint bilateral upsampling, Kopf et al. 2007). */
typedef struct p3d_upsample_params {
    int32_t res_x, res_y;        /* the LOW resolution, >= 1 each */
    int32_t factor;              /* s = 1, 2, 3 or 4: the output is res_x * s by res_y * s */
    int32_t n_frames;            /* >= 1, planes back to back as p3d_render_aov writes them */
    int32_t channels;            /* c = 1 (an ao plane) or 3 (a colour) floats per pixel of `low` and of the output */
    float   sigma_depth;         /* finite, > 0: the denoiser's relative depth stop */
    int32_t normal_power_log2;   /* 0..8: the denoiser's */
} p3d_upsample_params;
typedef struct p3d_upsample_inputs  { const float *low, *low_depth, *low_normal, *depth, *normal; int32_t memory; } p3d_upsample_inputs;
typedef struct p3d_upsample_outputs { float* plane; uint8_t* fallback; int32_t memory; } p3d_upsample_outputs;  /* either may be NULL, not both */
/* The reference has no upsampler; the result is DEFINED here, as p3d_denoise's is: float32 IEEE-754 basic operations in a
 * fixed order (no fused multiply-add, correctly rounded division, no exp and no pow), and the device, the host layer
 * (p3dh_upsample) and tests/upsample_reference.py agree on it in every bit.
 *  - planes: with s = factor, W = res_x * s and H = res_y * s, in->low is [n_frames][res_y][res_x][c], in->low_depth
 *    [n_frames][res_y][res_x] and in->low_normal [n_frames][res_y][res_x][3]: the signal and the planes it was computed on;
 *    in->depth [n_frames][H][W] and in->normal [n_frames][H][W][3]: the full frame's.  out->plane is [n_frames][H][W][c]
 *    and out->fallback [n_frames][H][W] bytes.  Rows bottom row first, frames back to back -- what p3d_render_aov writes
 *    with world == 1.  The low planes are those of a camera with the full frame's view window and res / s: pinhole_dir
 *    puts pixel i of a res_x-wide camera at (i + 0.5) / res_x of the window, so low pixel i has its centre at
 *    s * (i + 0.5) full-resolution pixels, and the full-resolution pixel x has its centre at x + 0.5.
 *  - the filter, per full-resolution pixel (x, y) of frame f, with its own depth Z_p and normal N_p:
 *      taps, per axis, in integers:  t = 2 x + 1 - s,  i0 = floor(t / (2 s))  (floor division: i0 = -1 occurs at the near
 *      border),  r = t - 2 s i0  (in [0, 2 s)),  fx = (float)r / (float)(2 s).  The two taps of the axis are i0 with weight
 *      bx0 = 1 - fx and i0 + 1 with weight bx1 = fx; y likewise (j0, by0, by1).  The four taps run dy = 0, 1 (outer),
 *      dx = 0, 1 (inner), q = (i0 + dx, j0 + dy), b = bx * by.  A tap outside the low frame contributes nothing to any sum.
 *      A depth is VALID when it is finite and > 0 (the denoiser's rule).
 *      A valid centre: inv_z = 1 / (sigma_depth * Z_p); only taps with a valid Z_q contribute, with
 *        wz = tz * tz,  tz = max(0, 1 - |Z_q - Z_p| * inv_z)
 *        wn = max(0, (N_p.x N_q.x + N_p.y N_q.y) + N_p.z N_q.z), then wn = wn * wn, normal_power_log2 times
 *        w  = (b * wz) * wn
 *      A centre that is not valid (a miss: +inf; 0; NaN): only taps that are themselves NOT valid contribute, with w = b --
 *      sky is made of sky.
 *      sum += w * C_q per channel (a product, then a sum);  sw += w.  max(0, v) is v > 0 ? v : 0.
 *      If sw > 0: out = sum / sw per channel and fallback = 0.  Otherwise no low sample explains the pixel (a thin feature,
 *      a silhouette): out is the plain bilinear value -- the same sums over every tap inside the low frame with w = b, in
 *      the same order, out = sum / sw -- and fallback = 1.  That sw is > 0: at least one tap inside the frame has b > 0.
 *      Per axis i0 lies in -1 .. res_x - 1; both taps are inside unless i0 = -1, where r >= s + 1 makes bx1 > 0 on tap 0, or
 *      i0 = res_x - 1, where r <= s - 1 makes bx0 >= 1 / 2 on tap res_x - 1; with both inside, bx0 or bx1 is >= 1 / 2.
 *    Non-finite values in `low` give unspecified results.  Frames of a batch are independent.
 *  - the fallback plane tells a caller which pixels to treat otherwise, for example to re-trace them with p3d_trace_rays.
 *  - memory: in->memory and out->memory are 0 (host) or 1 (device), independently.  Host planes are staged in buffers the
 *    handle owns (counted in p3d_scene_stats::device_bytes as they grow, kept for the next call, freed with the handle);
 *    the call copies back and waits -- with host inputs and device outputs too, so the caller's host planes have been read
 *    (pinned ones included) when it returns.  With everything in device memory the call only enqueues on the scene's
 *    stream: ONE launch for all n_frames frames.
 *  - stream capture: a call that has to allocate while the stream is being captured, or that has a plane in host memory,
 *    is refused with P3D_ERR_STATE; the capture survives.  After a call of the same shape made before the capture, the
 *    captured call is accepted and the graph replays.
 *  - P3D_ERR_ARG: a NULL scene, params, in or out; any NULL input plane; both output planes NULL; factor outside 1..4;
 *    channels not 1 or 3; res_x, res_y or n_frames below 1; sigma_depth not finite or not positive; normal_power_log2
 *    outside 0..8; a memory field outside 0 and 1; an output plane that is an input plane.  P3D_ERR_LIMIT, before anything
 *    is allocated, when n_frames * W * H * channels does not fit 31 bits.
 *  - shards: the compact shards of world > 1 are not frames; stitch them with p3d_deinterleave[_frames] first.
 *  - handle state: nothing of the handle's frame state changes -- the measured schedule choice, the learned tile orders,
 *    p3d_last_schedule(), p3d_last_primary_tiles() and the ray-stream state are what they were.
 *  - on every refusal the outputs are untouched. */
int p3d_upsample(p3d_scene* scene, const p3d_upsample_params* params, const p3d_upsample_inputs* in, const p3d_upsample_outputs* out);
int p3d_sync(p3d_scene* scene);
/* counters of the most recent render made with P3D_FLAG_COUNTERS (waits for it) */
int p3d_get_counters(p3d_scene* scene, p3d_counters* out);

/* Launch tuning that never changes results (0 keeps the current value): xcd_chunk =
 * consecutive 16x4-pixel tiles given to one XCD before moving to the next (1 = round robin,
 * best load balance; larger = more L2 locality per XCD for big scenes); workspace_mib = HBM
 * budget for the wavefront ray queues (default 65536, shared by the concurrent sample passes of a frame; frames that need more run in bands);
 * waves_per_simd = register budget of the ray kernels expressed as resident waves per SIMD:
 * 0 compiler default, 5 / 6 trade spilled registers for latency hiding, -1 keeps. */
int p3d_set_tuning(p3d_scene* scene, int32_t xcd_chunk, int32_t workspace_mib, int32_t waves_per_simd);

/* More launch tuning that never changes results: tiles = 16x16-pixel tiles a workgroup of the wavefront schedule's level-1
 * launch runs one after the other: 1, 2 or 3; 0 restores the default. Only scenes served from LDS, on the per-lane walk,
 * without counters, features, frame batches or AOV planes, and with xcd_chunk == 1 have such kernels; every other frame runs with 1
 * whatever is set here (p3d_last_primary_tiles() tells). P3D_PRIMARY_TILES=1..3 in the environment sets the same for every
 * scene created afterwards (measurement scripts: profiles/r06_primary_tiles.txt). */
int p3d_set_primary_tiles(p3d_scene* scene, int32_t tiles);
/* Tiles per workgroup the level-1 launch of the most recent p3d_render() / p3d_render_frames() of this scene ran with
 * (1 on the tile and tree schedules). P3D_ERR_STATE before the first render. */
int p3d_last_primary_tiles(p3d_scene* scene, int32_t* tiles);

/* Tile coverage mask of those multi-tile level-1 kernels, another switch that never changes results: on = 1 gives every
 * eligible frame a mask of the 16x16 tiles a primitive can project onto, made by one small launch on the frame's stream in
 * front of level 1 (camera from its arguments, primitives from the device-resident scene: it follows p3d_scene_update and
 * p3d_scene_rebuild, copies nothing from the host and waits for nothing).  A tile outside the mask gets the background
 * colour and hit_id -1 without a camera ray, a walk or shading; a workgroup with no tile inside it also skips its copy of
 * the scene.  The mask is conservative: the projected vertices of a triangle and the projected corners of a sphere's or a
 * box's bounds, per row of tiles, widened by two pixels; a primitive with a vertex or corner that is not in front of the eye
 * marks every tile, and the frame runs as it would without a mask.
 *  - eligible: a frame of p3d_render() whose level-1 launch is such a kernel (p3d_set_primary_tiles: tiles 2 or 3 and the
 *    conditions listed there), with spp == 0, without P3D_FEATURE_SKYBOX, of a scene without planes.  Sharded frames
 *    (world > 1) are eligible: a tile's rows are mapped to image rows exactly.  A frame captured into a graph takes its
 *    pre-pass with it, unless the mask's buffer would have to be allocated during the capture.  Every other frame --
 *    p3d_render_frames, p3d_render_aov, counters, features, samples, the other schedules -- runs exactly as before.
 *  - default: see kDefaultSkyTiles (csrc/p3d_kernel_variant.h) and profiles/sky_tiles.txt; P3D_SKY_TILES=0 / 1 in the
 *    environment sets it for every scene created afterwards.
 * P3D_ERR_ARG: a NULL scene, on outside 0 and 1. */
int p3d_set_sky_tiles(p3d_scene* scene, int32_t on);
/* Whether the most recent p3d_render() / p3d_render_frames() / p3d_render_aov() of this scene ran with such a mask
 * (*used = 1) and how many of the frame's tiles (this rank's, when sharded) it marked empty.  *used = 0, *empty_tiles = 0
 * for a frame that was not eligible and for one whose mask marked every tile because a primitive was not in front of the
 * eye.  Waits for the scene's stream (the marks are read back from the device): P3D_ERR_STATE while it is being captured,
 * and before the first render. */
int p3d_last_sky_tiles(p3d_scene* scene, int32_t* used, int32_t* empty_tiles);

/* Reflection children that the Fresnel term multiplies by zero, a switch that changes no bit of a frame of a finite scene:
 * the reference computes KR = 1 / 2 * (R0 + R1) for every material with T != 0 -- an integer division, so KR is +0 (SURVEY
 * Q5) -- and a node returns color + reflection_color * KR * spec + refraction_color * (1 - KR).  on = 1: a node whose
 * material has T != 0 spawns no reflection child; the child's closest-hit walk, its shadow queries and its whole subtree are
 * skipped, and the node adds the zero the reference adds for a child it never traced.  A finite child colour times +0 is a
 * zero of either sign, and the sum it goes into is added to a colour that is never -0: the node keeps every bit
 * (finding 5).
 *  - applies to every entry that shades -- p3d_render, p3d_render_frames, p3d_render_aov, p3d_trace_rays --, on all three
 *    schedules, with samples and without, with either scene placement.  The kernels read the switch in the scene's
 *    material records (no launch parameter, no instruction in the kernels that prune): a call that changes the setting
 *    BLOCKS -- it queues the rewritten records on the scene's stream behind the frames in flight and returns when the
 *    copy has been made (frames queued on a stream the scene used before a p3d_set_stream are the caller's to wait for)
 *    --, and a captured frame replays with the setting in force when it is replayed.
 *  - never applies to frames with P3D_FLAG_COUNTERS (their ray counts stay the reference's) or P3D_FEATURE_SCHLICK
 *    (SCHLICK_APPROX makes KR non-zero): they trace every ray whatever is set here.
 *  - the one exception: a skipped subtree that would have returned an infinite or NaN component.  The reference's pixel is
 *    then NaN (inf * 0) and the pruned frame's is not.  Finite rays meet that only through non-finite or overflowing scene
 *    data or a degenerate configuration (a zero-radius sphere, a zero-area triangle, a hit point that coincides with a
 *    light, L + V == 0 under a specular material): results for those are unspecified here as they are after a
 *    p3d_scene_update with non-finite data.  What p3d_scene_create can see of it -- a material, light or background
 *    component or a flattened triangle / plane normal that is not finite -- keeps the switch off for the handle's
 *    lifetime: p3d_get_prune_reflections() reports 0 whatever was set.
 *  - default: see kDefaultPruneReflections (csrc/p3d_kernel_variant.h) and profiles/prune_reflections.txt;
 *    P3D_PRUNE_REFLECTIONS=0 / 1 in the environment sets it for every scene created afterwards.
 * The schedule choice of the handle is measured again after a change.  P3D_ERR_ARG: a NULL scene, on outside 0 and 1.
 * P3D_ERR_STATE: a change while the scene's stream is being captured. */
int p3d_set_prune_reflections(p3d_scene* scene, int32_t on);
/* *on = 1 if frames of this scene prune: the switch is on and the scene was finite when it was created. */
int p3d_get_prune_reflections(const p3d_scene* scene, int32_t* on);
/* Closest-hit rays queued per tree level by the most recent wavefront-schedule frame (p3d_render, p3d_render_frames,
 * p3d_render_aov) or ray stream (p3d_trace_rays) of this scene: counts[l - 1] = rays of level l for l = 1 .. min(n,
 * max_depth), zero beyond; 1 <= n <= 16.  Level 1 is the frame's camera rays (the stream's rays); a deeper level is the sum
 * of the shard counters its launch read, which stay on the device until the handle's next wavefront pass.  On the last level
 * of a frame with max_depth >= 2 a node's two children travel as a pair of slots and the figure counts slots: twice the
 * nodes of level max_depth - 1 that have a child, an absent sibling included.  Waits for the scene's stream.
 * P3D_ERR_STATE: while the stream is being captured; before the first such frame; when the most recent p3d_render* call ran
 * the tile or the tree schedule; when the frame ran more passes than it has sets of counters (one per concurrent pass, four:
 * a frame of up to four sample passes or bands is summed over them, one of more -- spp >= 3, or a frame cut into many bands
 * because its queues exceed the workspace budget -- has lost its earlier passes).  P3D_ERR_ARG: a NULL argument, n outside
 * 1..16. */
int p3d_last_level_rays(p3d_scene* scene, uint32_t* counts, int32_t n);

/* Elapsed device time of the most recent render made with P3D_FLAG_PROFILE (waits for it):
 * the whole frame (all launches of the call, samples and bands included) and its dominant
 * kernel alone -- wf_primary_kernel, or whitted_tree_kernel with P3D_FLAG_TREE_KERNEL -- for
 * the first sample / band. HIP events on the scene's stream. */
int p3d_get_profile(p3d_scene* scene, float* frame_ms, float* kernel_ms);

/* Kernel schedule the most recent p3d_render() of this scene used: 0 = wavefront (level kernels),
 * 1 = tree (one launch, per-lane stacks), 2 = tile (one launch, per-tile levels). P3D_ERR_STATE before the
 * first render. */
int p3d_last_schedule(p3d_scene* scene, int32_t* schedule);

/* Schedule choice under the caller's load. For scenes read from HBM the library measures its kernel schedules (and whether
 * the lanes of a wave share their BVH walks) on the first frames of a configuration, ONE frame at a time, and keeps the
 * fastest (p3d_last_schedule). A caller that keeps several frames in flight -- n scene handles of the same scene, one
 * stream each -- can have the same candidates measured the way it runs them: every candidate renders `frames` frames
 * (<= 0: 3) on all n handles at once, timed as a batch on the host clock, and all handles adopt the candidate with the
 * shortest time per frame for this configuration (resolution, depth, accel, spp, flags, features). outs[i] is where
 * handle i renders (device memory: the frames are real frames; results never depend on the choice). Synchronous.
 * ms_per_frame (6 floats or NULL): wavefront / tree / tile with shared walks, then with private walks; -1 = not
 * available. best (or NULL): the adopted candidate's index, -1 when this configuration's schedule is set by rule
 * (scenes served from LDS) or by a P3D_FLAG_* of params -- then nothing is measured. Not while capturing a graph. */
int p3d_tune_schedule(p3d_scene** scenes, int32_t n, const p3d_camera* cam, const p3d_render_params* params,
                      const p3d_outputs* outs, int32_t frames, float* ms_per_frame, int32_t* best);

/* Use an existing hipStream_t (e.g. the caller's framework stream); NULL restores the
 * scene's own stream. */
int p3d_set_stream(p3d_scene* scene, void* hip_stream);

/* HIP-event bracket on the scene's stream: begin, enqueue renders, end -> elapsed ms of
 * everything enqueued in between (waits for completion). */
int p3d_timer_begin(p3d_scene* scene);
int p3d_timer_end(p3d_scene* scene, float* elapsed_ms);

/* Rank-0 side of the multi-GPU frame: `gathered` points at rank 0's compact
 * tile buffer (p3d_local_rows() rows); rank r's buffer starts rank_stride_bytes * r further
 * (0 = buffers back to back). Writes the full bottom-up frame. bytes_per_pixel = 3 (rgb8),
 * 12 (rgb32f) or 4 (hit_id). Device pointers, enqueued on the scene's stream. */
int p3d_deinterleave(p3d_scene* scene, const void* gathered, void* frame, int32_t res_x,
                     int32_t res_y, int32_t row_block, int32_t world, int32_t bytes_per_pixel,
                     uint64_t rank_stride_bytes);
/* The same for a batch of n_frames frames in ONE launch: frame f of rank r starts at
 * gathered + r * rank_stride_bytes + f * tile_stride_bytes (0 = one compact tile buffer; rank stride 0 =
 * n_frames tile buffers back to back) and is written to frames + f * frame_stride_bytes (0 = frames
 * back to back). Rows and strides that are multiples of 16 bytes are moved 16 bytes at a time. */
int p3d_deinterleave_frames(p3d_scene* scene, const void* gathered, void* frames, int32_t res_x, int32_t res_y,
                            int32_t row_block, int32_t world, int32_t bytes_per_pixel, uint64_t rank_stride_bytes,
                            int32_t n_frames, uint64_t tile_stride_bytes, uint64_t frame_stride_bytes);

/* ---- the multi-GPU frame (replaces nothing in the reference, which is one CPU thread:
 * it is what main()'s "renderScene(); save image" (RT/main.cpp:966-970) becomes on N GPUs) ----
 * Every rank renders its row blocks (p3d_render with rank / world) into a compact tile buffer of
 * p3d_local_rows() rows; ONE gather per frame moves the tile buffers to rank 0 over RCCL (grouped
 * ncclSend / ncclRecv: each peer writes straight into rank 0's memory over its own xGMI link, no ring),
 * where p3d_deinterleave() restores row order.  Scene + BVH are replicated: one p3d_scene per device. */
typedef struct p3d_comm p3d_comm;
#define P3D_COMM_ID_BYTES 128

/* One process per GPU: rank 0 makes an id (ncclGetUniqueId), the launcher carries its 128 bytes to the
 * other ranks (a torch.distributed / MPI broadcast, a file, ...), then every rank calls p3d_comm_create
 * with the same id (ncclCommInitRank; blocks until all `world` ranks have called). */
int p3d_comm_unique_id(void* id_out /* P3D_COMM_ID_BYTES */);
int p3d_comm_create(const void* id, int rank, int world, int device, p3d_comm** out);
/* One process driving n GPUs: out[r] is rank r on devices[r] (NULL = devices 0..n-1); ncclCommInitAll. */
int p3d_comm_create_all(const int* devices, int n, p3d_comm** out /* [n] */);
int p3d_comm_destroy(p3d_comm* comm);
int p3d_comm_info(const p3d_comm* comm, int* rank, int* world, int* device);

/* The gather, enqueued on `scene`'s stream (scene and comm on the same device): rank r > 0 sends
 * tile_bytes from `tile`; rank 0 receives rank r's bytes at gathered + r * tile_bytes and copies its own
 * tile to gathered + 0 (skipped when tile == gathered).  `gathered` is only read on rank 0.  Device
 * pointers.  Asynchronous: p3d_sync() / stream order as usual.  world == 1 degenerates to the copy. */
int p3d_gather(p3d_comm* comm, p3d_scene* scene, const void* tile, void* gathered, uint64_t tile_bytes);
/* The same for all n ranks of a p3d_comm_create_all() group from ONE thread (their sends and receives
 * must share one RCCL group): comms[r], scenes[r], tiles[r] belong to rank r. */
int p3d_gather_all(p3d_comm* const* comms, p3d_scene* const* scenes, const void* const* tiles, int n,
                   void* gathered, uint64_t tile_bytes);

/* Device memory on a scene's device for callers that have no HIP runtime of their own (the C++ host
 * layer): allocate / free, and copy from / to the host (enqueued on the scene's stream, waits for it). */
int p3d_device_alloc(p3d_scene* scene, uint64_t bytes, void** out);
int p3d_device_free(p3d_scene* scene, void* ptr);
int p3d_upload(p3d_scene* scene, void* device_dst, const void* host_src, uint64_t bytes);
int p3d_download(p3d_scene* scene, void* host_dst, const void* device_src, uint64_t bytes);

/* (Diagnostic build only -- make -C csrc stamps, libp3d_hip_stamps.so: the product library compiles the hooks out and
 * answers P3D_ERR_STATE to a non-NULL buffer.) With a device buffer of (tiles x waves-per-workgroup x 8) uint64 set here, the
 * level-1 kernel writes per-wave 100 MHz timestamps (tile start, after ray generation, after the
 * closest hit, after shading, after the queue append; slot 7 = hardware id). NULL turns it off
 * (default). Never changes results. tools/stamps.py turns them into a per-stage timeline. */
int p3d_debug_set_stamps(p3d_scene* scene, void* device_buffer);
/* Which launch of a frame writes the stamps: 1 (default) = the level-1 launch of the wavefront schedule, or the
 * single launch of the tree schedule (slots 0 = wave start, 4 = wave end); l >= 2 = the wavefront schedule's level-l
 * launch, ONE RECORD PER WAVE of that launch (buffer: waves x 8 uint64; at most 65536 waves are launched): slots
 * 0 start, 1 queue read, 2 closest hit, 3 shading (incl. shadow queries), 4 queue append / pair combine of the wave's
 * first batch, 5 wave done, 6 = number of batches it ran, 7 = hardware id. */
int p3d_debug_set_stamp_level(p3d_scene* scene, int32_t level);

/* Unit-level probe used by the parity tests: intersect n rays with one primitive each using
 * the DEVICE intersectors (Sphere/Triangle/aaBox/Plane::intercepts, RT/scene.cpp:55-283).
 * Host arrays: type[n], prim12[n*12] (plane = PN,D), origin[n*3], dir[n*3] -> hit[n], t[n],
 * normal[n*3] (getNormal(hit point).normalize()).  type: 0 sphere, 1 triangle, 2 box, 3 plane, and 4 = a triangle
 * through the reciprocal form of the test (1 / det by csrc/p3d_device_math.h's frcp()) that scenes read from HBM use:
 * the same bits as type 1 on every input. */
int p3d_debug_intersect(int device, uint32_t n, const uint32_t* type, const float* prim12,
                        const float* origin, const float* dir, int32_t* hit, float* t,
                        float* normal);

/* Unit-level probe of the one transcendental of the path: out[i] = the device's restatement of the host C library's
 * powf(x[i], y[i]) (the Blinn-Phong exponent, RT/main.cpp:520; csrc/p3d_powf.h). Host arrays of n floats.
 * The parity tests compare it bit for bit with the box's own libm. */
int p3d_debug_powf(int device, uint32_t n, const float* x, const float* y, float* out);

/* Unit-level probes of P3D_FEATURE_SCHLICK: out[i] = the device's restatement of the host C library's pow(x[i], y[i])
 * (csrc/p3d_pow.h; n doubles each), and out[i] = the KR expression of RT/main.cpp:700-701 as the shading evaluates it on
 * (ior_1[i], new_ior[i], cos_theta_i[i]) (n floats each). The parity tests compare both bit for bit with the host. */
int p3d_debug_pow(int device, uint32_t n, const double* x, const double* y, double* out);
int p3d_debug_schlick_kr(int device, uint32_t n, const float* ior_1, const float* new_ior, const float* cos_theta_i, float* out);

/* Exhaustive check of the device's 3-instruction reciprocal (csrc/p3d_device_math.h: frcp) against the correctly rounded
 * division 1.0f / x it replaces in normalize() and Triangle::intercepts: the bit patterns first_bits .. first_bits +
 * count - 1 (count <= 2^32: all floats). n_bad = patterns whose results differ (NaN = NaN), first_bad = the lowest. */
int p3d_debug_check_rcp(int device, uint32_t first_bits, uint64_t count, uint64_t* n_bad, uint32_t* first_bad);
/* The same check for rcp_len(x) (csrc/p3d_device_math.h), the branch-free reciprocal that normalize() applies to a
 * square root's output. */
int p3d_debug_check_rcp_len(int device, uint32_t first_bits, uint64_t count, uint64_t* n_bad, uint32_t* first_bad);

/* The tree of the device builder (p3d_build_opts::builder == 1; csrc/bvh_device.hip), built by the function p3d_scene_create
 * calls, over n >= 4 build primitives given as host arrays: padded bounds lo3[n*3], hi3[n*3] and the reference ref[n] each
 * carries into the leaf list. Returns, with L = (n + 1) / 2 leaves of two primitives (the last of an odd n holds one):
 * nodes16[(L-1)*16] = the L - 1 node pairs as the kernels read them (12 floats: child 0's lo xyz, hi xyz, child 1's lo xyz,
 * hi xyz; child0, child1 -- an inner node's index, or ~(first << 3 | count - 1) for the leaf that starts at leaf_refs[first];
 * two zero dwords), leaf_refs[n], stats4 = {n_nodes, n_leaves, n_leaf_refs, max_depth}, and sah_cost. max_depth counts the
 * leaf level: the walks' stacks are sized from it. n < 4 or a NULL pointer: P3D_ERR_ARG (scenes of fewer than 64
 * primitives are built on the host by p3d_scene_create; that threshold is not this entry's). */
int p3d_debug_lbvh_build(int device, uint32_t n, const float* lo3, const float* hi3, const uint32_t* ref, uint32_t* nodes16,
                         uint32_t* leaf_refs, uint32_t* stats4, float* sah_cost);
/* The same for builder 2 (csrc/bvh_ploc.hip), run by the function p3d_scene_create and p3d_scene_rebuild_with call: the same
 * leaves and leaf_refs; node 0 is the root and every inner child's index is above its parent's.  *rounds = clustering rounds
 * run (at most 95); *fell_back = 1 when clusters were left after them and everything returned is builder 1's tree. */
int p3d_debug_ploc_build(int device, uint32_t n, const float* lo3, const float* hi3, const uint32_t* ref, uint32_t* nodes16,
                         uint32_t* leaf_refs, uint32_t* stats4, float* sah_cost, int32_t* rounds, int32_t* fell_back);

/* The device grid build of p3d_scene_build_grid (csrc/grid_device.hip), run by the same function over host arrays: n boxes
 * lo3[n*3], hi3[n*3] in scene order and the reference ref[n] each is listed under (n == 0: the arrays may be NULL).  Returns
 * dims3 (cells per axis), mn3 / mx3 (the grid's box), *n_cells, *n_items, and -- unless cell_start or items is NULL, which
 * asks for the sizes only -- the first min(cell_cap, n_cells + 1) words of cell_start and min(item_cap, n_items) words of
 * items: what the host build (p3dh_grid_dump) makes of the same boxes, in every word.  P3D_ERR_LIMIT as for
 * p3d_scene_build_grid; P3D_ERR_ARG for a NULL size output or NULL boxes with n > 0. */
int p3d_debug_grid_build(int device, uint32_t n, const float* lo3, const float* hi3, const uint32_t* ref, int32_t* dims3,
                         float* mn3, float* mx3, uint64_t* n_cells, uint64_t* n_items, uint32_t* cell_start, uint64_t cell_cap,
                         uint32_t* items, uint64_t item_cap);

/* Unit-level probes of p3d_generate_samples (csrc/p3d_rand.h, csrc/sample_stream.hip); host arrays, synchronous.
 * p3d_debug_rand: out[i] = the device's restatement of the value number first + i that the host C library's rand()
 * returns after srand(seed), i < n; every device thread reaches its own position by a jump (first is 64-bit: positions
 * no serial loop reaches).  p3d_debug_sample_stream: the generator itself into a host array, with every pass forced to read
 * pairs_per_pass pairs of draws (0 = the entry's own sizing); *passes = how many passes ran, so that a test can take the
 * continuation path on purpose -- with 2, a pass can end between a sample's jitter and its lens pair. */
int p3d_debug_rand(int device, uint32_t seed, uint64_t first, uint32_t n, uint32_t* out);
int p3d_debug_sample_stream(int device, uint32_t seed, int32_t res_x, int32_t res_y, int32_t spp, float aperture,
                            uint64_t pairs_per_pass, float* out, int32_t* passes);

/* The launches of p3d_denoise (csrc/denoise.hip) run by the same function over HOST planes, without a scene: params and
 * in as p3d_denoise reads them with in->memory == 0, out->rgb32f / out->rgb8 (each may be NULL) with out->memory == 0.
 * Synchronous; scratch is allocated for the call and freed.  Refusals as p3d_denoise (in->memory or out->memory other than
 * 0: P3D_ERR_ARG). */
int p3d_debug_denoise(int device, const p3d_denoise_params* params, const p3d_denoise_inputs* in, const p3d_outputs* out);
/* Likewise the launches of p3d_denoise_variance (csrc/denoise_variance.hip) over HOST planes, without a scene.  Refusals as
 * p3d_denoise_variance (in->memory or out->memory other than 0: P3D_ERR_ARG). */
int p3d_debug_denoise_variance(int device, const p3d_denoise_params* params, const p3d_denoise_variance_inputs* in,
                               const p3d_denoise_variance_outputs* out);
/* Likewise the launch of p3d_upsample (csrc/upsample.hip) over HOST planes, without a scene.  Refusals as p3d_upsample
 * (in->memory or out->memory other than 0: P3D_ERR_ARG). */
int p3d_debug_upsample(int device, const p3d_upsample_params* params, const p3d_upsample_inputs* in, const p3d_upsample_outputs* out);

/* The launches of p3d_accumulate (csrc/accumulate.hip) run by the same function over HOST planes, without a scene: the
 * four structs as p3d_accumulate reads them, every memory field 0.  Synchronous; scratch is allocated for the call and
 * freed.  Refusals as p3d_accumulate (a memory field other than 0: P3D_ERR_ARG). */
int p3d_debug_accumulate(int device, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                         const p3d_accumulate_history* history, const p3d_accumulate_outputs* out);
/* Likewise the launches of p3d_accumulate_moving (csrc/accumulate.hip) over HOST planes and HOST geometry, without a
 * scene.  Refusals as p3d_accumulate_moving (a memory field other than 0: P3D_ERR_ARG). */
int p3d_debug_accumulate_moving(int device, const p3d_accumulate_params* params, const p3d_accumulate_frames* frames,
                                const p3d_accumulate_history* history, const p3d_accumulate_motion* motion,
                                const p3d_accumulate_moving_outputs* out);
/* Likewise the launches of p3d_accumulate_variance (csrc/accumulate.hip) over HOST planes and HOST geometry,
 * without a scene.  Refusals as p3d_accumulate_variance (a memory field other than 0: P3D_ERR_ARG). */
int p3d_debug_accumulate_variance(int device, const p3d_accumulate_params* params, const p3d_accumulate_variance_params* variance_params,
                                  const p3d_accumulate_frames* frames, const p3d_accumulate_history* history, const float* history_moments,
                                  const p3d_accumulate_motion* motion, const p3d_accumulate_variance_outputs* out);

#ifdef __cplusplus
}
#endif
#endif /* P3D_HIP_H */
