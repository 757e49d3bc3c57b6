// p3d_kernel_variant.h -- how the host names one build of a ray kernel, which builds of the level kernels exist, and the
// grid of the level-1 launch.  Plain C++: no HIP in here, so the host compiler can build it on its own
// (tests/test_primary_tiles_pick.py); p3d_kernels.hip makes its kernel tables of the same functions.
#ifndef P3D_KERNEL_VARIANT_H
#define P3D_KERNEL_VARIANT_H

namespace p3d {

// WALK selects the walk of a ray kernel at compile time (p3d_shade.h: TravCtx)
enum { WALK_LANE = 0, WALK_PACKET = 1, WALK_GRID = 2, WALK_SHARED = 3 };

// One build of a ray kernel, as the host asks for it.  Not every combination is built: the dispatchers of
// p3d_kernels.hip map a request to the build that serves it (level_variant() tells which one that is).
struct KernelVariant {
    bool count = false;     // P3D_FLAG_COUNTERS
    bool lds = false;       // scene read from an LDS copy
    int walk = 0;           // WALK_LANE / _PACKET / _GRID / _SHARED
    int occ = 1;            // register budget in waves per SIMD: 5 or 6; anything else is the compiler's default
    bool stoch = false;     // features with random draws
    bool schlick = false;   // P3D_FEATURE_SCHLICK
    bool batch = false;     // frame batch (p3d_render_frames)
    int tiles = 1;          // level-1 kernel: 16x16 tiles a workgroup runs one after the other (1, 2 or 3)
    bool aov = false;       // the frame writes AOV planes (p3d_render_aov): the kernels that see primary hits are built twice
    constexpr bool operator==(const KernelVariant& o) const {
        return count == o.count && lds == o.lds && walk == o.walk && occ == o.occ && stoch == o.stoch && schlick == o.schlick &&
               batch == o.batch && tiles == o.tiles && aov == o.aov;
    }
};

// The level kernels: wf_primary_kernel, wf_secondary_kernel (no BATCH: the deeper levels are shared), wf_tile_kernel,
// wf_rays_kernel: level 1 of a ray stream (p3d_trace_rays), wf_occlusion_kernel: the shadow query on the caller's
// segments (p3d_occluded), wf_ao_kernel (ao.hip): the same query on segments made in lanes (p3d_ambient_occlusion), and
// wf_indirect_kernel (indirect.hip): a ray stream's level 1 on rays made in lanes (p3d_indirect_diffuse), and
// wf_indirect_paths_kernel (indirect_paths.hip): that level 1 in a loop, a path per lane (p3d_indirect_paths).
enum class Level { Primary, Secondary, Tile, Rays, Occlusion, AmbientOcclusion, IndirectDiffuse, IndirectPaths };
constexpr int kMaxPrimaryTiles = 3;
// what a handle asks for until p3d_set_primary_tiles() says otherwise: 2 measured 2.4 % faster than 1 on the 1080p frame of
// mount_low with four frames in flight, 3 measured 1.6 % (profiles/r06_primary_tiles.txt)
constexpr int kDefaultPrimaryTiles = 2;
// whether a handle gives the frames of those kernels a tile coverage mask (p3d_tile_coverage.h) until p3d_set_sky_tiles()
// says otherwise; the measurement behind the value is profiles/sky_tiles.txt
constexpr bool kDefaultSkyTiles = true;
// whether a handle leaves out the reflection children that KR = 1 / 2 * (R0 + R1) = +0 scales to nothing (p3d_shade.h:
// shade_hit) until p3d_set_prune_reflections() says otherwise; the measurement behind the value is
// profiles/prune_reflections.txt
constexpr bool kDefaultPruneReflections = true;

// Several tiles per workgroup are built for the level-1 kernel of scenes served from LDS, walked per lane, and there only
// for the timed builds without features: the variant exists to spread a workgroup's fixed cost (scene copy, launch
// parameters, shard set-up) over more pixels, and the other builds are not bound by it.
constexpr bool has_primary_tiles(const KernelVariant& v, Level k) {
    return k == Level::Primary && v.lds && v.walk == WALK_LANE && !v.count && !v.stoch && !v.schlick && !v.batch && !v.aov;
}
// AOV planes are written where a primary hit is in registers: the level-1 kernel, the tile kernel and the tree kernel have a
// build with the writes (AOV = true) next to the build without, which is the code it was before the planes existed, to the
// instruction -- a run-time test of the plane pointers in ONE build moved the register allocation of the tile and tree
// kernels ("AOV planes").  The deeper levels and a ray stream's level 1 never see a frame's primary hit.
constexpr bool has_aov(Level k) { return k == Level::Primary || k == Level::Tile; }
// The ray-stream level-1 kernel is built per scene placement and walk and nothing else: the per-lane, grid and shared walks
// (a packet request gets the per-lane walk), at the register budget frames run their level kernels at by default.
constexpr int kRaysOcc = 6;
// The occlusion kernel, the ambient-occlusion kernel, the indirect-diffuse kernel and the indirect-paths kernel are built by
// the same rule: five builds each, LDS x {lane, grid} and HBM x {lane, shared, grid}.
constexpr bool caller_rays(Level k) {
    return k == Level::Rays || k == Level::Occlusion || k == Level::AmbientOcclusion || k == Level::IndirectDiffuse || k == Level::IndirectPaths;
}
// the build of level kernel k that serves request v
constexpr KernelVariant canonical_level(KernelVariant v, Level k) {
    if (k == Level::Secondary) v.batch = false;
    if (!has_aov(k)) v.aov = false;
    if (caller_rays(k)) {
        v.count = v.stoch = v.schlick = v.batch = false;
        v.occ = kRaysOcc;
        if (v.walk == WALK_PACKET) v.walk = WALK_LANE;
    }
    if (v.walk == WALK_SHARED && v.lds) v.walk = WALK_LANE;        // LDS scenes have no shared walk
    // a register budget only for the timed builds of the BVH walks: grid, counting, stochastic, Schlick, batch and AOV builds use the default
    if ((v.occ != 5 && v.occ != 6) || v.walk == WALK_GRID || v.count || v.stoch || v.schlick || v.batch || v.aov) v.occ = 1;
    if (v.tiles < 2 || v.tiles > kMaxPrimaryTiles || !has_primary_tiles(v, k)) v.tiles = 1;
    return v;
}
// ... and whether v itself is one of the builds of k: the one statement of which builds exist
constexpr bool built_level(const KernelVariant& v, Level k) {
    if (v.batch && k == Level::Secondary) return false;
    if (v.aov && !has_aov(k)) return false;
    if (caller_rays(k) && (v.count || v.stoch || v.schlick || v.batch || v.walk == WALK_PACKET || v.occ != (v.walk == WALK_GRID ? 1 : kRaysOcc)))
        return false;
    if (v.walk == WALK_SHARED && v.lds) return false;
    if (v.tiles != 1 && (v.tiles < 2 || v.tiles > kMaxPrimaryTiles || !has_primary_tiles(v, k))) return false;
    if (v.occ == 1) return true;
    return v.walk != WALK_GRID && !v.count && !v.stoch && !v.schlick && !v.batch && !v.aov;
}

// Grid of the level-1 launch over a band of tile_rows rows of tiles_x tiles.  LDS scenes on the identity tile map launch
// 2-D: blockIdx = (tile column, tile row), no division by a launch parameter in the kernel.  With TILES > 1 workgroup
// (bx, by) runs tile rows by, by + y, by + 2 y, ...: y = ceil(tile_rows / TILES), so a band whose rows are no multiple of
// TILES leaves the last workgroups' trailing iterations empty.
struct PrimaryGrid { unsigned x, y; };
constexpr bool primary_grid_2d(const KernelVariant& served, int tiles_x, int tile_rows, int n_tiles, int xcd_chunk) {
    return served.lds && xcd_chunk == 1 && tiles_x * tile_rows == n_tiles && (tile_rows > 1 || served.tiles > 1);
}
// (served: what served_primary() returned)
constexpr PrimaryGrid primary_grid(const KernelVariant& served, int tiles_x, int tile_rows, int n_tiles, int xcd_chunk, int grid_blocks) {
    if (!primary_grid_2d(served, tiles_x, tile_rows, n_tiles, xcd_chunk)) return {(unsigned)grid_blocks, 1u};
    return {(unsigned)tiles_x, (unsigned)((tile_rows + served.tiles - 1) / served.tiles)};
}
// The level-1 build a launch runs for request v: canonical_level(), and TILES > 1 only where the launch is 2-D (those
// kernels number their tiles by blockIdx alone).
constexpr KernelVariant served_primary(KernelVariant v, int tiles_x, int tile_rows, int n_tiles, int xcd_chunk) {
    v = canonical_level(v, Level::Primary);
    if (!primary_grid_2d(v, tiles_x, tile_rows, n_tiles, xcd_chunk)) v.tiles = 1;
    return v;
}

}  // namespace p3d
#endif
