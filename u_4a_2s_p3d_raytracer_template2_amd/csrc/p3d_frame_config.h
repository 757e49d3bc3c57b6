// p3d_frame_config.h -- what a render request asks for, the cache keys made of it, and the measured schedule choice.
// Plain C++: no HIP in here, so the host compiler can build it on its own (tests/test_schedule_pick.py).
#ifndef P3D_FRAME_CONFIG_H
#define P3D_FRAME_CONFIG_H

#include <stdint.h>

#include "p3d_hip.h"

#pragma GCC visibility push(hidden)
namespace p3d {

enum { SCHED_WAVEFRONT = 0, SCHED_TREE = 1, SCHED_TILE = 2 };
constexpr int kSchedules = 3;

// the flags that change what a schedule costs or which kernels run (the others force a schedule or say where data lives)
constexpr uint32_t kConfigFlags = P3D_FLAG_NO_LDS_SCENE | P3D_FLAG_PACKET_WALK | P3D_FLAG_COUNTERS | P3D_FLAG_PRIVATE_WALK;

// A validated, normalised request (validate_request).  Every cache key below is made of it, by one function each.
struct FrameConfig {
    int32_t res_x = 0, res_y = 0, max_depth = 0, accel = 0, spp = 0;
    int32_t rank = 0, world = 1, row_block = 16;
    uint32_t flags = 0;         // the request's flags & kConfigFlags
    uint32_t features = 0;      // P3D_FEATURE_*
    int32_t n_frames = 1;
    int32_t frame_rows = 0;     // rows of one frame this rank renders (p3d_local_rows)
    int32_t out_rows = 0;       // rows between two frames of the caller's planes
    bool batch() const { return n_frames > 1; }
};

// A cache's key: nothing matches until one was adopted, or after invalidate().
template <typename K>
struct Keyed {
    K key{};
    bool set = false;
    bool matches(const K& k) const { return set && key == k; }
    void adopt(const K& k) { key = k; set = true; }
    void invalidate() { set = false; }
};

// the measured schedule choice: everything that changes what the schedules cost
struct PickKey {
    int32_t res_x, res_y, max_depth, accel, spp, rank, world;
    uint32_t flags, features;
    int32_t n_frames;
    bool operator==(const PickKey& o) const {
        return res_x == o.res_x && res_y == o.res_y && max_depth == o.max_depth && accel == o.accel && spp == o.spp && rank == o.rank &&
               world == o.world && flags == o.flags && features == o.features && n_frames == o.n_frames;
    }
};
inline PickKey pick_key(const FrameConfig& c) {
    return {c.res_x, c.res_y, c.max_depth, c.accel, c.spp, c.rank, c.world, c.flags, c.features, c.n_frames};
}

// the workspace budget: what sizes the workspaces
struct BudgetKey {
    int32_t res_x, res_y, max_depth, spp;
    bool operator==(const BudgetKey& o) const { return res_x == o.res_x && res_y == o.res_y && max_depth == o.max_depth && spp == o.spp; }
};
inline BudgetKey budget_key(const FrameConfig& c) { return {c.res_x, c.res_y, c.max_depth, c.spp}; }

// a ray stream's reading of the workspace budget (p3d_trace_rays): streams keep their own, so that they never touch a frame's key
struct RayStreamKey {
    uint64_t budget; int32_t max_depth; uint32_t n;
    bool operator==(const RayStreamKey& o) const { return budget == o.budget && max_depth == o.max_depth && n == o.n; }
};

// a tile order: what decides the tiles' number (res, rank / world / row_block, n) and their relative cost, the schedule whose
// tiles they are, and for batches the tile count itself
struct TileOrderKey {
    int32_t res_x, res_y, max_depth, accel, spp, rank, world, row_block;
    uint32_t features;
    int32_t schedule, n_frames, batch_tiles;
    bool operator==(const TileOrderKey& o) const {
        return res_x == o.res_x && res_y == o.res_y && max_depth == o.max_depth && accel == o.accel && spp == o.spp && rank == o.rank &&
               world == o.world && row_block == o.row_block && features == o.features && schedule == o.schedule &&
               n_frames == o.n_frames && batch_tiles == o.batch_tiles;
    }
};
inline TileOrderKey tile_order_key(const FrameConfig& c, int schedule, int n_tiles) {
    return {c.res_x, c.res_y, c.max_depth, c.accel, c.spp, c.rank, c.world, c.row_block, c.features, schedule, c.n_frames,
            c.batch() ? n_tiles : 0};
}

// Schedule choice: measured, not guessed.  The first frames of a (resolution, depth, accel, spp, shard, flags, features, n)
// configuration run every available schedule twice, the second time bracketed by HIP events; later frames use the
// fastest one.  All produce identical bits, so the choice is invisible in the output.
// Candidate c is schedule c % 3; scenes whose lanes can share their walks have six (0-2 shared walks, 3-5 private).
// This class is the bookkeeping only: the caller reads the events and hands in the elapsed time.
class SchedulePick {
public:
    float ms[2 * kSchedules] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f};   // wavefront, tree, tile with shared walks; the same with private walks
    int best = SCHED_TILE;

    void invalidate() { key_.invalidate(); }
    // a choice made elsewhere (p3d_tune_schedule): adopted for k without measuring
    void adopt(const PickKey& k, int cand, int nc) {
        key_.adopt(k);
        best = cand < nc ? cand : SCHED_TILE;
        step_ = 2 * nc + 1; pending_ = -1;
    }
    // every candidate of k has had its frames (a stream being captured can use `best`, and measures nothing)
    bool measured(const PickKey& k, int nc) const { return key_.matches(k) && step_ >= 2 * nc; }
    // a frame of configuration k begins: another configuration than the last one starts the measurement over
    void begin(const PickKey& k) {
        if (key_.matches(k)) return;
        key_.adopt(k);
        for (float& m : ms) m = -1.0f;
        pending_ = -1; step_ = 0; best = SCHED_TILE;
    }
    int pending() const { return pending_; }            // candidate whose timed frame is in flight, or -1
    void collect(float elapsed_ms) {                    // ... and what that frame took
        if (ms[pending_] < 0.0f || elapsed_ms < ms[pending_]) ms[pending_] = elapsed_ms;
        pending_ = -1;
    }
    struct Next { int cand; bool timed; bool decided; };   // decided: this call made the choice (once per configuration)
    // the candidate this frame runs as: each available one twice, the second time timed; then the fastest
    Next next(int nc, const bool (&avail)[kSchedules]) {
        while (step_ < 2 * nc && !avail[(step_ / 2) % kSchedules]) step_ = (step_ / 2 + 1) * 2;     // skip what cannot run
        if (step_ < 2 * nc) {
            const Next r = {step_ / 2, (step_ & 1) != 0, false};
            step_++;
            return r;
        }
        bool decided = false;
        if (step_ == 2 * nc) {
            best = -1;
            for (int k = 0; k < nc; k++)
                if (avail[k % kSchedules] && ms[k] >= 0.0f && (best < 0 || ms[k] < ms[best])) best = k;
            if (best < 0) best = avail[SCHED_TILE] ? SCHED_TILE : (avail[SCHED_WAVEFRONT] ? SCHED_WAVEFRONT : SCHED_TREE);
            step_++;
            decided = true;
        }
        return {best, false, decided};
    }
    // the timed frame of `cand` was enqueued; a frame pushed onto another schedule by the workspace budget says the
    // measured one is not available
    void enqueued(int cand, bool ran_as_chosen) {
        if (ran_as_chosen) pending_ = cand;
        else ms[cand] = 3.0e38f;
    }

private:
    Keyed<PickKey> key_;
    int pending_ = -1, step_ = 0;
};

}  // namespace p3d
#pragma GCC visibility pop
#endif
