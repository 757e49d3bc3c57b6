"""Walks of one scene handle through configuration changes (not a test module; plain Python and numpy, no GPU).

A p3d_scene handle caches tile orders, the measured schedule choice, the workspace budget, the ray-factor table, grow-only
workspaces, the soft lights and the lazily built grid between calls (csrc/p3d_scene_state.h).  A walk is a list of steps,
each a render configuration whose expected frame is a committed fixture; consecutive steps are the transitions a cache key
can get wrong.  tests/test_handle_walks.py checks on the CPU that the walks hold the transitions they are meant to and that
the tile-order key decides the tile count; tests/test_gpu_handle_walks.py renders them on one handle each.

The arithmetic below restates p3d_local_rows (csrc/p3d_capi_misc.cpp) and the tile geometry of fill_frame_geometry /
plan_workspaces (csrc/p3d_render.cpp): image row = (blk * world + rank) * row_block + r for row blk * row_block + r of a
rank's compact buffer; 16x16 tiles for the tile schedule; 16 x (4 * wg_waves) wave tiles for the tree and wavefront
level-1 launches, wg_waves being 4 for a scene served from LDS and 1 for one read from HBM.
"""
import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CSRC = os.path.join(REPO, "u_4a_2s_p3d_raytracer_template2_amd", "csrc")

SCHED_WAVEFRONT, SCHED_TREE, SCHED_TILE = 0, 1, 2            # p3d_frame_config.h
SCHEDULE_ID = {"wavefront": SCHED_WAVEFRONT, "tree": SCHED_TREE, "tile": SCHED_TILE}
FLAG_NO_LDS_SCENE, FEATURE_SOFT_SHADOW = 4, 1                 # include/p3d_hip.h (test_handle_walks.py compares them with it)
MIN_ORDER_TILES = 64                                          # run_tile / run_tree / run_wavefront: fewer tiles draw in natural order
LDS_SCENES = {"mount_low"}                                    # served from LDS unless a step says no_lds; balls_high never fits


def tile_order_period():
    """kTileOrderPeriod of csrc/p3d_scene_state.h: a tile order is sorted again after this many frames."""
    with open(os.path.join(CSRC, "p3d_scene_state.h")) as f:
        m = re.search(r"constexpr\s+int\s+kTileOrderPeriod\s*=\s*(\d+)\s*;", f.read())
    assert m, "kTileOrderPeriod not found in p3d_scene_state.h"
    return int(m.group(1))


# ---- fixtures: the reference's own frames (tests/golden/README.md)

def _load_fixtures():
    out = {}
    bh = np.load(os.path.join(GOLDEN, "balls_high_frames.npz"))
    for n in sorted({k.split("/")[0] for k in bh.files}):
        out[n] = (bh, json.loads(str(bh[n + "/meta"])))
    fr = np.load(os.path.join(GOLDEN, "frames.npz"))
    with open(os.path.join(GOLDEN, "cases.json")) as f:
        for n, m in json.load(f).items():
            out[n] = (fr, dict(m, soft_shadow=False))
    return out


_FIXTURES = _load_fixtures()
META = {n: m for n, (_, m) in _FIXTURES.items()}


def fixture(name):
    """{"meta", "rgb8", "rgb32f", "hit_id"} of a committed frame, read-only."""
    z, m = _FIXTURES[name]
    out = {"meta": m}
    for k in ("rgb8", "rgb32f", "hit_id"):
        out[k] = z[name + "/" + k]
        out[k].setflags(write=False)
    return out


# ---- rows and tiles

def local_rows(res_y, row_block=16, world=1):
    """Rows of a rank's compact buffer: its share of the row blocks, dealt round robin, each padded to row_block rows."""
    row_block = row_block if row_block > 0 else 16
    world = world if world > 0 else 1
    nblocks = (res_y + row_block - 1) // row_block
    return ((nblocks + world - 1) // world) * row_block


def shard_rows(res_y, row_block, world, rank):
    """[(local row, image row)] of the image rows rank owns; local rows past the image are left out."""
    out = []
    for lr in range(local_rows(res_y, row_block, world)):
        blk, r = divmod(lr, row_block)
        y = (blk * world + rank) * row_block + r
        if y < res_y:
            out.append((lr, y))
    return out


def stitch(parts, H, W, world, rb):
    """The ranks' compact planes -> one frame; the counters of the shards summed."""
    st = {"rgb8": np.zeros((H, W, 3), np.uint8), "rgb32f": np.zeros((H, W, 3), np.float32),
          "hit_id": np.full((H, W), -2, np.int32)}
    for r, part in enumerate(parts):
        rows = part["rgb8"].shape[0]
        assert rows == local_rows(H, rb, world)
        for lb in range(rows // rb):
            y0 = (lb * world + r) * rb
            if y0 >= H:
                continue
            n = min(rb, H - y0)
            for k in st:
                st[k][y0:y0 + n] = part[k][lb * rb:lb * rb + n]
    st["counters"] = {k: sum(p["counters"][k] for p in parts) for k in ("closest_queries", "shadow_queries", "rays", "pixels")}
    return st


def step(fixture, row_block=16, world=1, rank=0, **flags):
    """One step of a walk.  rank: the rank rendered first; a sharded step renders every rank (calls())."""
    return dict(fixture=fixture, row_block=row_block, world=world, rank=rank, no_lds=bool(flags.pop("no_lds", False)), **flags)


def lds_scene(st):
    return META[st["fixture"]]["scene"] in LDS_SCENES and not st["no_lds"]


def step_rows(st):
    return local_rows(META[st["fixture"]]["res"][1], st["row_block"], st["world"])


def tiles16(st):
    """16x16 tiles of the tile schedule."""
    return (META[st["fixture"]]["res"][0] + 15) // 16 * (step_rows(st) // 16)


def tiles_wave(st, wg_waves=None):
    """16 x (4 * wg_waves) tiles of the tree and wavefront level-1 launches."""
    wg_waves = wg_waves or (4 if lds_scene(st) else 1)
    return (META[st["fixture"]]["res"][0] + 15) // 16 * (step_rows(st) // (4 * wg_waves))


def tiles_of(st, schedule):
    return tiles16(st) if schedule == SCHED_TILE else tiles_wave(st)


def order_used(st, schedule):
    """Whether a frame of this step on `schedule` draws its tiles through a learned order (xcd_chunk 1, whole-frame passes)."""
    m = META[st["fixture"]]
    if tiles_of(st, schedule) < MIN_ORDER_TILES:
        return False
    if schedule == SCHED_TILE:
        return True
    if lds_scene(st):
        return False            # run_tree / run_wavefront: a scene served from LDS keeps the natural order
    return not (schedule == SCHED_WAVEFRONT and m["spp"] > 0)      # sample passes run on several lanes


def tree_refuses(st):
    """validate_request: features with random draws need the tile or the wavefront schedule."""
    m = META[st["fixture"]]
    return bool(m["soft_shadow"]) and m["spp"] > 0


def calls(walk):
    """The render configurations of a walk in the order the GPU test issues them: a sharded step is one per rank."""
    out = []
    for st in walk:
        for k in range(st["world"]):
            out.append(dict(st, rank=(st["rank"] + k) % st["world"]))
    return out


def frame_config(st, schedule):
    """The 13 ints the key harness of test_handle_walks.py takes: FrameConfig's fields, the schedule and its tile count."""
    m = META[st["fixture"]]
    return [m["res"][0], m["res"][1], m["max_depth"], m["accel"], m["spp"], st["rank"], st["world"], st["row_block"],
            FLAG_NO_LDS_SCENE if st["no_lds"] else 0, FEATURE_SOFT_SHADOW if m["soft_shadow"] else 0, 1, schedule, tiles_of(st, schedule)]


# ---- the walks

BH_SCENE, ML_SCENE = "balls_high", "mount_low"
BIG = "bh_200x150_d4_bvh"       # 130 16x16 tiles / 520 wave tiles at row_block 16, world 1
A = "c2_mount_low_256x144_d4_bvh"


def _shard_walk(f, **flags):
    """One resolution, every (row_block, world) of the issue: the tile count grows, shrinks and stays equal under another
    key (200x150: 16 and 32 both give 130; 256x144: 16 and 48 both give 144), power-of-two and other row blocks, 1 to 3 ranks."""
    seq = [(16, 1), (32, 1), (16, 1), (48, 1), (16, 1), (112, 1), (48, 1), (48, 2), (16, 2), (48, 2), (48, 1),
           (16, 3), (16, 1), (16, 3), (16, 2), (16, 1)]
    return [step(f, rb, w, **flags) for rb, w in seq]


# balls_high: every frame walks the quantised nodes from HBM, so all three schedules learn tile orders
BH = _shard_walk(BIG) + [
    # accel BVH, GRID (built lazily by the first such frame), NONE, BVH and back the other way; 200x150 <-> 128x128 have 64
    # or more tiles on both sides
    step("bh_128_d4_grid"), step("bh_128_d4_none"), step(BIG), step("bh_128_d4_none"), step("bh_128_d4_grid"), step(BIG),
    # soft shadow on and off (16 sub-lights bound and unbound); 96x64 has 24 16x16 tiles: no order on the tile schedule,
    # and as two shards 48 wave tiles: none on the others either
    step("bh_96x64_d4_bvh_soft"), step(BIG), step("bh_96x64_d4_bvh_soft", 16, 2), step(BIG),
    # depth 4, 6, 4: the level queues grow and are then used partly
    step("bh_96_d6_bvh"), step(BIG),
    # spp 0, 2, 0: the lanes and the sample planes
    step("bh_64_d4_spp2"), step(BIG),
    # small to small, then the first configuration again
    step("bh_96_d6_bvh"), step("bh_64_d4_spp2"), step("bh_96x64_d4_bvh_soft"), step("bh_64_d4_spp2", 16, 2), step(BIG),
]

# mount_low: served from LDS (wg_waves 4, no learned order on the tree and wavefront schedules) unless a step says no_lds,
# which changes the wave-tile count under an otherwise equal request.  Its fixtures have one resolution of 64 or more
# tiles and no soft shadow, so those two transitions are BH's alone.
ML = _shard_walk(A) + [
    step(A, no_lds=True), step(A), step(A, no_lds=True), step(A, 48, 1, no_lds=True), step(A, 16, 2, no_lds=True),
    step(A, no_lds=True), step(A),
    step("mount_low_256x144_d4_grid"), step("mount_low_256x144_d4_none"), step(A), step("mount_low_256x144_d4_none"),
    step("mount_low_256x144_d4_grid"), step(A),
    step("c4_mount_low_96_d6_spp2"), step(A), step("mount_low_37x23_d4_bvh"), step(A), step("mount_low_1x1_d1"), step(A),
    step("c4_mount_low_96_d6_spp2"), step("mount_low_37x23_d4_bvh", 16, 2), step("mount_low_1x1_d1"),
    step("c4_mount_low_96_d6_spp2", 48, 1), step(A),
]

WALKS = {"BH": (BH_SCENE, BH), "ML": (ML_SCENE, ML)}
