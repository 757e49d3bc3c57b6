"""balls_high.p3f on the GPU: the level-4 sphereflake the reference ships (7 381 spheres, one plane, three lights, Ks 0.5 on
every sphere).  Its sphere records alone exceed the LDS budget, so every frame walks the 32-byte quantised BVH nodes
from HBM, with the plane gate, tiny tangent spheres (radii down to 0.006) and reflection chains starting next to them.

Frames are compared with tests/golden/balls_high_frames.npz (rendered by oracle/_ref, tests/golden/make_balls_high_golden.py)
and with live oracle renders, at the project's bar: rgb32f bit for bit (conftest.RGB_TOL = 0), rgb8 equal, primary hit
ids equal, closest / shadow query counts and ray counts equal.  Everything goes through the C-ABI.

Every test here makes a fresh handle per configuration (or repeats one configuration).  One handle rendered with several
row_block values, resolutions, worlds, depths and accel modes -- the tile-order key holds row_block since the keys were
named (csrc/p3d_frame_config.h) -- is tests/test_gpu_handle_walks.py.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, RGB_TOL, assert_rgb8_equal
from extra_scenes import scene_path
from handle_walks import stitch
from oracle import oracle_py as O
import u_4a_2s_p3d_raytracer_template2_amd as P

pytestmark = pytest.mark.gpu

SCENE = "balls_high"
FRAMES = np.load(os.path.join(GOLDEN, "balls_high_frames.npz"))
CASES = {n: json.loads(str(FRAMES[n + "/meta"])) for n in sorted({k.split("/")[0] for k in FRAMES.files})}
BIG = "bh_200x150_d4_bvh"          # >= 64 tiles on every schedule (130 16x16 tiles, 520 16x4 tiles)
SCHEDULES = ["tile", "wavefront", "tree"]
THREADS = 16


def handle(res, **opts):
    hs = P.HostScene(scene_path(SCENE))
    if res is not None:
        hs.set_resolution(*res)
    return hs, P.DeviceScene.from_host(hs, **opts)


def render_args(m, hs, **over):
    kw = dict(max_depth=m["max_depth"], accel=m["accel"], spp=m["spp"], soft_shadow=m["soft_shadow"], counters=True,
              samples=hs.samples(m["seed"], m["spp"]) if m["spp"] else None)
    kw.update(over)
    return kw


def render_case(name, opts=None, **over):
    m = CASES[name]
    hs, ds = handle(m["res"], **(opts or {}))
    out = ds.render(hs.camera(), **render_args(m, hs, **over))
    out["schedule"] = ds.last_schedule()
    ds.close()
    return out


def compare(out, rgb8, rgb32f, hit_id, what):
    assert np.array_equal(out["hit_id"], hit_id), "%s: primary hit ids differ in %d px, first at %s" % (
        what, int((out["hit_id"] != hit_id).sum()), np.argwhere(out["hit_id"] != hit_id)[:1].tolist())
    assert np.isfinite(out["rgb32f"]).all(), what
    bad = (out["rgb32f"].view(np.uint32) != rgb32f.view(np.uint32)).any(-1)
    diff = float(np.abs(out["rgb32f"].astype(np.float64) - rgb32f.astype(np.float64)).max())
    assert diff <= RGB_TOL and not bad.any(), "%s: rgb32f differs in %d px (max %g), first at %s" % (
        what, int(bad.sum()), diff, np.argwhere(bad)[:1].tolist())
    assert_rgb8_equal(out["rgb8"], rgb8, what)


def assert_fixture(out, name, what, counters=True):
    compare(out, FRAMES[name + "/rgb8"], FRAMES[name + "/rgb32f"], FRAMES[name + "/hit_id"], what)
    if counters:
        c, m = out["counters"], CASES[name]
        assert c["closest_queries"] == m["counters"]["closest_queries"], what
        assert c["shadow_queries"] == m["counters"]["shadow_queries"], what
        assert c["rays"] == int(FRAMES[name + "/rays"]) == m["counters"]["rays"], what
        assert c["pixels"] == m["res"][0] * m["res"][1], what


def assert_oracle(out, ref, what):
    compare(out, ref["rgb8"], ref["rgb32f"], ref["hit_id"], what)
    for k in ("closest_queries", "shadow_queries", "rays"):
        assert out["counters"][k] == ref["counters"][k], (what, k)


_oracle_cache = {}


def oracle(res, accel, depth):
    key = (tuple(res), accel, depth)
    if key not in _oracle_cache:
        sc = O.Scene(scene_path(SCENE))
        sc.set_resolution(*res)
        _oracle_cache[key] = sc.render(max_depth=depth, accel=accel, threads=THREADS)
    return _oracle_cache[key]


# ---- every fixture frame, every schedule, both walks of a scene read from HBM

@pytest.mark.parametrize("private_walk", [False, True], ids=["shared", "private"])
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_balls_high_frame_is_the_reference_frame(name, schedule, private_walk):
    out = render_case(name, private_walk=private_walk, **{schedule: True})
    assert_fixture(out, name, "%s %s private_walk=%s" % (name, schedule, private_walk))


@pytest.mark.parametrize("opts", [dict(leaf_max=1), dict(leaf_max=2), dict(leaf_max=8), dict(builder=1)],
                         ids=["leaf1", "leaf2", "leaf8", "lbvh"])
def test_balls_high_is_independent_of_the_bvh_shape(opts):
    """Host SAH trees with 1, 2 and 8 primitives per leaf and the LBVH built on the GPU: other quantised nodes, other
    leaf orders, the same nearest hits and lowest-id ties."""
    for kw in (dict(), dict(private_walk=True)):
        out = render_case(BIG, opts, **kw)
        assert_fixture(out, BIG, "%s %s" % (opts, kw))


# ---- state kept on one handle over many frames

def test_measured_schedule_pick_keeps_the_reference_frame():
    """No schedule forced: the first 2 x 6 + 1 frames run every candidate (3 schedules x shared / private walks) and pick
    the fastest, later frames draw their tiles heaviest first.  Every frame is the reference's."""
    m = CASES[BIG]
    hs, ds = handle(m["res"])
    kw = render_args(m, hs)
    seen = []
    for k in range(2 * 6 + 1 + 4):
        out = ds.render(hs.camera(), **kw)
        assert_fixture(out, BIG, "default schedule, frame %d" % k)
        seen.append(ds.last_schedule())
    ds.close()
    assert len(set(seen[:13])) == 3, seen            # a scene read from HBM: measured, not picked by rule
    assert len(set(seen[13:])) == 1, seen            # ... and the pick stays


@pytest.mark.parametrize("private_walk", [False, True], ids=["shared", "private"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_forced_schedule_repeated_frames_keep_the_reference_frame(schedule, private_walk):
    """The first frame measures every tile, the next ones draw the tiles in the learned heaviest-first order."""
    m = CASES[BIG]
    hs, ds = handle(m["res"])
    kw = render_args(m, hs, private_walk=private_walk, **{schedule: True})
    for k in range(4):
        out = ds.render(hs.camera(), **kw)
        assert ds.last_schedule() == schedule
        assert_fixture(out, BIG, "%s private_walk=%s frame %d" % (schedule, private_walk, k))
    ds.close()


# ---- shards of the frame (row blocks dealt round robin over ranks)

def shards(name, world, rb, **over):
    m = CASES[name]
    hs, ds = handle(m["res"])
    kw = render_args(m, hs, rank=0, world=world, row_block=rb, **over)
    parts = []
    for r in range(world):
        kw["rank"] = r
        parts.append(ds.render(hs.camera(), **kw))
        assert parts[-1]["rgb8"].shape[0] == P.local_rows(m["res"][1], rb, world)
    ds.close()
    return stitch(parts, m["res"][1], m["res"][0], world, rb)


@pytest.mark.parametrize("schedule", [None] + SCHEDULES, ids=["default"] + SCHEDULES)
@pytest.mark.parametrize("world", [2, 3])
def test_shards_stitch_to_the_reference_frame(world, schedule):
    st = shards(BIG, world, 16, **({schedule: True} if schedule else {}))
    assert_fixture(st, BIG, "world %d %s" % (world, schedule))


@pytest.mark.parametrize("schedule", [None] + SCHEDULES, ids=["default"] + SCHEDULES)
def test_row_block_32_shards_on_a_fresh_handle(schedule):
    st = shards(BIG, 2, 32, **({schedule: True} if schedule else {}))
    assert_fixture(st, BIG, "row_block 32 world 2 %s" % schedule)


# ---- against the live oracle

def test_scene_as_shipped_against_live_oracle():
    """balls_high.p3f as the reference ships it: 512x512, accel 0 (brute force), depth 4."""
    hs, ds = handle(None)
    assert (hs.camera().res_x, hs.camera().res_y) == (512, 512)
    ref = oracle((512, 512), 0, 4)
    for kw in (dict(), dict(tree=True), dict(tile=True, private_walk=True)):
        out = ds.render(hs.camera(), max_depth=4, accel=0, counters=True, **kw)
        assert_oracle(out, ref, "as shipped %s" % kw)
    ds.close()


def test_full_hd_bvh_against_live_oracle():
    ref = oracle((1920, 1080), 2, 4)
    hs, ds = handle((1920, 1080))
    for kw in (dict(), dict(tile=True), dict(wavefront=True), dict(tree=True), dict(tree=True, private_walk=True)):
        out = ds.render(hs.camera(), max_depth=4, accel=2, counters=True, **kw)
        assert_oracle(out, ref, "1080p bvh %s" % kw)
    ds.close()


@pytest.mark.parametrize("depth", [8, 10])
def test_deep_reflection_chains_against_live_oracle(depth):
    """The tree kernel keeps its per-level frames in private memory for scenes read from HBM up to depth 8 and in LDS
    beyond: one depth on each side, on every schedule."""
    ref = oracle((128, 128), 2, depth)
    hs, ds = handle((128, 128))
    for kw in (dict(tree=True), dict(tree=True, private_walk=True), dict(tile=True), dict(wavefront=True)):
        out = ds.render(hs.camera(), max_depth=depth, accel=2, counters=True, **kw)
        if kw.get("tree"):
            assert ds.last_schedule() == "tree"
        assert_oracle(out, ref, "depth %d %s" % (depth, kw))
    ds.close()


@pytest.mark.parametrize("res", [(128, 128), (1920, 1080)], ids=["128", "1080p"])
def test_grid_mode_against_live_oracle(res):
    """GRID mode over the reference's 39^3 grid: the plane lies outside it and shadow rays that miss the grid count as
    shadowed, so the frame differs from the BVH frame in many pixels; the device reproduces every one of them."""
    ref = oracle(res, 1, 4)
    bvh = oracle(res, 2, 4)
    if res == (128, 128):
        compare(ref, FRAMES["bh_128_d4_grid/rgb8"], FRAMES["bh_128_d4_grid/rgb32f"], FRAMES["bh_128_d4_grid/hit_id"], "oracle")
    where = (ref["rgb8"] != bvh["rgb8"]).any(axis=2)
    assert where.sum() > res[0] * res[1] // 4, int(where.sum())
    hs, ds = handle(res)
    for kw in (dict(), dict(tile=True), dict(wavefront=True), dict(tree=True)):
        out = ds.render(hs.camera(), max_depth=4, accel=1, counters=True, **kw)
        assert_oracle(out, ref, "grid %s %s" % (res, kw))
        assert np.array_equal(out["rgb8"][where], ref["rgb8"][where])
    ds.close()
