"""balls_high.p3f, the level-4 sphereflake: tests/golden/balls_high_frames.npz holds REFERENCE output (the reference's
own rayTracing() object code, tests/golden/make_balls_high_golden.py).  The oracle must reproduce every frame in float
bits, rgb8, primary hit ids, ray count and query counters; where oracle/_ref is built, so must the live reference."""
import json
import multiprocessing
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN
from extra_scenes import scene_path
from oracle import oracle_py as O
from oracle import ref_py as R

NPZ = os.path.join(GOLDEN, "balls_high_frames.npz")
FRAMES = np.load(NPZ)
CASES = {n: json.loads(str(FRAMES[n + "/meta"])) for n in sorted({k.split("/")[0] for k in FRAMES.files})}
THREADS = max(1, min(8, os.cpu_count() or 1))


def assert_fixture_frame(r, name, rays):
    assert np.array_equal(r["hit_id"], FRAMES[name + "/hit_id"]), "%s: primary hit ids differ in %d px" % (
        name, int((r["hit_id"] != FRAMES[name + "/hit_id"]).sum()))
    bad = r["rgb32f"].view(np.uint32) != FRAMES[name + "/rgb32f"].view(np.uint32)
    assert not bad.any(), "%s: rgb32f differs in %d values" % (name, int(bad.sum()))
    assert np.array_equal(r["rgb8"], FRAMES[name + "/rgb8"]), name
    assert rays == int(FRAMES[name + "/rays"]), name


def test_fixture_covers_the_scene():
    """The frames are what the issue asked for: the whole sphereflake, its plane, every accel mode."""
    data = open(scene_path("balls_high")).read().split()
    assert data.count("s") == 7381 and data.count("pl") == 1 and data.count("l") == 3
    assert {m["accel"] for m in CASES.values()} == {0, 1, 2}
    assert len(CASES) == 6
    for name, m in CASES.items():
        W, H = m["res"]
        assert FRAMES[name + "/rgb8"].shape == (H, W, 3) and FRAMES[name + "/hit_id"].shape == (H, W)
        hid = FRAMES[name + "/hit_id"]
        assert (hid == 0).any() and (hid > 0).sum() > W * H // 8, name          # the plane (id 0) and many spheres


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_reproduces_the_balls_high_reference_frames(name):
    m = CASES[name]
    sc = O.Scene(scene_path("balls_high"))
    sc.set_resolution(*m["res"])
    r = sc.render(max_depth=m["max_depth"], accel=m["accel"], spp=m["spp"], seed=m["seed"], soft_shadow=m["soft_shadow"],
                  threads=1 if m["spp"] else THREADS)
    assert_fixture_frame(r, name, r["counters"]["rays"])
    assert r["counters"] == m["counters"], name


@pytest.mark.parametrize("name", sorted(CASES))
def test_live_reference_reproduces_the_balls_high_frames(name):
    m = CASES[name]
    if not R.available(m["max_depth"]):
        pytest.skip("oracle/_ref not built (needs the reference tree at build time)")
    sys.path.insert(0, GOLDEN)
    import make_balls_high_golden as G
    if m["spp"]:
        r = G.render_ref(m)
    else:
        # fresh interpreters, not forks of this process, render the strips
        with ProcessPoolExecutor(THREADS, mp_context=multiprocessing.get_context("spawn")) as ex:
            r = G.render_split(m, THREADS, pool=ex)
    assert_fixture_frame(r, name, r["rays"])


def test_grid_mode_differs_from_bvh_mode_on_this_scene():
    """The GRID frame is not the BVH frame (plane outside the grid, missed grid = shadowed): the GRID fixture pins the
    device's grid walk, not a copy of its BVH walk."""
    sc = O.Scene(scene_path("balls_high"))
    sc.set_resolution(128, 128)
    bvh = sc.render(max_depth=4, accel=2, threads=THREADS)
    grid = FRAMES["bh_128_d4_grid/rgb8"]
    none = FRAMES["bh_128_d4_none/rgb8"]
    assert int((grid != bvh["rgb8"]).any(-1).sum()) > 1000
    assert np.array_equal(FRAMES["bh_128_d4_none/hit_id"], bvh["hit_id"])
    assert int((none != bvh["rgb8"]).any(-1).sum()) < 20
