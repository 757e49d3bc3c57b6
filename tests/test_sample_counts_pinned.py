"""Sampled frames (spp x spp jittered samples and the thin lens) at every sample count from 1 to 8, in accel NONE, GRID and
BVH: tests/golden/sample_counts.npz holds REFERENCE output (the reference's own rayTracing() object code,
tests/golden/make_sample_counts_golden.py).  The oracle must reproduce every frame in float bits, rgb8, primary hit ids,
ray count and query counters; where oracle/_ref is built, so must the live reference.

The frames are also restated sample by sample from HostScene.samples -- the array the device reads -- which ties that
array's layout ([y][x][i * spp + j] = pixel x, pixel y, lens x, lens y) and the order of the float sum to the frame, and
the fixture is checked for the properties the device tests rely on: a sum in another order, a missing clamp at 1.0 or a
frame without hits would not go unseen.  tests/test_gpu_sample_counts.py checks the device against the same file."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from extra_scenes import scene_path
from oracle import oracle_py as O
from oracle import ref_py as R
import u_4a_2s_p3d_raytracer_template2_amd as P

FRAMES = np.load(os.path.join(GOLDEN, "sample_counts.npz"))
with open(os.path.join(GOLDEN, "sample_counts.json")) as _f:
    CASES = json.load(_f)
DOF = ["dof_40x24_d4_spp%d" % s for s in (1, 3, 5, 6, 7, 8)]
# name -> scene, (W, H), depth, accel, spp, seed: the table the fixture was asked for
TABLE = dict([(n, ("dof", (40, 24), 4, 2, int(n[-1]), 101)) for n in DOF] + [
    ("bl_40x24_d3_none_spp3", ("balls_low", (40, 24), 3, 0, 3, 102)),
    ("bl_40x24_d3_grid_spp5", ("balls_low", (40, 24), 3, 1, 5, 103)),
    ("ml_33x17_d6_spp3", ("mount_low", (33, 17), 6, 2, 3, 104)),
    ("bh_32x16_d4_spp3", ("balls_high", (32, 16), 4, 2, 3, 105)),
    ("bl_16x160_d3_spp3", ("balls_low", (16, 160), 3, 2, 3, 106)),
])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_fixture_frame(r, name, rays):
    assert np.array_equal(r["hit_id"], FRAMES[name + "/hit_id"]), "%s: primary hit ids differ in %d px" % (
        name, int((r["hit_id"] != FRAMES[name + "/hit_id"]).sum()))
    bad = bits(r["rgb32f"]) != bits(FRAMES[name + "/rgb32f"])
    assert not bad.any(), "%s: rgb32f differs in %d values" % (name, int(bad.sum()))
    assert np.array_equal(r["rgb8"], FRAMES[name + "/rgb8"]), name
    assert rays == int(FRAMES[name + "/rays"]) == CASES[name]["rays"], name


def test_fixture_holds_the_cases_asked_for():
    assert sorted(CASES) == sorted(TABLE)
    assert sorted({k.split("/")[0] for k in FRAMES.files}) == sorted(TABLE)
    for name, (scene, res, depth, accel, spp, seed) in TABLE.items():
        m = CASES[name]
        assert (m["scene"], tuple(m["res"]), m["max_depth"], m["accel"], m["spp"], m["seed"], m["soft_shadow"]) == (
            scene, res, depth, accel, spp, seed, False), name
        W, H = res
        assert FRAMES[name + "/rgb8"].shape == (H, W, 3) and FRAMES[name + "/rgb32f"].shape == (H, W, 3), name
        assert FRAMES[name + "/hit_id"].shape == (H, W), name
        # ragged against the 16x16 tile, but for the banded frame (whole tile rows on purpose) and the 32x16 of balls_high
        assert (W % 16 or H % 16) or name in ("bl_16x160_d3_spp3", "bh_32x16_d4_spp3"), name
    assert {m["spp"] for m in CASES.values()} == {1, 3, 5, 6, 7, 8}
    assert {m["accel"] for m in CASES.values()} == {0, 1, 2}
    with open(scene_path("dof")) as f:
        assert "aperture 12" in f.read().splitlines()
    assert P.HostScene(scene_path("dof")).camera().aperture > 0.1        # the lens pair of a sample moves the ray
    assert os.path.getsize(os.path.join(GOLDEN, "sample_counts.npz")) < 256 * 1024


@pytest.mark.parametrize("name", sorted(TABLE))
def test_oracle_reproduces_the_reference_frames(name):
    m = CASES[name]
    sc = O.Scene(scene_path(m["scene"]))
    sc.set_resolution(*m["res"])
    r = sc.render(max_depth=m["max_depth"], accel=m["accel"], spp=m["spp"], seed=m["seed"], soft_shadow=m["soft_shadow"], threads=1)
    assert_fixture_frame(r, name, r["counters"]["rays"])
    assert r["counters"] == m["counters"], name


@pytest.mark.parametrize("name", sorted(TABLE))
def test_live_reference_reproduces_the_frames(name):
    m = CASES[name]
    if not R.available(m["max_depth"]):
        pytest.skip("oracle/_ref not built (needs the reference tree at build time)")
    sys.path.insert(0, GOLDEN)
    import make_sample_counts_golden as G
    assert G.CASES[name] == {k: m[k] for k in G.CASES[name]}, "the script's table and sample_counts.json differ"
    r = G.render_ref(m)
    assert_fixture_frame(r, name, r["rays"])


# ---- the frame restated sample by sample, from the array the device reads

_per_sample = {}


def primary_hit(osc, accel, o, d, prims):
    """Scene index of the nearest hit of one primary ray, -1 on a miss.  GRID mode asks the restated grid.  NONE is
    rayTracing()'s own loop over the restated intersectors: the first primitive with the strictly smallest t.  BVH mode
    ends in that loop too in the reference (its switch falls through), planes included, which the tree does
    not hold.  Scenes of up to 256 primitives run the loop as it is; mount_low and balls_high, with thousands, run it
    over the restated BVH's answer and the planes."""
    if accel == 1:
        ok, obj, _ = osc.refgrid_closest(o, d)
        return obj if ok else -1
    among = range(len(prims[0]))
    if accel == 2 and len(prims[0]) > 256:
        ok, obj, _ = osc.refbvh_closest(o, d)
        among = sorted(set([obj] if ok and obj >= 0 else []) | set(int(i) for i in np.flatnonzero(prims[0] == O.PLANE)))
    best, best_t = -1, np.float32(np.finfo(np.float32).max)
    for i in among:
        h, t, _ = O.intersect(prims[0][i], prims[1][i], o, d)
        if h and np.float32(t) < best_t:
            best, best_t = i, np.float32(t)
    return best


def per_sample(name):
    """(colour of every sample, clamped to [0, 1], as (H, W, ns, 3) float32; hit id of sample 0 as (H, W)), once per case."""
    if name not in _per_sample:
        m = CASES[name]
        W, H = m["res"]
        hs = P.HostScene(scene_path(m["scene"]))
        hs.set_resolution(W, H)
        samples = hs.samples(m["seed"], m["spp"])
        ns = m["spp"] ** 2
        assert samples.shape == (H, W, ns, 4)
        osc = O.Scene(scene_path(m["scene"]))
        osc.set_resolution(W, H)
        prims = osc.prims()
        col = np.zeros((H, W, ns, 3), np.float32)
        hid = np.full((H, W), -2, np.int32)
        for y in range(H):
            for x in range(W):
                for s in range(ns):
                    px, py, lx, ly = samples[y, x, s]
                    o, d = osc.primary_ray_lens(lx, ly, px, py)
                    col[y, x, s] = osc.trace(m["accel"], o, d, m["max_depth"])
                    if s == 0:
                        hid[y, x] = primary_hit(osc, m["accel"], o, d, prims)
        col = np.minimum(np.maximum(col, np.float32(0)), np.float32(1))
        col.setflags(write=False)
        _per_sample[name] = (col, hid)
    return _per_sample[name]


def summed(col, order):
    """color = color + sample in `order`, in float32 from zero, then color / (4 * 4) whatever spp is."""
    acc = np.zeros(col.shape[:2] + (3,), np.float32)
    for s in order:
        acc = acc + col[:, :, s]
    assert acc.dtype == np.float32
    return acc / np.float32(16)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_frame_is_the_sum_of_its_samples_in_index_order(name):
    m = CASES[name]
    col, hid = per_sample(name)
    ns = m["spp"] ** 2
    got = summed(col, range(ns))
    bad = (bits(got) != bits(FRAMES[name + "/rgb32f"])).any(-1)
    assert not bad.any(), "%s: %d px differ from the sum of HostScene.samples' rays, first at %s" % (
        name, int(bad.sum()), np.argwhere(bad)[:1].tolist())
    assert np.array_equal(hid, FRAMES[name + "/hit_id"]), "%s: the hit id is not sample 0's in %d px" % (
        name, int((hid != FRAMES[name + "/hit_id"]).sum()))


# ---- the fixture keeps the properties the device tests need

@pytest.mark.parametrize("name", sorted(n for n in TABLE if CASES[n]["spp"] ** 2 >= 9))
def test_a_sum_in_reverse_order_is_another_frame(name):
    """A device that adds the samples in another order than the reference must not be able to pass: the same clamped
    colours added last sample first change the bits of at least a tenth of the pixels."""
    col, _ = per_sample(name)
    ns = CASES[name]["spp"] ** 2
    fwd, rev = summed(col, range(ns)), summed(col, reversed(range(ns)))
    share = float((bits(fwd) != bits(rev)).any(-1).mean())
    print("%s: reverse-order sum changes %.1f %% of the pixels" % (name, 100 * share))
    assert share >= 0.10, "%s: only %.1f %% of the pixels depend on the order of the sum" % (name, 100 * share)


@pytest.mark.parametrize("name", [n for n in DOF if int(n[-1]) >= 5])
def test_saturated_and_unsaturated_channels(name):
    """From ns > 16 the reference's / (4 * 4) leaves sums above 1.0, which u8fromfloat must saturate: both kinds show."""
    f = FRAMES[name + "/rgb32f"]
    high = float((f >= 1.0).mean())
    print("%s: %.1f %% of the channels are >= 1.0" % (name, 100 * high))
    assert high >= 0.15 and 1.0 - high >= 0.15, (name, high)
    assert (FRAMES[name + "/rgb8"][f >= 1.0] == 255).all()
    assert float(f.max()) <= CASES[name]["spp"] ** 2 / 16.0


@pytest.mark.parametrize("name", DOF + ["ml_33x17_d6_spp3"])
def test_hits_and_misses(name):
    hid = FRAMES[name + "/hit_id"]
    assert ((hid >= 0) | (hid == -1)).all()
    hit = float((hid >= 0).mean())
    assert hit >= 0.10 and 1.0 - hit >= 0.10, (name, hit)
