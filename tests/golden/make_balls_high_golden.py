#!/usr/bin/env python3
"""Generate tests/golden/balls_high_frames.npz: frames of the reference's OWN object code (oracle/_ref) on balls_high.p3f,
the level-4 sphereflake the reference ships (7 381 spheres, one plane, three lights, Ks 0.5 on every sphere).

Run where oracle/_ref is built (oracle/Makefile builds it when the reference tree is present):
    python tests/golden/make_balls_high_golden.py
Every frame is rendered by the reference's rayTracing() through oracle/ref_py.py; the script asserts that the oracle
restatement reproduces it bit for bit (rgb8, rgb32f bits, primary hit ids, ray count) and takes the per-kind query
counters, which the reference does not keep, from the oracle.  Frames without samples (spp == 0) are pure functions of
the pixel, so their rows are split over worker processes; the sampled case draws the reference's serial rand() stream
and is rendered in one piece.

balls_high_frames.npz   per case "<name>/rgb8" [H,W,3] u8 (bottom row first), "/rgb32f" [H,W,3] f32, "/hit_id" [H,W] i32,
                        "/rays" (Ray::nextId delta); case parameters and the oracle's counters in "<name>/meta" (json).
"""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from extra_scenes import scene_path  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from oracle import ref_py as R  # noqa: E402

OUT = os.path.join(HERE, "balls_high_frames.npz")
SCENE = "balls_high"

# name -> (W, H), accel, spp, max_depth, seed, soft_shadow
CASES = {
    # ragged against the 16x16 and 16x4 tiles
    "bh_200x150_d4_bvh": dict(res=[200, 150], accel=2, spp=0, max_depth=4, seed=0, soft_shadow=False),
    "bh_128_d4_none": dict(res=[128, 128], accel=0, spp=0, max_depth=4, seed=0, soft_shadow=False),
    # GRID mode: 39^3 cells, the plane outside the grid, shadow rays that miss the grid count as shadowed
    "bh_128_d4_grid": dict(res=[128, 128], accel=1, spp=0, max_depth=4, seed=0, soft_shadow=False),
    # the deepest reflection chains the reference harness is built for
    "bh_96_d6_bvh": dict(res=[96, 96], accel=2, spp=0, max_depth=6, seed=0, soft_shadow=False),
    # the reference's SOFT_SHADOW global at spp 0: 16 deterministic sub-lights per light
    "bh_96x64_d4_bvh_soft": dict(res=[96, 64], accel=2, spp=0, max_depth=4, seed=0, soft_shadow=True),
    # 2x2 jittered samples from the serial rand() stream
    "bh_64_d4_spp2": dict(res=[64, 64], accel=2, spp=2, max_depth=4, seed=24680, soft_shadow=False),
}


def render_ref(m, y0=0, y1=0):
    """The reference's frame of case m (rows [y0, y1) when y1 > 0)."""
    sc = O.Scene(scene_path(SCENE))
    sc.set_resolution(*m["res"])
    rs = R.RefScene.from_oracle_scene(sc, scene_path(SCENE), res=tuple(m["res"]), depth=m["max_depth"])
    try:
        return rs.render(m["accel"], m["spp"], m["seed"], soft_shadow=m["soft_shadow"], y0=y0, y1=y1)
    finally:
        rs.close()


def strip(args):
    """(y0, y1, rows [y0, y1) of the reference's frame of case m with their ray count): one worker's share."""
    m, y0, y1 = args
    r = render_ref(m, y0, y1)
    return y0, y1, {"rgb8": r["rgb8"][y0:y1], "rgb32f": r["rgb32f"][y0:y1], "hit_id": r["hit_id"][y0:y1], "rays": r["rays"]}


def render_split(m, workers, pool=None):
    """A whole frame of the reference, its rows split over `workers` processes (spp == 0 only: no random draws)."""
    W, H = m["res"]
    if m["spp"] or workers <= 1:
        return render_ref(m)
    step = max(1, (H + 4 * workers - 1) // (4 * workers))
    rgb8 = np.zeros((H, W, 3), np.uint8)
    f32 = np.zeros((H, W, 3), np.float32)
    hid = np.full((H, W), -2, np.int32)
    rays = 0
    own = pool is None
    ex = ProcessPoolExecutor(workers) if own else pool
    try:
        for y0, y1, r in ex.map(strip, [(m, y, min(H, y + step)) for y in range(0, H, step)]):
            rgb8[y0:y1] = r["rgb8"]
            f32[y0:y1] = r["rgb32f"]
            hid[y0:y1] = r["hit_id"]
            rays += r["rays"]
    finally:
        if own:
            ex.shutdown()
    return {"rgb8": rgb8, "rgb32f": f32, "hit_id": hid, "rays": rays}


def render_oracle(m, threads):
    sc = O.Scene(scene_path(SCENE))
    sc.set_resolution(*m["res"])
    return sc.render(max_depth=m["max_depth"], accel=m["accel"], spp=m["spp"], seed=m["seed"],
                     soft_shadow=m["soft_shadow"], threads=1 if m["spp"] else threads)


def main():
    for d in sorted({m["max_depth"] for m in CASES.values()}):
        assert R.available(d), "oracle/_ref is not built for depth %d" % d
    workers = min(16, os.cpu_count() or 1)
    out = {}
    for name, m in CASES.items():
        ref = render_split(m, workers)
        assert (ref["hit_id"] != -2).all(), name
        r = render_oracle(m, workers)
        for k in ("rgb8", "hit_id"):
            assert np.array_equal(ref[k], r[k]), (name, k)
        assert np.array_equal(ref["rgb32f"].view(np.uint32), r["rgb32f"].view(np.uint32)), name
        assert ref["rays"] == r["counters"]["rays"], name
        for k in ("rgb8", "rgb32f", "hit_id"):
            out[name + "/" + k] = ref[k]
        out[name + "/rays"] = np.array(ref["rays"], np.uint64)
        meta = dict(m, scene=SCENE, counters={k: int(v) for k, v in r["counters"].items()})
        out[name + "/meta"] = np.array(json.dumps(meta, sort_keys=True))
        print(name, ref["rays"], "rays", flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
