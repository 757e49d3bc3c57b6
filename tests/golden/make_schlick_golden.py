#!/usr/bin/env python3
"""Generate tests/golden/schlick_frames.npz: frames of the reference's OWN object code (oracle/_ref) with its
SCHLICK_APPROX switch on (RT/main.cpp:99, :699-702, :710).

Run in the build container (needs oracle/_ref, i.e. /root/reference at build time):
    python tests/golden/make_schlick_golden.py
The reference global is set through ctypes (c_bool.in_dll(ref_py.lib(depth), "SCHLICK_APPROX")) around each render and
reset in a `finally`.  Frames without samples (spp == 0) are pure functions of the pixel, so their rows are split over
worker processes (the harness renders rows [y0, y1)); the sampled case draws the reference's serial rand() stream and
is rendered in one piece.  The CPU oracle restatement has no Schlick branch: these frames come from the reference only.

schlick_frames.npz   per case "<name>/rgb8" [H,W,3] u8 (bottom row first), "/rgb32f" [H,W,3] f32, "/hit_id" [H,W] i32,
                     "/rays" (Ray::nextId delta); case parameters in "<name>/meta" (json).
"""
import ctypes as C
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from conftest import scene_path  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from oracle import ref_py as R  # noqa: E402

OUT = os.path.join(HERE, "schlick_frames.npz")

# name -> scene, (W, H), accel, spp, max_depth, seed, soft_shadow
CASES = {
    "ml_320x180_d4_bvh": dict(scene="mount_low", res=[320, 180], accel=2, spp=0, max_depth=4, seed=0, soft_shadow=False),
    "ml_320x180_d4_grid": dict(scene="mount_low", res=[320, 180], accel=1, spp=0, max_depth=4, seed=0, soft_shadow=False),
    "ml_160x90_d2_bvh": dict(scene="mount_low", res=[160, 90], accel=2, spp=0, max_depth=2, seed=0, soft_shadow=False),
    "ml_160x90_d4_bvh_soft": dict(scene="mount_low", res=[160, 90], accel=2, spp=0, max_depth=4, seed=0, soft_shadow=True),
    # BASELINE config 4's shape: depth 6, 2x2 jittered samples + thin lens
    "ml_128x72_d6_spp2": dict(scene="mount_low", res=[128, 72], accel=2, spp=2, max_depth=6, seed=12345, soft_shadow=False),
    "mh_160x90_d4_bvh": dict(scene="mount_high", res=[160, 90], accel=2, spp=0, max_depth=4, seed=0, soft_shadow=False),
    # read from HBM on the device (too large for the LDS copy)
    "dragon_160x90_d4_bvh": dict(scene="dragon", res=[160, 90], accel=2, spp=0, max_depth=4, seed=0, soft_shadow=False),
}


def render_ref(m, y0=0, y1=0, schlick=True):
    """The reference's frame of case m (rows [y0, y1) when y1 > 0), SCHLICK_APPROX = schlick during the call."""
    depth = m["max_depth"]
    flag = C.c_bool.in_dll(R.lib(depth), "SCHLICK_APPROX")
    sc = O.Scene(scene_path(m["scene"]))
    sc.set_resolution(*m["res"])
    rs = R.RefScene.from_oracle_scene(sc, scene_path(m["scene"]), res=tuple(m["res"]), depth=depth)
    flag.value = schlick
    try:
        return rs.render(m["accel"], m["spp"], m["seed"], soft_shadow=m["soft_shadow"], y0=y0, y1=y1)
    finally:
        flag.value = False
        rs.close()


def strip(args):
    """(y0, y1, rows [y0, y1) of the reference's frame of case m with their ray count): one worker's share."""
    m, y0, y1 = args
    r = render_ref(m, y0, y1)
    return y0, y1, {"rgb8": r["rgb8"][y0:y1], "rgb32f": r["rgb32f"][y0:y1], "hit_id": r["hit_id"][y0:y1], "rays": r["rays"]}


def render_split(m, workers):
    """A whole frame, its rows split over `workers` processes (spp == 0 only: no random draws)."""
    W, H = m["res"]
    if m["spp"] or workers <= 1:
        return render_ref(m)
    step = (H + workers - 1) // workers
    rgb8 = np.zeros((H, W, 3), np.uint8)
    f32 = np.zeros((H, W, 3), np.float32)
    hid = np.full((H, W), -2, np.int32)
    rays = 0
    with ProcessPoolExecutor(workers) as ex:
        for y0, y1, r in ex.map(strip, [(m, y, min(H, y + step)) for y in range(0, H, step)]):
            rgb8[y0:y1] = r["rgb8"]
            f32[y0:y1] = r["rgb32f"]
            hid[y0:y1] = r["hit_id"]
            rays += r["rays"]
    return {"rgb8": rgb8, "rgb32f": f32, "hit_id": hid, "rays": rays}


def main():
    assert R.available(), "oracle/_ref is not built"
    workers = min(16, os.cpu_count() or 1)
    out = {}
    for name, m in CASES.items():
        r = render_split(m, workers)
        assert (r["hit_id"] != -2).all(), name
        for k in ("rgb8", "rgb32f", "hit_id"):
            out[name + "/" + k] = r[k]
        out[name + "/rays"] = np.array(r["rays"], np.uint64)
        out[name + "/meta"] = np.array(json.dumps(m))
        print(name, r["rays"], "rays", flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
