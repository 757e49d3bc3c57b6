#!/usr/bin/env python3
"""Generate tests/golden/sample_counts.npz and sample_counts.json: sampled frames (spp > 0: spp x spp jittered samples and
the thin lens) of the reference's OWN object code (oracle/_ref) at every sample count from 1 to 8 and in all three accel
modes.

Run where oracle/_ref is built (oracle/Makefile builds it when the reference tree is present):
    python tests/golden/make_sample_counts_golden.py
Every frame is rendered by the reference's rayTracing() through oracle/ref_py.py in one piece (the samples come from the
reference's serial rand() stream); the script asserts that the oracle restatement reproduces it bit for bit (rgb8,
rgb32f bits, primary hit ids, ray count) and takes the per-kind query counters, which the reference does not keep, from
the oracle.  Recorded outputs only.

sample_counts.npz    per case "<name>/rgb8" [H,W,3] u8 (bottom row first), "/rgb32f" [H,W,3] f32, "/hit_id" [H,W] i32 (the
                     primary hit of sample 0), "/rays" (Ray::nextId delta)
sample_counts.json   {name: case parameters, "rays", and the oracle's "counters"}
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from extra_scenes import scene_path  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from oracle import ref_py as R  # noqa: E402

OUT = os.path.join(HERE, "sample_counts.npz")
OUT_JSON = os.path.join(HERE, "sample_counts.json")


def case(scene, res, max_depth, accel, spp, seed):
    return dict(scene=scene, res=list(res), max_depth=max_depth, accel=accel, spp=spp, seed=seed, soft_shadow=False)


# Most resolutions are ragged against the 16x16 tile; the last one is cut into bands of whole tile rows.  ns = spp * spp = 1 is the only sampled frame with one lane stream; 9, 25 and 49 load four lanes unevenly;
# from ns > 16 the reference's color / (4 * 4) passes 1.0.
CASES = {}
for _spp in (1, 3, 5, 6, 7, 8):
    # dof.p3f: aperture 12, so the lens pair of every sample moves the ray
    CASES["dof_40x24_d4_spp%d" % _spp] = case("dof", (40, 24), 4, 2, _spp, 101)
CASES["bl_40x24_d3_none_spp3"] = case("balls_low", (40, 24), 3, 0, 3, 102)
CASES["bl_40x24_d3_grid_spp5"] = case("balls_low", (40, 24), 3, 1, 5, 103)
CASES["ml_33x17_d6_spp3"] = case("mount_low", (33, 17), 6, 2, 3, 104)
# balls_high is read from HBM on the device without a flag asking for it
CASES["bh_32x16_d4_spp3"] = case("balls_high", (32, 16), 4, 2, 3, 105)
# one 16x16 tile wide, ten tile rows tall: bands x samples
CASES["bl_16x160_d3_spp3"] = case("balls_low", (16, 160), 3, 2, 3, 106)


def render_ref(m):
    """The reference's frame of case m."""
    sc = O.Scene(scene_path(m["scene"]))
    sc.set_resolution(*m["res"])
    rs = R.RefScene.from_oracle_scene(sc, scene_path(m["scene"]), res=tuple(m["res"]), depth=m["max_depth"])
    try:
        return rs.render(m["accel"], m["spp"], m["seed"], soft_shadow=m["soft_shadow"])
    finally:
        rs.close()


def render_oracle(m):
    sc = O.Scene(scene_path(m["scene"]))
    sc.set_resolution(*m["res"])
    return sc.render(max_depth=m["max_depth"], accel=m["accel"], spp=m["spp"], seed=m["seed"], soft_shadow=m["soft_shadow"],
                     threads=1)


def main():
    for d in sorted({m["max_depth"] for m in CASES.values()}):
        assert R.available(d), "oracle/_ref is not built for depth %d" % d
    out, names = {}, {}
    for name, m in CASES.items():
        ref = render_ref(m)
        assert (ref["hit_id"] != -2).all(), name
        r = render_oracle(m)
        for k in ("rgb8", "hit_id"):
            assert np.array_equal(ref[k], r[k]), (name, k)
        assert np.array_equal(ref["rgb32f"].view(np.uint32), r["rgb32f"].view(np.uint32)), name
        assert ref["rays"] == r["counters"]["rays"], name
        for k in ("rgb8", "rgb32f", "hit_id"):
            out[name + "/" + k] = ref[k]
        out[name + "/rays"] = np.array(ref["rays"], np.uint64)
        names[name] = dict(m, rays=int(ref["rays"]), counters={k: int(v) for k, v in r["counters"].items()})
        print(name, ref["rays"], "rays", flush=True)
    np.savez_compressed(OUT, **out)
    with open(OUT_JSON, "w") as f:
        json.dump(names, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
