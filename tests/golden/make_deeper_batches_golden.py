#!/usr/bin/env python3
"""Generate tests/golden/deeper_batches_schlick.npz: the scene of tests/test_gpu_deeper_batches.py at 128 x 128, depth 4,
rendered by the reference's OWN object code (oracle/_ref) with its SCHLICK_APPROX switch on, as make_schlick_golden.py does
for the shipped scenes.  The CPU oracle restatement has no Schlick branch, so this frame comes from the reference only.

Run in the build container (needs oracle/_ref):
    python tests/golden/make_deeper_batches_golden.py

deeper_batches_schlick.npz   "rgb8" [H,W,3] u8 (bottom row first), "rgb32f" [H,W,3] f32, "hit_id" [H,W] i32, "rays"
                             (Ray::nextId delta), "scene" (the .p3f text the frame was rendered from).
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import oracle_py as O  # noqa: E402
from oracle import ref_py as R  # noqa: E402

OUT = os.path.join(HERE, "deeper_batches_schlick.npz")
RES, DEPTH = (128, 128), 4


def scene_text():
    """SCENE of tests/test_gpu_deeper_batches.py, read from the file's text: importing the module needs the GPU library."""
    src = open(os.path.join(REPO, "tests", "test_gpu_deeper_batches.py")).read()
    return src.split('SCENE = """', 1)[1].split('"""', 1)[0]


def main():
    assert R.available(DEPTH), "oracle/_ref is not built"
    text = scene_text()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "glass.p3f")
        with open(path, "w") as f:
            f.write(text)
        sc = O.Scene(path)
        sc.set_resolution(*RES)
        plain = sc.render(max_depth=DEPTH, accel=2)
        flag = C.c_bool.in_dll(R.lib(DEPTH), "SCHLICK_APPROX")
        rs = R.RefScene.from_oracle_scene(sc, path, res=RES, depth=DEPTH)
        try:
            off = rs.render(2, 0, 0)
            flag.value = True
            r = rs.render(2, 0, 0)
        finally:
            flag.value = False
            rs.close()
    # the reference without the switch is the oracle's frame; with it, another frame
    assert np.array_equal(off["rgb32f"].view(np.uint32), plain["rgb32f"].view(np.uint32)) and off["rays"] == plain["counters"]["rays"]
    assert not np.array_equal(r["rgb32f"].view(np.uint32), off["rgb32f"].view(np.uint32))
    assert (r["hit_id"] == 0).all() and np.isfinite(r["rgb32f"]).all()
    np.savez_compressed(OUT, rgb8=r["rgb8"], rgb32f=r["rgb32f"], hit_id=r["hit_id"], rays=np.array(r["rays"], np.uint64),
                        scene=np.array(text))
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", r["rays"], "rays")


if __name__ == "__main__":
    main()
