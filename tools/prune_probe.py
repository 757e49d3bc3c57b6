"""Frames of mount_low on the wavefront schedule with p3d_set_prune_reflections off and on, one handle, one stream, one
frame at a time (profiles/prune_reflections.txt): the rays each tree level queued (p3d_last_level_rays), whether the two
frames are equal in every bit, and the time of a frame with nothing else in flight.  Also the program to put behind

  rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU -d DIR --output-format csv -- python3 tools/prune_probe.py --prune 1
  python3 tools/pmc_summary.py OUT.json DIR --kernels wf_

(--prune 0 / 1 renders with that setting only, so that a launch's counters are one setting's).  P3D_NO_PAIR_MODE=1 in the
environment queues the last level's rays singly: its figure is then rays, not pair slots.  One JSON line.
usage: python tools/prune_probe.py [--prune 0|1|both] [--res 1920x1080] [--depth 4] [--frames 20] [--scene mount_low]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

from conftest import scene_path  # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prune", choices=["0", "1", "both"], default="both")
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--scene", default="mount_low")
    a = ap.parse_args()
    import torch
    W, H = (int(v) for v in a.res.split("x"))
    hs = P.HostScene(scene_path(a.scene))
    hs.set_resolution(W, H)
    cam = hs.camera()
    ds = P.DeviceScene.from_host(hs)
    kw = dict(max_depth=a.depth, accel=P.ACCEL_BVH, wavefront=True)
    buf = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    res = {"scene": a.scene, "res": [W, H], "depth": a.depth, "frames": a.frames, "pair_mode": "P3D_NO_PAIR_MODE" not in os.environ}
    frames = {}
    for on in ([0, 1] if a.prune == "both" else [int(a.prune)]):
        ds.set_prune_reflections(on)
        frames[on] = ds.render(cam, **kw)["rgb32f"].view(np.uint32)
        res["level_rays_prune_%d" % on] = [int(v) for v in ds.last_level_rays(a.depth)]
        for _ in range(3):
            ds.render_device(cam, buf.data_ptr(), **kw)
        ds.sync()
        t0 = time.perf_counter()
        for _ in range(a.frames):
            ds.render_device(cam, buf.data_ptr(), **kw)
        ds.sync()
        res["ms_per_frame_one_in_flight_prune_%d" % on] = round((time.perf_counter() - t0) * 1e3 / max(a.frames, 1), 5)
    if len(frames) == 2:
        res["frames_equal_in_every_bit"] = bool(np.array_equal(frames[0], frames[1]))
        res["non_finite_values"] = int((~np.isfinite(frames[0].view(np.float32))).sum())
    print(json.dumps(res), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
