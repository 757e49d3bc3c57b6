"""Frames of config 2 (mount_low 1920x1080, depth 4, BVH) seen through the file's camera or through one turned away from
the scene so that every tile is sky, for counters of the level-1 launch (profiles/sky_tiles.txt):

  rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU -d DIR --output-format csv -- python3 tools/sky_tiles_probe.py --camera sky
  python3 tools/pmc_summary.py OUT.json DIR --kernels wf_primary

One handle, one stream, one frame at a time: a launch's counters do not depend on what runs next to it.  The first frame
goes to host planes and says what the camera sees (pixels and 16x16 tiles with a primary hit); the timed ones go to a
device plane as bench.py's do.  One JSON line.
usage: python tools/sky_tiles_probe.py [--camera scene|sky] [--frames 20] [--scene mount_low] [--res 1920x1080]
                                       [--sky-tiles 0|1] [--primary-tiles N]"""
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


def turned_away(cam):
    """The same eye looking the opposite way: n and u negated (v kept, so the frame stays right-handed)."""
    for a in range(3):
        cam.n[a] = -cam.n[a]
        cam.u[a] = -cam.u[a]
    return cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--camera", choices=["scene", "sky"], default="scene")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--scene", default="mount_low")
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--sky-tiles", type=int, default=-1, help="p3d_set_sky_tiles (default: the library's)")
    ap.add_argument("--primary-tiles", type=int, default=0)
    a = ap.parse_args()
    import torch
    W, H = (int(v) for v in a.res.split("x"))
    hs = P.HostScene(scene_path(a.scene))
    hs.set_resolution(W, H)
    cam = hs.camera()
    if a.camera == "sky":
        cam = turned_away(cam)
    ds = P.DeviceScene.from_host(hs)
    if a.primary_tiles:
        ds.set_primary_tiles(a.primary_tiles)
    if a.sky_tiles >= 0:
        ds.set_sky_tiles(a.sky_tiles)
    kw = dict(max_depth=4, accel=P.ACCEL_BVH)
    hit = ds.render(cam, want_f32=False, **kw)["hit_id"] >= 0
    th, tw = (H + 15) // 16, (W + 15) // 16
    pad = np.zeros((th * 16, tw * 16), bool)
    pad[:H, :W] = hit
    hit_tiles = int(pad.reshape(th, 16, tw, 16).any(axis=(1, 3)).sum())
    buf = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    for _ in range(3):
        ds.render_device(cam, buf.data_ptr(), **kw)
    ds.sync()
    t0 = time.perf_counter()
    for _ in range(a.frames):
        ds.render_device(cam, buf.data_ptr(), **kw)
    ds.sync()
    ms = (time.perf_counter() - t0) * 1e3 / max(a.frames, 1)
    res = {"scene": a.scene, "res": [W, H], "camera": a.camera, "frames": a.frames, "hit_pixels": int(hit.sum()),
           "hit_pixel_share": round(float(hit.mean()), 4), "tiles_16x16": th * tw, "tiles_with_a_hit": hit_tiles,
           "primary_tiles": ds.last_primary_tiles(), "schedule": ds.last_schedule(), "ms_per_frame_one_in_flight": round(ms, 5)}
    if hasattr(ds, "last_sky_tiles"):
        used, empty = ds.last_sky_tiles()
        res["sky_tiles_used"], res["sky_tiles_empty"] = used, empty
    print(json.dumps(res), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
