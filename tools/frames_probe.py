"""ms per frame of p3d_render_frames against one-frame p3d_render calls (host clock around work that ends in a device
synchronise; median and spread of the timed repeats).  One JSON line per scene:
  config 2: mount_low 1920x1080, depth 4, BVH;  config 3: dragon 1920x1080, depth 4.
Every way of rendering runs on a handle of its own, so that each keeps its measured schedule pick and tile order (a
batch's pick and order are keyed on n: one handle alternating n would re-measure at every change):
  frames_n1 / _n4 / _n12   12 orbit frames (+-15 degrees around the file's eye) as batches of n, one handle, one stream;
  render_x12               the same 12 frames as p3d_render calls, one handle;
  bench_4x3                bench.py's method: 4 handles on 4 streams, 3 frames each, all in flight;
  n12_wavefront / n12_tile (--forced) n = 12 batches with the schedule forced, for the pick rule of LDS scenes.
The ways alternate within each repeat.  The last frame of an n = 12 batch whose last camera is the file's own is checked
against the CPU oracle (rgb8 equal).
usage: python tools/frames_probe.py [--repeats 20] [--scenes mount_low,dragon] [--forced]"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

from conftest import scene_path  # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P  # noqa: E402


def orbit_cams(hs, path, n, half_deg=15.0):
    frm = [l for l in open(path).read().splitlines() if l.startswith("from ")][0].split()[1:4]
    x, y, z = (float(v) for v in frm)
    r, a0 = math.hypot(x, y), math.atan2(y, x)
    cams = []
    for k in range(n):
        a = a0 + math.radians(-half_deg + 2 * half_deg * k / max(n - 1, 1))
        hs.set_eye(np.float32(r * math.cos(a)), np.float32(r * math.sin(a)), np.float32(z))
        cams.append(hs.camera())
    return cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--scenes", default="mount_low,dragon")
    ap.add_argument("--forced", action="store_true")
    a = ap.parse_args()
    import torch
    from oracle import oracle_py as O
    for scene in a.scenes.split(","):
        hs = P.HostScene(scene_path(scene))
        hs.set_resolution(1920, 1080)
        file_cam = hs.camera()
        cams = orbit_cams(hs, scene_path(scene), 12)
        kw = dict(max_depth=4, accel=P.ACCEL_BVH)
        bufs = [torch.zeros((12, 1080, 1920, 3), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
        handles = []

        def handle():
            ds = P.DeviceScene.from_host(hs)
            handles.append(ds)
            return ds

        def batch(n, **force):
            ds = handle()

            def run():
                for k in range(0, 12, n):
                    ds.render_frames_device(cams[k:k + n], bufs[0][k].data_ptr(), **kw, **force)
                ds.sync()
            return run

        def singles():
            ds = handle()

            def run():
                for k in range(12):
                    ds.render_device(cams[k], bufs[0][k].data_ptr(), **kw)
                ds.sync()
            return run

        def bench_method():
            streams = [torch.cuda.Stream() for _ in range(4)]
            hds = [handle() for _ in range(4)]
            for ds, st in zip(hds, streams):
                ds.set_stream(st.cuda_stream)

            def run():
                for j in range(3):
                    for i, ds in enumerate(hds):
                        ds.render_device(cams[3 * i + j], bufs[i][3 * i + j].data_ptr(), **kw)
                for ds in hds:
                    ds.sync()
            return run
        runs = {"frames_n1": batch(1), "frames_n4": batch(4), "frames_n12": batch(12), "render_x12": singles(),
                "bench_4x3": bench_method()}
        if a.forced:
            runs["n12_wavefront"] = batch(12, wavefront=True)
            runs["n12_tile"] = batch(12, tile=True)
        for _ in range(16):                                  # each handle's measured pick and tile order settle
            for r in runs.values():
                r()
        times = {k: [] for k in runs}
        for _ in range(a.repeats):                           # alternated
            for k, r in runs.items():
                t0 = time.perf_counter()
                r()
                times[k].append((time.perf_counter() - t0) * 1e3 / 12)
        res = {"scene": scene, "res": [1920, 1080], "depth": 4, "frames": 12, "repeats": a.repeats, "measured": True}
        for k, v in times.items():
            res[k + "_ms_per_frame"] = round(float(np.median(v)), 4)
            res[k + "_spread"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
        if scene == "mount_low":
            ds = handles[2]                                  # the n = 12 handle, last camera = the file's own
            last = ds.render_frames(cams[:11] + [file_cam], **kw)["rgb8"][-1]
            sc = O.Scene(scene_path(scene))
            sc.set_resolution(1920, 1080)
            ref = sc.render(max_depth=4, accel=2, threads=16)["rgb8"]
            res["last_frame_equals_oracle"] = bool(np.array_equal(last, ref))
        print(json.dumps(res), flush=True)
        for ds in handles:
            ds.close()


if __name__ == "__main__":
    main()
