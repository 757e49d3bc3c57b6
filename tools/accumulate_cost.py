#!/usr/bin/env python3
"""What p3d_accumulate costs (profiles/accumulate_cost.txt): a dof sequence of 4 orbit frames at 1920x1080 (soft shadows;
hits and misses) with its planes in device memory, accumulated in one call, and the last frame alone with the third as its
history (the shape of a render-again loop), each timed with p3d_timer_begin / p3d_timer_end over CALLS calls after WARMUP
warm-ups, REPEATS times.  Beside every figure stands the traffic floor at the copy bandwidth measured in the same process
(a device-to-device copy of 1 GiB, bytes read plus bytes written over its time).  Per pixel a frame with history must
read its own colour, depth, normal and hit_id (32 bytes) and the previous frame's colour, depth, normal, length and hit_id
(36), each once, and write colour and length (16); a frame without history reads its colour (12) and writes 16.  The
result is compared with the host restatement, every bit, before anything is timed.
usage: python tools/accumulate_cost.py [CALLS [WARMUP [REPEATS]]]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

from conftest import scene_path  # noqa: E402
import torch  # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P  # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api  # noqa: E402

CALLS, WARMUP, REPEATS = [int(a) for a in sys.argv[1:4]] + [100, 10, 3][len(sys.argv[1:4]):]
W, H, N = 1920, 1080, 4
STEP_DEG = 1.0
PLANES = ("rgb32f", "depth", "normal", "hit_id")


def copy_bandwidth():
    """Bytes read plus bytes written per second of a 1 GiB device-to-device copy: the median of 5 windows of 10 copies."""
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda:0").normal_()
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    rates = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            b.copy_(a)
        e1.record()
        e1.synchronize()
        rates.append(10 * 2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3))
    return float(np.median(rates))


def main():
    print("library: %s" % api.LIB_PATH)
    bw = copy_bandwidth()
    print("copy bandwidth (1 GiB device-to-device, read + written): %.2f TB/s" % (bw / 1e12))
    hs = P.HostScene(scene_path("dof"))
    hs.set_resolution(W, H)
    ds = P.DeviceScene.from_host(hs)
    cams = hs.orbit_cameras(N, STEP_DEG)
    frames = ds.render_aov(cams, max_depth=4, accel=hs.accel, soft_shadow=True)
    kw = dict(depth_tolerance=api.ACCUMULATE_DEPTH_TOLERANCE, normal_min=api.ACCUMULATE_NORMAL_MIN, max_history=api.ACCUMULATE_MAX_HISTORY)
    ref = {ids: api.host_accumulate(frames["rgb32f"], frames["depth"], frames["normal"], cams, frames["hit_id"] if ids else None, **kw)
           for ids in (True, False)}
    hit = frames["hit_id"] >= 0
    print("dof %dx%d, %d orbit frames %g degrees apart, soft shadows, %.1f %% of the pixels hit; tolerance %g, normal_min %g, max_history %g"
          % (W, H, N, STEP_DEG, 100 * hit.mean(), kw["depth_tolerance"], kw["normal_min"], kw["max_history"]))
    print("pixels that took history, frame by frame: %s" % ", ".join("%.1f %%" % (100 * (ref[True]["length"][f] > 1).mean()) for f in range(N)))
    dev = {k: torch.from_numpy(frames[k]).cuda() for k in PLANES}
    px = W * H
    o32 = torch.zeros(N * px * 3, dtype=torch.float32, device="cuda:0")
    ol = torch.zeros(N * px, dtype=torch.float32, device="cuda:0")

    def sequence(ids=True):
        ds.accumulate_device(W, H, cams, *[dev[k].data_ptr() for k in PLANES[:3]], hit_ptr=dev["hit_id"].data_ptr() if ids else 0,
                             out_rgb32f_ptr=o32.data_ptr(), out_length_ptr=ol.data_ptr(), **kw)

    def last_frame():
        # frame 3 alone, looking back at the accumulated frame 2 (o32 / ol hold the whole sequence's result)
        hist = dict(rgb32f=o32.data_ptr() + 2 * px * 12, length=ol.data_ptr() + 2 * px * 4, depth=dev["depth"].data_ptr() + 2 * px * 4,
                    normal=dev["normal"].data_ptr() + 2 * px * 12, hit_id=dev["hit_id"].data_ptr() + 2 * px * 4, cam=cams[2])
        ds.accumulate_device(W, H, cams[3:], dev["rgb32f"].data_ptr() + 3 * px * 12, dev["depth"].data_ptr() + 3 * px * 4,
                             dev["normal"].data_ptr() + 3 * px * 12, hit_ptr=dev["hit_id"].data_ptr() + 3 * px * 4,
                             out_rgb32f_ptr=one32.data_ptr(), out_length_ptr=onel.data_ptr(), history=hist, **kw)

    one32 = torch.zeros(px * 3, dtype=torch.float32, device="cuda:0")
    onel = torch.zeros(px, dtype=torch.float32, device="cuda:0")
    for ids in (True, False):
        sequence(ids)
        ds.sync()
        equal = (np.array_equal(o32.cpu().numpy().view(np.uint32), ref[ids]["rgb32f"].reshape(-1).view(np.uint32))
                 and np.array_equal(ol.cpu().numpy().view(np.uint32), ref[ids]["length"].reshape(-1).view(np.uint32)))
        print("4 frames, hit ids %s: the device == the host restatement in every bit: %s" % (ids, equal))
    sequence(True)
    last_frame()
    ds.sync()
    equal = (np.array_equal(one32.cpu().numpy().view(np.uint32), ref[True]["rgb32f"][3].reshape(-1).view(np.uint32))
             and np.array_equal(onel.cpu().numpy().view(np.uint32), ref[True]["length"][3].reshape(-1).view(np.uint32)))
    print("frame 3 alone with frame 2 as history == frame 3 of the sequence in every bit: %s" % equal)
    with_history, without = 32 + 36 + 16, 12 + 16
    cases = [("4 frames, hit ids           ", lambda: sequence(True), (N - 1) * with_history + without),
             ("4 frames, no hit ids        ", lambda: sequence(False), (N - 1) * (with_history - 8) + without),
             ("1 frame with history        ", last_frame, with_history)]
    for rep in range(REPEATS):
        for name, run, bytes_per_pixel in cases:
            for _ in range(WARMUP):
                run()
            ds.sync()
            ds.timer_begin()
            for _ in range(CALLS):
                run()
            ms = ds.timer_end() / CALLS
            floor = bytes_per_pixel * px / bw * 1e3
            print("  repeat %d  %s %8.4f ms   floor %7.4f ms (%3d bytes per pixel)   ratio %5.2f" % (rep, name, ms, floor, bytes_per_pixel, ms / floor),
                  flush=True)
    ds.close()


if __name__ == "__main__":
    main()
