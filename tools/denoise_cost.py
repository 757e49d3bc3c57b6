#!/usr/bin/env python3
"""What p3d_denoise costs (profiles/denoise_cost.txt): the planes of a dof frame at 1920x1080 (soft shadows; hits and
misses) in device memory, filtered with K passes, one frame and a batch of 4, each timed with p3d_timer_begin /
p3d_timer_end over CALLS calls after WARMUP warm-ups, REPEATS times.  Beside every figure stands the traffic floor: 52
bytes per pixel per pass (40 read, 12 written) at the copy bandwidth measured in the same process (a device-to-device
copy of 1 GiB, bytes read plus bytes written over its time).  The K = 5 result is compared with the host restatement,
every bit, before anything is timed.
usage: python tools/denoise_cost.py [CALLS [WARMUP [REPEATS]]]"""
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
W, H = 1920, 1080


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
    bw = copy_bandwidth()
    print("copy bandwidth (1 GiB device-to-device, read + written): %.2f TB/s" % (bw / 1e12))
    hs = P.HostScene(scene_path("dof"))
    hs.set_resolution(W, H)
    ds = P.DeviceScene.from_host(hs)
    frame = ds.render_aov(hs.camera(), max_depth=4, accel=hs.accel, soft_shadow=True)
    hit = float((frame["hit_id"] >= 0).mean())
    planes = [frame[k] for k in ("rgb32f", "depth", "normal", "albedo")]
    kw = dict(sigma_depth=api.DENOISE_SIGMA_DEPTH, sigma_albedo=api.DENOISE_SIGMA_ALBEDO, sigma_color=api.DENOISE_SIGMA_COLOR,
              normal_power_log2=api.DENOISE_NORMAL_POWER_LOG2)
    ref = api.host_denoise(*planes, iterations=5, **kw)
    print("dof %dx%d, soft shadows, %.1f %% of the pixels hit; sigmas %g %g %g, normal_power_log2 %d; ms per call over %d calls after %d warm-ups"
          % (W, H, 100 * hit, kw["sigma_depth"], kw["sigma_albedo"], kw["sigma_color"], kw["normal_power_log2"], CALLS, WARMUP))
    for n in (1, 4):
        dev = [torch.from_numpy(np.concatenate([p] * n)).cuda() for p in planes]
        o32 = torch.zeros(n * H * W * 3, dtype=torch.float32, device="cuda:0")
        o8 = torch.zeros(n * H * W * 3, dtype=torch.uint8, device="cuda:0")
        run = lambda k: ds.denoise_device(W, H, *[t.data_ptr() for t in dev], out_rgb32f_ptr=o32.data_ptr(), out_rgb8_ptr=o8.data_ptr(),
                                          n_frames=n, iterations=k, **kw)
        run(5)
        ds.sync()
        got = o32.cpu().numpy().reshape(n, H, W, 3)
        equal = all(np.array_equal(got[f].view(np.uint32), ref["rgb32f"][0].view(np.uint32)) for f in range(n))
        print("%d frame(s): K = 5 on the device == the host restatement in every bit: %s" % (n, equal))
        for rep in range(REPEATS):
            for k in (0, 1, 2, 3, 4, 5, 6):
                for _ in range(WARMUP):
                    run(k)
                ds.sync()
                ds.timer_begin()
                for _ in range(CALLS):
                    run(k)
                ms = ds.timer_end() / CALLS
                floor = max(k, 1) * 52 * n * W * H / bw * 1e3 if k else (12 + 12 + 3) * n * W * H / bw * 1e3
                print("  repeat %d  %d frame(s)  K = %d  %8.4f ms   floor %7.4f ms   ratio %5.2f" % (rep, n, k, ms, floor, ms / floor), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
