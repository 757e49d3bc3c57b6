#!/usr/bin/env python3
"""What p3d_ambient_occlusion costs (profiles/ao_cost.txt): mount_low (served from LDS) and dragon (read from HBM) at
1920x1080, accel BVH, 4 and 16 samples per pixel, planes in device memory, one process.  Timed with p3d_timer_begin /
p3d_timer_end over CALLS calls after WARMUP warm-ups; the cases alternate REPEATS times and each figure is the median.
  (a) the fused entry.
  (b) the unfused pipeline on the device, which the library could already run: the segments written to memory, p3d_occluded
      on them, a counting pass.  The segments of the pixels that have a query are made once by the host restatement
      (api.host_ao_segments) and uploaded; what stands in for the kernel that would write them is a device-to-device copy of
      the two arrays (24 bytes read and 24 written per segment: such a kernel's traffic, none of its arithmetic), and the
      counting pass is one reduction over the answers.  Both flatter (b), not (a); the host round trip is not timed at all.
  (c) p3d_occluded alone on the materialised segments.
Pixels without a query have no segment in (b) and (c): the unfused pipeline gets that compaction for free.
Before anything is timed the fused result is compared, every bit, with the restatement's resolve of p3d_occluded's answers.
With P3D_LIB naming a library built with the other lane mapping (make -C csrc ao_lane_per_pixel) and --fused-only, only (a)
is checked and timed: the two mappings are measured by running the tool twice in one session.
usage: python tools/ao_cost.py [--fused-only] [CALLS [WARMUP [REPEATS]]]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

from extra_scenes import scene_path  # noqa: E402
import torch  # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P  # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api  # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
FUSED_ONLY = "--fused-only" in sys.argv[1:]
CALLS, WARMUP, REPEATS = [int(a) for a in ARGS[:3]] + [20, 3, 3][len(ARGS[:3]):]
W, H = 1920, 1080
RADIUS, BIAS, SEED = api.AO_RADIUS, api.AO_BIAS, 1


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


def timed(ds, run):
    for _ in range(WARMUP):
        run()
    ds.sync()
    ds.timer_begin()
    for _ in range(CALLS):
        run()
    return ds.timer_end() / CALLS


def measure(name, samples, bw):
    hs = P.HostScene(scene_path(name))
    hs.set_resolution(W, H)
    ds = P.DeviceScene.from_host(hs)
    cam = hs.camera()
    f = ds.render_aov(cam, max_depth=1, accel=P.ACCEL_BVH)
    depth, normal = f["depth"][0], f["normal"][0]
    dev = {k: torch.from_numpy(np.ascontiguousarray(f[k][0])).cuda() for k in ("depth", "normal")}
    ao = torch.zeros(H * W, dtype=torch.float32, device="cuda:0")
    fused = lambda: ds.ambient_occlusion_device(cam, dev["depth"].data_ptr(), dev["normal"].data_ptr(), out_ao_ptr=ao.data_ptr(),
                                                samples=samples, radius=RADIUS, bias=BIAS, seed=SEED, accel=P.ACCEL_BVH)
    o, d, valid = api.host_ao_segments(cam, depth, normal, samples=samples, radius=RADIUS, bias=BIAS, seed=SEED)
    m = valid.astype(bool)
    o, d = np.ascontiguousarray(o[m].reshape(-1, 3)), np.ascontiguousarray(d[m].reshape(-1, 3))
    n = len(o)
    src_o, src_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    seg_o, seg_d = torch.empty_like(src_o), torch.empty_like(src_d)
    ans = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    cnt = torch.zeros(n // samples, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.Stream()
    ds.set_stream(stream.cuda_stream)                       # one stream for the library's launches and the tool's
    with torch.cuda.stream(stream):
        occluded = lambda: ds.occluded_device(n, seg_o.data_ptr(), seg_d.data_ptr(), ans.data_ptr(), accel=P.ACCEL_BVH)

        def unfused():
            seg_o.copy_(src_o); seg_d.copy_(src_d)
            occluded()
            torch.sum(ans.view(-1, samples), dim=1, dtype=torch.int32, out=cnt)

        unfused()
        fused()
        ds.sync()
        full = np.zeros((H, W), np.int32)
        full[m] = cnt.cpu().numpy()
        ref = api.host_ao_resolve(full, samples)["ao"]
        got = ao.cpu().numpy().reshape(H, W)
        equal = np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        print("%s S=%d: %.1f %% of the pixels have a query, %d segments, %.1f %% of them occluded; fused == resolve(p3d_occluded(host segments)) in every bit: %s"
              % (name, samples, 100 * m.mean(), n, 100.0 * float(ans.float().mean()), equal), flush=True)
        assert equal
        cases = [("(a) fused", fused)] + ([] if FUSED_ONLY else [("(b) unfused", unfused), ("(c) p3d_occluded", occluded)])
        ms = {k: [] for k, _ in cases}
        for rep in range(REPEATS):
            for k, run in cases:
                ms[k].append(timed(ds, run))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k, _ in cases:
            print("  %-10s S=%-2d %-18s %8.4f ms  (%s)" % (name, samples, k, med[k], " ".join("%.4f" % v for v in ms[k])))
        floor_a = H * W * 20 / bw * 1e3
        print("  %-10s S=%-2d traffic of (a): 16 bytes read + 4 written per pixel = %.4f ms at the copy bandwidth" % (name, samples, floor_a))
        if not FUSED_ONLY:
            print("  %-10s S=%-2d (a) / (b) = %.3f   (a) / (c) = %.3f   segment records of (b): %.0f MB + %.0f MB of answers"
                  % (name, samples, med["(a) fused"] / med["(b) unfused"], med["(a) fused"] / med["(c) p3d_occluded"], n * 24 / 1e6, n / 1e6), flush=True)
    ds.set_stream(0)
    ds.close()


def main():
    print("library: %s" % api.LIB_PATH)
    bw = copy_bandwidth()
    print("copy bandwidth (1 GiB device-to-device, read + written): %.2f TB/s" % (bw / 1e12))
    print("%dx%d, accel BVH, radius %g, bias %g, device memory, %d calls after %d warm-ups, %d alternated repetitions, medians"
          % (W, H, RADIUS, BIAS, CALLS, WARMUP, REPEATS))
    for name in ("mount_low", "dragon"):
        for samples in (4, 16):
            measure(name, samples, bw)


if __name__ == "__main__":
    main()
