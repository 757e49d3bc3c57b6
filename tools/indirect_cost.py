#!/usr/bin/env python3
"""What p3d_indirect_diffuse costs (profiles/indirect_cost.txt): mount_low (served from LDS) and dragon (read from HBM) at
1920x1080, accel BVH, 4 and 16 samples per pixel, planes in device memory, one process.  Timed with p3d_timer_begin /
p3d_timer_end over CALLS calls after WARMUP warm-ups; the cases alternate REPEATS times and each figure is the median.
  (a) the fused entry, writing the indirect plane.
  (b) the unfused composition of the entries the library had before it: the rays of the pixels that have a query, made once
      by the host restatement (api.host_ao_segments at radius 1) and already in device memory -- neither making nor
      uploading them is timed --, p3d_trace_rays(max_depth = 1) on them, and one reduction over the samples' colours.  The
      reduction is torch's mean, not the definition's tree: it stands for the pass's traffic.
  (c) p3d_trace_rays alone on the materialised rays.
Pixels without a query have no ray in (b) and (c): the unfused pipeline gets that compaction for free.
Before anything is timed the fused result is compared, every bit, with the restatement's resolve of p3d_trace_rays' colours.
usage: python tools/indirect_cost.py [CALLS [WARMUP [REPEATS]]]"""
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
CALLS, WARMUP, REPEATS = [int(a) for a in ARGS[:3]] + [10, 2, 3][len(ARGS[:3]):]
W, H = 1920, 1080
BIAS, SEED = api.INDIRECT_BIAS, 1


def timed(ds, run):
    for _ in range(WARMUP):
        run()
    ds.sync()
    ds.timer_begin()
    for _ in range(CALLS):
        run()
    return ds.timer_end() / CALLS


def measure(name, samples):
    hs = P.HostScene(scene_path(name))
    hs.set_resolution(W, H)
    ds = P.DeviceScene.from_host(hs)
    cam = hs.camera()
    f = ds.render_aov(cam, max_depth=1, accel=P.ACCEL_BVH)
    depth, normal = f["depth"][0], f["normal"][0]
    dev = {k: torch.from_numpy(np.ascontiguousarray(f[k][0])).cuda() for k in ("depth", "normal")}
    ind = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda:0")
    fused = lambda: ds.indirect_diffuse_device(cam, dev["depth"].data_ptr(), dev["normal"].data_ptr(), out_indirect_ptr=ind.data_ptr(),
                                               samples=samples, bias=BIAS, seed=SEED, accel=P.ACCEL_BVH)
    o, d, valid = api.host_ao_segments(cam, depth, normal, samples=samples, radius=1.0, bias=BIAS, seed=SEED)
    m = valid.astype(bool)
    o, d = np.ascontiguousarray(o[m].reshape(-1, 3)), np.ascontiguousarray(d[m].reshape(-1, 3))
    n = len(o)
    ray_o, ray_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    col = torch.zeros(n, 3, dtype=torch.float32, device="cuda:0")
    mean = torch.zeros(n // samples, 3, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream()
    ds.set_stream(stream.cuda_stream)                       # one stream for the library's launches and the tool's
    with torch.cuda.stream(stream):
        before = ds.stats()["device_bytes"]
        trace = lambda: ds.trace_rays_device(n, ray_o.data_ptr(), ray_d.data_ptr(), rgb32f_ptr=col.data_ptr(), max_depth=1, accel=P.ACCEL_BVH)

        def unfused():
            trace()
            torch.mean(col.view(-1, samples, 3), dim=1, out=mean)

        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        unfused()
        ds.sync()
        workspace = free0 - torch.cuda.mem_get_info()[0]
        fused()
        ds.sync()
        rad = np.zeros((H, W, samples, 3), np.float32)
        rad[m] = col.cpu().numpy().reshape(-1, samples, 3)
        ref = api.host_indirect_resolve(rad, valid)["indirect"]
        got = ind.cpu().numpy().reshape(H, W, 3)
        equal = np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        print("%s S=%d: %.1f %% of the pixels have a query, %d rays; fused == resolve(p3d_trace_rays(host rays, max_depth 1)) in every bit: %s"
              % (name, samples, 100 * m.mean(), n, equal), flush=True)
        assert equal
        cases = [("(a) fused", fused), ("(b) unfused", unfused), ("(c) p3d_trace_rays", trace)]
        ms = {k: [] for k, _ in cases}
        for rep in range(REPEATS):
            for k, run in cases:
                ms[k].append(timed(ds, run))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k, _ in cases:
            print("  %-10s S=%-2d %-20s %8.4f ms  (%s)" % (name, samples, k, med[k], " ".join("%.4f" % v for v in ms[k])))
        print("  %-10s S=%-2d (a) / (b) = %.3f   (a) / (c) = %.3f   (b) allocates %.0f MB of rays + %.0f MB of colours, and its first call took "
              "%.0f MB more of the device (queues and workspace of the ray stream; the handle's device_bytes grew by %.0f MB)"
              % (name, samples, med["(a) fused"] / med["(b) unfused"], med["(a) fused"] / med["(c) p3d_trace_rays"], n * 24 / 1e6, n * 12 / 1e6,
                 workspace / 1e6, (ds.stats()["device_bytes"] - before) / 1e6), flush=True)
    ds.set_stream(0)
    ds.close()


def main():
    print("library: %s" % os.path.relpath(api.LIB_PATH, REPO))
    print("%dx%d, accel BVH, bias %g, device memory, %d calls after %d warm-ups, %d alternated repetitions, medians"
          % (W, H, BIAS, CALLS, WARMUP, REPEATS))
    for name in ("mount_low", "dragon"):
        for samples in (4, 16):
            measure(name, samples)


if __name__ == "__main__":
    main()
