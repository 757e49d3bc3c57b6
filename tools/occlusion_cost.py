"""What p3d_occluded costs: N segments in the style of tests/test_oracle_vs_ref.scene_rays (half camera rays through random
pixels, half between scene points with 0.3 of normal noise) on balls_box and mount_low (served from LDS), mount_high and dragon (read from
HBM), device memory in and out, BVH mode, timed with p3d_timer_begin / p3d_timer_end over CALLS calls after WARMUP warm-ups,
REPEATS times.  The yardstick is p3d_trace_rays on the same handle and rays with max_depth = 1 and only hit_id requested,
timed the same way in the same process.
usage: python tools/occlusion_cost.py [LOG2_N [CALLS [WARMUP [REPEATS]]]]"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from extra_scenes import scene_path                  # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P      # noqa: E402

LOG2_N, CALLS, WARMUP, REPEATS = [int(a) for a in sys.argv[1:5]] + [20, 500, 20, 3][len(sys.argv[1:5]):]
N = 1 << LOG2_N


def segments(hs, rng, n):
    """scene_rays, vectorised: Camera::PrimaryRay in float32 for the first half, point-to-point segments for the second."""
    cam = hs.camera()
    f = np.float32
    eye, u, v, nn = [np.array(list(getattr(cam, k)), f) for k in ("eye", "u", "v", "n")]
    half = n // 2
    px, py = (rng.random(half) * cam.res_x).astype(f), (rng.random(half) * cam.res_y).astype(f)
    dirs = (u * f(cam.w))[None] * (px / f(cam.res_x) - f(0.5))[:, None] + (v * f(cam.h))[None] * (py / f(cam.res_y) - f(0.5))[:, None] \
        + (nn * f(-cam.plane_dist))[None]
    dirs = (dirs / np.sqrt((dirs * dirs).sum(-1, dtype=f))[:, None]).astype(f)
    pts = hs.arrays()[1][:, :3]
    a = pts[rng.integers(len(pts), size=n - half)] + rng.standard_normal((n - half, 3)).astype(f) * f(0.3)
    b = pts[rng.integers(len(pts), size=n - half)] + rng.standard_normal((n - half, 3)).astype(f) * f(0.3)
    o = np.concatenate([np.broadcast_to(eye, (half, 3)), a]).astype(f)
    d = np.concatenate([dirs, b - a]).astype(f)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def timed(ds, run):
    for _ in range(WARMUP):
        run()
    ds.sync()
    ds.timer_begin()
    for _ in range(CALLS):
        run()
    return ds.timer_end() / CALLS


def measure(name, what):
    """-> lines of `what` ("occluded", "trace") timings on a fresh handle of scene `name`."""
    hs = P.HostScene(scene_path(name))
    ds = P.DeviceScene.from_host(hs)
    L = P.lib()
    o, d = segments(hs, np.random.default_rng(7), N)
    ptr = {}
    for k, b in (("o", 12 * N), ("d", 12 * N), ("occ", N), ("hit", 4 * N)):
        p = C.c_void_p()
        assert L.p3d_device_alloc(ds.h, b, C.byref(p)) == 0
        ptr[k] = p.value
    assert L.p3d_upload(ds.h, ptr["o"], o.ctypes.data, 12 * N) == 0 and L.p3d_upload(ds.h, ptr["d"], d.ctypes.data, 12 * N) == 0
    runs = {"occluded": lambda: ds.occluded_device(N, ptr["o"], ptr["d"], ptr["occ"], accel=P.ACCEL_BVH),
            "trace": lambda: ds.trace_rays_device(N, ptr["o"], ptr["d"], hit_ptr=ptr["hit"], max_depth=1, accel=P.ACCEL_BVH)}
    # the two entries agree on what they both know: occluded <=> the closest hit of the normalised ray is nearer than |dir|
    # is tests/test_gpu_occluded.py's; here only the share of occluded segments is printed
    runs["occluded"]()
    ds.sync()
    occ = np.zeros(N, np.uint8)
    assert L.p3d_download(ds.h, occ.ctypes.data, ptr["occ"], N) == 0
    out = []
    for rep in range(REPEATS):
        for k in what:
            ms = timed(ds, runs[k])
            out.append("  repeat %d  %-10s %-28s %8.4f ms  %9.1f Msegments/s" % (
                rep, name, {"occluded": "p3d_occluded", "trace": "p3d_trace_rays depth 1 hit_id"}[k],
                ms, N / ms / 1e3))
    out.append("             %-10s %.1f %% of the segments are occluded" % (name, 100.0 * occ.mean()))
    for p in ptr.values():
        L.p3d_device_free(ds.h, C.c_void_p(p))
    ds.close()
    return out


def main():
    print("2^%d segments, BVH mode, device memory, %d calls after %d warm-ups, one call at a time" % (LOG2_N, CALLS, WARMUP))
    for name in ("balls_box", "mount_low", "mount_high", "dragon"):
        print("\n".join(measure(name, ("occluded", "trace"))), flush=True)


if __name__ == "__main__":
    main()
