#!/usr/bin/env python3
"""What p3d_upsample costs and buys (profiles/upsample_cost.txt): one MI355X, 1920x1080 output, accel BVH, planes in device
memory, one process.  Timed with p3d_timer_begin / p3d_timer_end over CALLS calls after WARMUP warm-ups; the cases alternate
REPEATS times and each figure is the median.  Every result is compared, every bit, with the host restatement
(api.host_upsample) before it is timed.
  1. the entry against its traffic floor, on dragon's planes: factor 2 and 4, 1 and 3 channels, both output planes, one frame
     per launch and the same frame 8 times in one launch (what a call costs besides its pixels drops out).  The floor
     is 16 + 4 c bytes read and written per output pixel (its depth and normal, its result), (16 + 4 c) / s^2 read per low
     pixel and 1 for the fallback byte, at the copy bandwidth measured in this process.
  2. the pipeline against what it replaces, on dragon and mount_low at 16 samples per pixel: (a) p3d_ambient_occlusion at the
     full resolution; (b) p3d_render_aov (depth and normal only, max_depth 1) and p3d_ambient_occlusion at res / 2, then
     p3d_upsample -- each part and the sum.
  3. quality, recorded and not asserted: the RMS difference, over the pixels with a hit, of (b)'s plane and of the plain
     bilinear plane (all guides made equal) against p3d_ambient_occlusion at the full resolution with 64 samples; the same for
     the full-resolution plane at 16 samples (the noise a 16-sample plane has anyway); the share of fallback pixels.
With P3D_LIB naming the library built without LDS staging (make -C csrc upsample_unstaged) and --entry-only, only part 1 runs:
the two variants are measured by running the tool twice in one session.
usage: python tools/upsample_cost.py [--entry-only] [CALLS [WARMUP [REPEATS]]]"""
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
ENTRY_ONLY = "--entry-only" in sys.argv[1:]
CALLS, WARMUP, REPEATS = [int(a) for a in ARGS[:3]] + [20, 3, 3][len(ARGS[:3]):]
W, H = 1920, 1080
BATCH = 8
RADIUS, BIAS, SEED = api.AO_RADIUS, api.AO_BIAS, 1
KW = dict(sigma_depth=api.UPSAMPLE_SIGMA_DEPTH, normal_power_log2=api.UPSAMPLE_NORMAL_POWER_LOG2)


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


def alternate(ds, cases):
    ms = {k: [] for k, _ in cases}
    for _ in range(REPEATS):
        for k, run in cases:
            ms[k].append(timed(ds, run))
    return {k: float(np.median(v)) for k, v in ms.items()}, ms


def low_camera(cam, s):
    low = api.Camera.from_buffer_copy(cam)
    low.res_x, low.res_y = cam.res_x // s, cam.res_y // s
    return low


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def entry(ds, hs, bw):
    cam = hs.camera()
    full = ds.render_aov(cam, max_depth=1, accel=P.ACCEL_BVH)
    d_depth, d_normal = cuda(full["depth"]), cuda(full["normal"])
    for s in (2, 4):
        lc = low_camera(cam, s)
        low = ds.render_aov(lc, max_depth=1, accel=P.ACCEL_BVH)
        ao = ds.ambient_occlusion(lc, low["depth"], low["normal"], samples=4, radius=RADIUS, bias=BIAS, seed=SEED, want=("ao",))["ao"]
        d_ld, d_ln = cuda(low["depth"]), cuda(low["normal"])
        for c, signal in ((1, ao), (3, low["rgb32f"])):
            d_low = cuda(signal)
            plane = torch.zeros(H * W * c, dtype=torch.float32, device="cuda:0")
            fb = torch.zeros(H * W, dtype=torch.uint8, device="cuda:0")
            run = lambda: ds.upsample_device(lc.res_x, lc.res_y, s, d_low.data_ptr(), d_ld.data_ptr(), d_ln.data_ptr(), d_depth.data_ptr(),
                                             d_normal.data_ptr(), out_plane_ptr=plane.data_ptr(), out_fallback_ptr=fb.data_ptr(), channels=c, **KW)
            torch.cuda.synchronize()                        # the buffers are made on torch's stream, the call runs on the scene's
            run()
            ds.sync()
            ref = api.host_upsample(signal, low["depth"], low["normal"], full["depth"], full["normal"], **KW)
            equal = same_bits(plane.cpu().numpy().reshape(ref["plane"].shape), ref["plane"]) and \
                same_bits(fb.cpu().numpy().reshape(ref["fallback"].shape), ref["fallback"])
            print("dragon s=%d c=%d: %.2f %% fallback pixels; device == host in every bit: %s" % (s, c, 100 * ref["fallback"].mean(), equal), flush=True)
            assert equal
            med, ms = alternate(ds, [("upsample", run)])
            per_px = 16 + 4 * c + (16 + 4 * c) / (s * s) + 1
            floor = H * W * per_px / bw * 1e3
            print("  dragon s=%d c=%d p3d_upsample %8.4f ms  (%s)   traffic %.2f bytes per output pixel = %.4f ms at the copy bandwidth: %.2f times the floor"
                  % (s, c, med["upsample"], " ".join("%.4f" % v for v in ms["upsample"]), per_px, floor, med["upsample"] / floor), flush=True)
            # the same frame BATCH times in ONE launch: what a call costs besides its pixels drops out
            b_in = [t.reshape(-1).repeat(BATCH) for t in (d_low, d_ld, d_ln, d_depth, d_normal)]
            b_plane = torch.zeros(BATCH * H * W * c, dtype=torch.float32, device="cuda:0")
            b_fb = torch.zeros(BATCH * H * W, dtype=torch.uint8, device="cuda:0")
            run_batch = lambda: ds.upsample_device(lc.res_x, lc.res_y, s, *[t.data_ptr() for t in b_in], out_plane_ptr=b_plane.data_ptr(),
                                                   out_fallback_ptr=b_fb.data_ptr(), n_frames=BATCH, channels=c, **KW)
            torch.cuda.synchronize()
            run_batch()
            ds.sync()
            equal = all(torch.equal(b_plane.view(BATCH, -1)[f].view(torch.int32), plane.view(torch.int32)) and torch.equal(b_fb.view(BATCH, -1)[f], fb)
                        for f in range(BATCH))
            assert equal, "a frame of the batch differs from the single frame"
            med, ms = alternate(ds, [("batch", run_batch)])
            print("  dragon s=%d c=%d p3d_upsample, %d frames in one launch %8.4f ms  (%s)   = %.4f ms per frame: %.2f times the floor"
                  % (s, c, BATCH, med["batch"], " ".join("%.4f" % v for v in ms["batch"]), med["batch"] / BATCH, med["batch"] / BATCH / floor), flush=True)


def pipeline(name, bw):
    hs = P.HostScene(scene_path(name))
    hs.set_resolution(W, H)
    ds = P.DeviceScene.from_host(hs)
    if name == "dragon":
        entry(ds, hs, bw)
        if ENTRY_ONLY:
            ds.close()
            return
    cam, s, S = hs.camera(), 2, 16
    lc = low_camera(cam, s)
    lw, lh = lc.res_x, lc.res_y
    full = ds.render_aov(cam, max_depth=1, accel=P.ACCEL_BVH)
    d_depth, d_normal = cuda(full["depth"]), cuda(full["normal"])
    ao_full = torch.zeros(H * W, dtype=torch.float32, device="cuda:0")
    d_ld = torch.zeros(lh * lw, dtype=torch.float32, device="cuda:0")
    d_ln = torch.zeros(lh * lw * 3, dtype=torch.float32, device="cuda:0")
    ao_low = torch.zeros(lh * lw, dtype=torch.float32, device="cuda:0")
    up = torch.zeros(H * W, dtype=torch.float32, device="cuda:0")
    fb = torch.zeros(H * W, dtype=torch.uint8, device="cuda:0")
    ao_kw = dict(radius=RADIUS, bias=BIAS, seed=SEED, accel=P.ACCEL_BVH)
    a_full = lambda: ds.ambient_occlusion_device(cam, d_depth.data_ptr(), d_normal.data_ptr(), out_ao_ptr=ao_full.data_ptr(), samples=S, **ao_kw)
    b_planes = lambda: ds.render_aov_device(lc, depth_ptr=d_ld.data_ptr(), normal_ptr=d_ln.data_ptr(), max_depth=1, accel=P.ACCEL_BVH)
    b_ao = lambda: ds.ambient_occlusion_device(lc, d_ld.data_ptr(), d_ln.data_ptr(), out_ao_ptr=ao_low.data_ptr(), samples=S, **ao_kw)
    b_up = lambda: ds.upsample_device(lw, lh, s, ao_low.data_ptr(), d_ld.data_ptr(), d_ln.data_ptr(), d_depth.data_ptr(), d_normal.data_ptr(),
                                      out_plane_ptr=up.data_ptr(), out_fallback_ptr=fb.data_ptr(), **KW)

    def b_all():
        b_planes(); b_ao(); b_up()

    torch.cuda.synchronize()
    a_full(); b_all()
    ds.sync()
    low_planes = (ao_low.cpu().numpy().reshape(1, lh, lw), d_ld.cpu().numpy().reshape(1, lh, lw), d_ln.cpu().numpy().reshape(1, lh, lw, 3))
    ref = api.host_upsample(*low_planes, full["depth"], full["normal"], **KW)
    got, got_fb = up.cpu().numpy().reshape(1, H, W), fb.cpu().numpy().reshape(1, H, W)
    equal = same_bits(got, ref["plane"]) and same_bits(got_fb, ref["fallback"])
    print("%s S=%d s=%d: the pipeline's plane == host_upsample of its low planes in every bit: %s" % (name, S, s, equal), flush=True)
    assert equal
    med, ms = alternate(ds, [("(a) full-resolution AO", a_full), ("(b) low planes", b_planes), ("(b) low AO", b_ao), ("(b) upsample", b_up),
                             ("(b) all three", b_all)])
    for k in med:
        print("  %-10s S=%d %-24s %8.4f ms  (%s)" % (name, S, k, med[k], " ".join("%.4f" % v for v in ms[k])))
    parts = med["(b) low planes"] + med["(b) low AO"] + med["(b) upsample"]
    print("  %-10s S=%d (b) sum of the parts %.4f ms; (b) / (a) = %.3f (sum of the parts), %.3f (the three enqueued together)"
          % (name, S, parts, parts / med["(a) full-resolution AO"], med["(b) all three"] / med["(a) full-resolution AO"]), flush=True)
    # quality: against the full resolution at 64 samples, hits only
    truth = ds.ambient_occlusion(cam, full["depth"], full["normal"], samples=64, want=("ao",), **ao_kw)["ao"]
    hit = np.isfinite(full["depth"]) & (full["depth"] > 0)
    flat = api.host_upsample(low_planes[0], np.ones_like(low_planes[1]), np.zeros_like(low_planes[2]) + np.float32((0, 0, 1)),
                             np.ones_like(full["depth"]), np.zeros_like(full["normal"]) + np.float32((0, 0, 1)), **KW)["plane"]
    rms = lambda a: float(np.sqrt(np.mean((a[hit].astype(np.float64) - truth[hit]) ** 2)))
    print("  %-10s quality against full-resolution AO at S=64, %d pixels with a hit (RMS): guided upsample of half-resolution S=%d %.5f; "
          "plain bilinear of the same plane %.5f; full-resolution S=%d %.5f; fallback pixels %.3f %% of the frame"
          % (name, int(hit.sum()), S, rms(got), rms(flat), S, rms(ao_full.cpu().numpy().reshape(1, H, W)), 100 * got_fb.mean()), flush=True)
    ds.close()


def main():
    print("library: %s" % os.path.basename(api.LIB_PATH))
    bw = copy_bandwidth()
    print("copy bandwidth (1 GiB device-to-device, read + written): %.2f TB/s" % (bw / 1e12))
    print("%dx%d output, accel BVH, radius %g, bias %g, device memory, %d calls after %d warm-ups, %d alternated repetitions, medians"
          % (W, H, RADIUS, BIAS, CALLS, WARMUP, REPEATS))
    for name in ("dragon",) if ENTRY_ONLY else ("dragon", "mount_low"):
        pipeline(name, bw)


if __name__ == "__main__":
    main()
