#!/usr/bin/env python3
"""What p3d_accumulate_moving costs beside p3d_accumulate (profiles/accumulate_moving_cost.txt): sequences of 4 frames at
1920x1080 whose primitives move between the frames (p3d_scene_update, then p3d_render_aov, frame by frame), planes and
geometry in device memory, accumulated in one call by
    p3d_accumulate                              the yardstick: the parent's code, which drops (or smears) what moved
    p3d_accumulate_moving, unchanged geometry   the lookup alone: kind and two records per hit pixel, the static rule, no arithmetic
    p3d_accumulate_moving                       the lookup and the map of the hit point
    p3d_accumulate_moving with prev_xy          and 8 more bytes written per pixel
alternated REPEATS times, each timed with p3d_timer_begin / p3d_timer_end over CALLS calls after WARMUP warm-ups; the medians
are reported.  Three cases: the dof orbit of tools/accumulate_cost.py with three of its spheres moving; dragon with every
triangle of the model moving, through a camera of this tool's that orbits the model from near; and, since dragon's frames
show only a few dozen of its 100 005 primitives whatever the camera, the dof sequence again with its primitives copied
11 111 times and every 2 x 2 block of pixels given a copy of its own (measure(copies=...)) -- about one primitive per four
pixels, where the record gather is worst.  Beside every figure stands the traffic floor at the copy
bandwidth measured in the same process: p3d_accumulate's 84 bytes per pixel of a frame with history (28 without), plus
4 + 96 bytes (kind, two records) of every primitive such a frame shows, counted once however many of its pixels ask for
them, plus 8 per pixel where prev_xy is written.  What the lanes ASK for -- 100 bytes per hit pixel -- is printed beside
it: the caches stand between the two.  Every timed result is compared with the host restatement, every bit, before it is
timed.
usage: python tools/accumulate_moving_cost.py [CALLS [WARMUP [REPEATS]]]"""
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
import accumulate_reference as R  # noqa: E402
from accumulate_cost import copy_bandwidth  # noqa: E402

CALLS, WARMUP, REPEATS = [int(a) for a in sys.argv[1:4]] + [50, 5, 5][len(sys.argv[1:4]):]
W, H, N = 1920, 1080, 4
PLANES = ("rgb32f", "depth", "normal", "hit_id")
KW = dict(depth_tolerance=api.ACCUMULATE_DEPTH_TOLERANCE, normal_min=api.ACCUMULATE_NORMAL_MIN, max_history=api.ACCUMULATE_MAX_HISTORY)


def same(t, ref):
    return bool(np.array_equal(t.cpu().numpy().view(np.uint32).reshape(-1), np.ascontiguousarray(ref).view(np.uint32).reshape(-1)))


def close_orbit(ptype, data, moved, step_deg):
    """N cameras that orbit the moving primitives' bounding box by step_deg per frame, near enough for it to fill the frame."""
    pts = data[moved][:, :9].reshape(-1, 3).astype(np.float64)
    lo, hi = pts.min(0), pts.max(0)
    centre, reach = (lo + hi) / 2, 1.1 * (hi - lo).max()
    cams = []
    for f in range(N):
        a = np.radians(40.0 + step_deg * f)
        cams.append(R.look_at(centre + reach * np.array([np.sin(a), 0.45, np.cos(a)]), centre, W, H))
    return cams


def measure(name, scene, step_deg, moved_of, step_of, bw, close=False, copies=1, **render):
    """One scene: moved_of(ptype, data) -> the indices that move; step_of(f) -> their translation in frame f.  copies > 1: after
    rendering, the primitives are copied that many times (id k + n_prims * j carries the record of k) and every hit pixel's id
    moved to the copy of its 2 x 2 screen block, in every frame alike: the arithmetic per pixel is what it was, but
    neighbouring blocks now read records far apart -- a primitive per 4 pixels.  Blocks are fixed on the screen, so under the
    orbit the id test drops the taps that cross a block's border: fewer taps are read than in a real scene of that density."""
    hs = P.HostScene(scene_path(scene))
    hs.set_resolution(W, H)
    ptype, data = hs.arrays()[:2]
    ds = P.DeviceScene.from_host(hs)
    moved = moved_of(ptype, data)
    cams = close_orbit(ptype, data, moved, step_deg) if close else hs.orbit_cameras(N, step_deg)
    recs = np.stack([data] * N)
    for f in range(N):
        s = np.asarray(step_of(f), np.float32)
        sph, tri = moved[ptype[moved] == 0], moved[ptype[moved] == 1]
        recs[f, sph, :3] += s
        recs[f, tri, :9] += np.tile(s, 3)
    frames = []
    for f in range(N):
        ds.update(recs[f])
        frames.append(ds.render_aov(cams[f], max_depth=4, accel=hs.accel, **render))
    pl = {k: np.concatenate([fr[k] for fr in frames]) for k in PLANES}
    if copies > 1:
        ys, xs = np.mgrid[0:H, 0:W]
        copy = (((xs // 2) * 7919 + (ys // 2) * 104729) % copies).astype(np.int32)
        pl["hit_id"] = np.ascontiguousarray(np.where(pl["hit_id"] >= 0, pl["hit_id"] + len(ptype) * copy, pl["hit_id"]).astype(np.int32))
        moved = (moved[None, :] + len(ptype) * np.arange(copies)[:, None]).reshape(-1)
        ptype, data, recs = np.tile(ptype, copies), np.tile(data, (copies, 1)), np.ascontiguousarray(np.tile(recs, (1, copies, 1)))
    still = np.stack([data] * N)
    args = tuple(pl[k] for k in PLANES[:3]) + (cams, pl["hit_id"])
    ref_plain = api.host_accumulate(*args, **KW)
    ref_still = api.host_accumulate_moving(*args, ptype, still, **KW)
    ref = api.host_accumulate_moving(*args, ptype, recs, **KW)
    hit = pl["hit_id"] >= 0
    on = np.isin(pl["hit_id"], moved)
    px = W * H
    print("\n%s: %s %dx%d, %d primitives, %d of them moving, %d orbit frames %g degrees apart; %.1f %% of the pixels hit, %.1f %% show a moving primitive"
          % (name, scene, W, H, len(ptype), len(moved), N, step_deg, 100 * hit.mean(), 100 * on.mean()))
    print("  pixels of moving primitives that took history, frames 1 to %d: p3d_accumulate %s, p3d_accumulate_moving %s" % (
        N - 1, ", ".join("%.1f %%" % (100 * (ref_plain["length"][f][on[f]] > 1).mean()) for f in range(1, N)),
        ", ".join("%.1f %%" % (100 * (ref["length"][f][on[f]] > 1).mean()) for f in range(1, N))))
    print("  the host restatement with unchanged geometry == p3dh_accumulate in every bit: %s" % all(
        np.array_equal(ref_still[k].view(np.uint32), ref_plain[k].view(np.uint32)) for k in ("rgb32f", "length")))
    dev = {k: torch.from_numpy(pl[k]).cuda() for k in PLANES}
    d_type = torch.from_numpy(ptype.view(np.int32)).cuda()
    d_recs, d_still = torch.from_numpy(recs).cuda(), torch.from_numpy(still).cuda()
    o32 = torch.zeros(N * px * 3, dtype=torch.float32, device="cuda:0")
    ol = torch.zeros(N * px, dtype=torch.float32, device="cuda:0")
    oxy = torch.zeros(N * px * 2, dtype=torch.float32, device="cuda:0")
    planes = [dev[k].data_ptr() for k in PLANES[:3]]

    def plain():
        ds.accumulate_device(W, H, cams, *planes, hit_ptr=dev["hit_id"].data_ptr(), out_rgb32f_ptr=o32.data_ptr(), out_length_ptr=ol.data_ptr(), **KW)

    def moving(geometry=d_recs, xy=False):
        ds.accumulate_moving_device(W, H, cams, *planes, dev["hit_id"].data_ptr(), len(ptype), d_type.data_ptr(), geometry.data_ptr(),
                                    out_rgb32f_ptr=o32.data_ptr(), out_length_ptr=ol.data_ptr(), out_prev_xy_ptr=oxy.data_ptr() if xy else 0, **KW)

    hist_frames = N - 1
    base = hist_frames * 84 + 28
    # the lookup of the frames with history, in bytes per pixel of one frame: what the lanes ask for (kind and two records per
    # hit pixel), and what must come from memory at least once (kind and two records per primitive a frame shows)
    asked = 100 * float(hit[1:].sum()) / px
    lookup = 100 * float(sum(len(np.unique(pl["hit_id"][f][hit[f]])) for f in range(1, N))) / px
    print("  primitives a frame shows: %s; pixels per shown primitive %.1f; the lanes ask for %.1f bytes of kinds and records per pixel and frame with history, %.2f must be fetched"
          % (", ".join(str(len(np.unique(pl["hit_id"][f][hit[f]]))) for f in range(N)), hit[1:].sum() / max(1.0, lookup * px / 100),
             asked / hist_frames, lookup / hist_frames))
    cases = [("p3d_accumulate                           ", plain, ref_plain, False, base),
             ("p3d_accumulate_moving, unchanged geometry", lambda: moving(d_still), ref_still, False, base + lookup),
             ("p3d_accumulate_moving                    ", moving, ref, False, base + lookup),
             ("p3d_accumulate_moving with prev_xy       ", lambda: moving(xy=True), ref, True, base + lookup + 8 * N)]
    for label, run, r, xy, _ in cases:
        o32.zero_(); ol.zero_(); oxy.zero_()
        torch.cuda.synchronize()                                 # the library runs on the scene's stream, not on torch's
        run()
        ds.sync()
        ok = same(o32, r["rgb32f"]) and same(ol, r["length"]) and (not xy or same(oxy, r["prev_xy"]))
        print("  %s the device == the host restatement in every bit: %s" % (label, ok), flush=True)
        if not ok:
            raise SystemExit("not timed: the results differ")
    ms = {label: [] for label, *_ in cases}
    for rep in range(REPEATS):
        for label, run, *_ in cases:
            for _ in range(WARMUP):
                run()
            ds.sync()
            ds.timer_begin()
            for _ in range(CALLS):
                run()
            ms[label].append(ds.timer_end() / CALLS)
    yard = float(np.median(ms[cases[0][0]]))
    for label, _, _, _, bytes_per_pixel in cases:
        m = float(np.median(ms[label]))
        floor = bytes_per_pixel * px / bw * 1e3
        print("  %s median %8.4f ms  (%s)   floor %7.4f ms (%6.1f bytes per pixel)   over the floor %5.2f   over p3d_accumulate %5.2f"
              % (label, m, " ".join("%.4f" % v for v in ms[label]), floor, bytes_per_pixel, m / floor, m / yard), flush=True)
    ds.close()


def main():
    print("library: %s" % api.LIB_PATH)
    bw = copy_bandwidth()
    print("copy bandwidth (1 GiB device-to-device, read + written): %.2f TB/s" % (bw / 1e12))
    print("%d calls after %d warm-ups, %d alternated repetitions; tolerance %g, normal_min %g, max_history %g" % (
        CALLS, WARMUP, REPEATS, KW["depth_tolerance"], KW["normal_min"], KW["max_history"]))
    # dof: spheres 3, 4 and 5 (radius 0.5) slide 0.1 along x per frame
    measure("small scene", "dof", 1.0, lambda t, d: np.array([3, 4, 5]), lambda f: (0.1 * f, 0.0, 0.0), bw, soft_shadow=True)
    # dragon: every triangle of the model (the two ground triangles and the spheres stay) slides 0.004 along x per frame
    measure("dragon", "dragon", 1.0, lambda t, d: np.flatnonzero((t == 1) & (np.abs(d[:, :9]).max(1) < 3)), lambda f: (0.004 * f, 0.0, 0.0), bw, close=True)
    # a primitive per 4 pixels: the dof sequence with its 9 primitives copied 11111 times (99 999 records per frame, 4.8 MB)
    measure("dense ids", "dof", 1.0, lambda t, d: np.array([3, 4, 5]), lambda f: (0.1 * f, 0.0, 0.0), bw, copies=11111, soft_shadow=True)


if __name__ == "__main__":
    main()
