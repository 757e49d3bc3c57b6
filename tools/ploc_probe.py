#!/usr/bin/env python3
"""The three BVH builders side by side, and p3d_scene_rebuild_with(2) on a moved scene (GPU box).

Scenes: the dragon and the 1e6-primitive synthetic scene at 1920x1080, depth 4.  In one run, for builders 0 (host binned
SAH), 1 (device LBVH) and 2 (device clustering, csrc/bvh_ploc.hip): wall time of p3d_scene_create, SAH cost and depth of the
tree, clustering rounds (asked of p3d_debug_ploc_build over the same build primitives), and the frame time.  A second fresh
builder-1 handle is timed too: the difference between the two is this run's own noise.  Then the rows of
tools/scene_rebuild_probe.py for builder 2: every primitive displaced by a seeded random vector (|component| <= 1 %, then
10 %, of the largest scene extent), a handle updated from device memory, and p3d_scene_rebuild_with(1) and (2) on it:
wall time, SAH cost, frame time.  One process; writes profiles/ploc_build.txt.
usage: ploc_probe.py [SCENE_OR_N ...]      (default: dragon 1000000)"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import scene_path
import torch
import u_4a_2s_p3d_raytracer_template2_amd as P
from u_4a_2s_p3d_raytracer_template2_amd import synthetic as S, api

RES, DEPTH = (1920, 1080), 4
NAMES = {0: "host SAH", 1: "device LBVH", 2: "device clustering"}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def displaced(ptype, data, share, seed):
    """Every primitive translated by a random vector of at most `share` of the largest scene extent per component."""
    rng = np.random.default_rng(seed)
    d = np.array(data, np.float32)
    pts = np.concatenate([d[ptype == 0, :3], d[ptype == 1, :9].reshape(-1, 3), d[ptype == 2, :6].reshape(-1, 3)])
    extent = float((pts.max(0) - pts.min(0)).max())
    step = rng.uniform(-share * extent, share * extent, (len(d), 3)).astype(np.float32)
    d[ptype == 0, :3] += step[ptype == 0]
    d[ptype == 1, :9] += np.tile(step[ptype == 1], 3)
    d[ptype == 2, :6] += np.tile(step[ptype == 2], 2)
    return d                                             # (planes stay)


def frame_ms(ds, cam, buf):
    for _ in range(8):                                   # the measured schedule choice settles in the first six
        ds.render_device(cam, rgb8_ptr=buf.data_ptr(), max_depth=DEPTH)
    ds.timer_begin()
    for _ in range(8):
        ds.render_device(cam, rgb8_ptr=buf.data_ptr(), max_depth=DEPTH)
    return ds.timer_end() / 8


def created(desc, keep, builder, times=2):
    """(handle, best wall time of p3d_scene_create)"""
    best, ds = 1e9, None
    for _ in range(times):
        if ds is not None:
            ds.close()
        t0 = time.perf_counter(); ds = P.DeviceScene(desc, keepalive=keep, builder=builder); t = time.perf_counter() - t0
        best = min(best, t)
    return ds, best


for arg in (sys.argv[1:] or ["dragon", "1000000"]):
    if arg.isdigit():
        cam = P.HostScene(S.camera_p3f("/tmp/synth_camera.p3f", *RES)).camera()
        arrays = S.arrays(int(arg))
    else:
        hs = P.HostScene(scene_path(arg)); hs.set_resolution(*RES); cam = hs.camera()
        arrays = hs.arrays()
    ptype, data = np.asarray(arrays[0]), np.ascontiguousarray(arrays[1], np.float32)
    buf = torch.zeros((RES[1] + 16, RES[0], 3), dtype=torch.uint8, device="cuda")
    desc, keep = api.make_desc(*arrays)
    for b in (1, 2):                                     # first-use costs (module load) out of the timings
        warm = P.DeviceScene(desc, keepalive=keep, builder=b); warm.rebuild(builder=b); warm.close()
    say("%s: %d primitives" % (arg, len(ptype)))
    lo, hi, ref = api.host_build_prims(desc)
    probe = api.ploc_build(lo, hi, ref)
    frames, times_ms = {}, {}
    for b in (0, 1, 2):
        ds, t_create = created(desc, keep, b, times=1 if b == 0 else 2)
        st = ds.stats()
        times_ms[b] = frame_ms(ds, cam, buf)
        frames[b] = buf.cpu().numpy().copy()
        rounds = "%d rounds%s" % (probe["rounds"], ", fell back" if probe["fell_back"] else "") if b == 2 else "-"
        say("  builder %d (%s): p3d_scene_create %.4f s | SAH cost %.2f, max_depth %d, %s | frame %.3f ms | last_builder %d" % (
            b, NAMES[b], t_create, st["sah_cost"], st["max_depth"], rounds, times_ms[b], ds.last_builder()))
        ds.close()
    again, _ = created(desc, keep, 1, times=1)
    second = frame_ms(again, cam, buf)
    again.close()
    noise = abs(second - times_ms[1])
    say("  builder 1 again: frame %.3f ms (noise of this run %.3f ms) | same frame on all three: %s" % (
        second, noise, np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[2])))
    say("  builder 2 - builder 1 frame time %+.3f ms; builder 2 - builder 0 %+.3f ms" % (
        times_ms[2] - min(times_ms[1], second), times_ms[2] - times_ms[0]))
    for share in (0.01, 0.10):
        moved = displaced(ptype, data, share, 17)
        d_moved = torch.from_numpy(moved).cuda(); torch.cuda.synchronize()
        row = {}
        for b in (1, 2):
            t_rebuild = 1e9
            for k in range(3):                           # a new handle each time: every rebuild starts from the refitted SAH tree
                ds = P.DeviceScene(desc, keepalive=keep)
                ds.update_device(len(moved), d_moved.data_ptr())
                if b == 1 and k == 2:
                    refit_ms = frame_ms(ds, cam, buf)
                    frame_refit = buf.cpu().numpy().copy()
                ds.sync()
                t0 = time.perf_counter(); info = ds.rebuild(builder=b); t = time.perf_counter() - t0
                t_rebuild = min(t_rebuild, t)
                if k < 2:
                    ds.close()
            ms = frame_ms(ds, cam, buf)
            row[b] = (t_rebuild, info["sah_cost_before"], info["sah_cost_after"], info["max_depth"], ms, ds.last_builder(),
                      np.array_equal(buf.cpu().numpy(), frame_refit))
            ds.close()
        say("  motion %2d %%: refitted SAH tree: cost %.1f, frame %.3f ms" % (round(100 * share), row[1][1], refit_ms))
        for b in (1, 2):
            say("             rebuild_with(%d) %.4f s | SAH cost -> %.1f, max_depth %d | frame %.3f ms | last_builder %d | same frame: %s" % (
                b, row[b][0], row[b][2], row[b][3], row[b][4], row[b][5], row[b][6]))

os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
with open(os.path.join(REPO, "profiles", "ploc_build.txt"), "w") as f:
    f.write("tools/ploc_probe.py: %dx%d, depth %d, wall times best of 2 (host SAH: 1; rebuilds: best of 3), frames mean of 8\n" % (*RES, DEPTH))
    f.write("\n".join(lines) + "\n")
