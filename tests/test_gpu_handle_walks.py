"""One scene handle across configuration changes, on the GPU.

A p3d_scene handle keeps tile orders, the measured schedule choice, the workspace budget, the ray-factor table, grow-only
workspaces, self-re-arming control words, occupancy caches, the soft lights and the lazily built grid between calls
(csrc/p3d_scene_state.h), each keyed on a part of the request (csrc/p3d_frame_config.h).  The other GPU tests make a fresh
handle per configuration; these change the configuration under a live one: the walks of tests/handle_walks.py (whose
transitions tests/test_handle_walks.py asserts on the CPU), the periodic re-sort of a tile order, row blocks that are no
power of two, the other entries of the C-ABI between frames, and tuning changes.

Expected pixels are the committed fixtures tests/golden/balls_high_frames.npz and tests/golden/frames.npz -- the
reference's own object code -- at the project's bar: rgb32f bit for bit (conftest.RGB_TOL = 0), rgb8 equal, hit ids equal,
closest / shadow query and ray counts equal.  The rows of a shard are the fixture's rows under image row =
(blk * world + rank) * row_block + r; rows of a compact buffer past the image are not looked at in host outputs.
Nothing here captures a graph: a captured frame holds addresses a later, larger configuration may replace.
"""
import tempfile

import numpy as np
import pytest

from conftest import RGB_TOL, assert_rgb8_equal
from extra_scenes import scene_path
from oracle import oracle_py as O
import handle_walks as W
import occlusion_refs as R
from test_gpu_render_frames import eyes_around, p3f_with_eye
import u_4a_2s_p3d_raytracer_template2_amd as P

pytestmark = pytest.mark.gpu

assert RGB_TOL == 0.0
SCHEDULES = [None, "tile", "wavefront", "tree"]
IDS = ["default", "tile", "wavefront", "tree"]
PERIOD = W.tile_order_period()
THREADS = 16

_fixtures, _samples, _refs = {}, {}, {}


def fx(name):
    if name not in _fixtures:
        _fixtures[name] = W.fixture(name)
    return _fixtures[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_frame(out, ref, what):
    assert np.array_equal(out["hit_id"], ref["hit_id"]), "%s: primary hit ids differ in %d px, first at %s" % (
        what, int((out["hit_id"] != ref["hit_id"]).sum()), np.argwhere(out["hit_id"] != ref["hit_id"])[:1].tolist())
    bad = (bits(out["rgb32f"]) != bits(ref["rgb32f"])).any(-1)
    assert not bad.any(), "%s: rgb32f differs in %d px, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[:1].tolist())
    assert_rgb8_equal(out["rgb8"], ref["rgb8"], what)


def check(out, name, what):
    """A frame with counters against fixture `name`."""
    f = fx(name)
    same_frame(out, f, what)
    c, m = out["counters"], f["meta"]
    for k in ("closest_queries", "shadow_queries", "rays"):
        assert c[k] == m["counters"][k], (what, k, c[k], m["counters"][k])
    assert c["pixels"] == m["res"][0] * m["res"][1], what


def open_scene(scene, **opts):
    hs = P.HostScene(scene_path(scene))
    return hs, P.DeviceScene.from_host(hs, **opts)


def request(hs, st, schedule, private_walk=False):
    """(camera, keyword arguments of DeviceScene.render, forced schedule or None) of a step."""
    m = W.META[st["fixture"]]
    hs.set_resolution(*m["res"])
    if m["spp"] and st["fixture"] not in _samples:
        _samples[st["fixture"]] = hs.samples(m["seed"], m["spp"])
    kw = dict(max_depth=m["max_depth"], accel=m["accel"], spp=m["spp"], samples=_samples[st["fixture"]] if m["spp"] else None,
              soft_shadow=m["soft_shadow"], counters=True, row_block=st["row_block"], world=st["world"], no_lds=st["no_lds"],
              private_walk=private_walk)
    forced = None if schedule is None or (schedule == "tree" and W.tree_refuses(st)) else schedule
    if forced:
        kw[forced] = True
    return hs.camera(), kw, forced


def render_step(hs, ds, st, schedule, private_walk=False, frames=2):
    """`frames` frames of a step, rank by rank (so that a rank's second frame can draw from the order its first one
    learned), each stitched from every rank's shard.  A rank reports the pixels of the image rows it owns: none for a rank
    whose row blocks all lie past the image.  Host planes are copies of the handle's staging planes, which keep the last
    frame: a tile left undrawn by a stale order would show the previous frame's pixels, so every frame is rendered with
    counters -- zeroed per frame -- and its pixel, query and ray counts are asserted with its pixels."""
    cam, kw, forced = request(hs, st, schedule, private_walk)
    Wd, H = W.META[st["fixture"]]["res"]
    parts = {}
    for c in W.calls([st]):
        parts[c["rank"]] = []
        for k in range(frames):
            out = ds.render(cam, rank=c["rank"], **kw)
            if forced:
                assert ds.last_schedule() == forced, (st, k)
            assert out["counters"]["pixels"] == len(W.shard_rows(H, st["row_block"], st["world"], c["rank"])) * Wd, (st, c["rank"], k)
            parts[c["rank"]].append(out)
    if st["world"] == 1:
        return parts[0]
    return [W.stitch([parts[r][k] for r in range(st["world"])], H, Wd, st["world"], st["row_block"]) for k in range(frames)]


# ---- a. the walks

@pytest.mark.parametrize("schedule", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("walk,private_walk", [("BH", False), ("BH", True), ("ML", False)], ids=["BH-shared", "BH-private", "ML"])
def test_walk_on_one_handle(walk, private_walk, schedule):
    scene, steps = W.WALKS[walk]
    hs, ds = open_scene(scene)
    for i, st in enumerate(steps):
        for k, out in enumerate(render_step(hs, ds, st, schedule, private_walk)):
            check(out, st["fixture"], "%s step %d %s, frame %d, %s" % (walk, i, st, k, schedule))
    ds.close()


# ---- b. the periodic re-sort

@pytest.mark.parametrize("schedule", SCHEDULES, ids=IDS)
def test_tile_order_is_sorted_again_after_a_period_of_frames(schedule):
    """Frame 0 measures, frame 1 draws through the first order; frames PERIOD + 1 and 2 * PERIOD + 2 sort again, so the
    2 * PERIOD + 3 frames draw through three orders."""
    hs, ds = open_scene(W.BH_SCENE)
    cam, kw, forced = request(hs, W.step(W.BIG), schedule)
    for k in range(2 * PERIOD + 3):
        out = ds.render(cam, **kw)
        if forced:
            assert ds.last_schedule() == forced
        check(out, W.BIG, "%s frame %d" % (schedule, k))
    ds.close()


# ---- c. row blocks that are no power of two, fresh handles

@pytest.mark.parametrize("schedule", SCHEDULES, ids=IDS)
@pytest.mark.parametrize("name", [W.BIG, W.A], ids=["balls_high", "mount_low"])
def test_row_blocks_that_are_no_power_of_two(name, schedule):
    """image_row() divides instead of shifting.  row_block 80 and 112 cut both images into two blocks: rank 2 of 3 owns no
    image row, its call succeeds and reports no pixel (render_step)."""
    hs = P.HostScene(scene_path(W.META[name]["scene"]))
    assert W.shard_rows(W.META[name]["res"][1], 80, 3, 2) == []
    for rb in (48, 80, 112):
        for world in (1, 2, 3):
            ds = P.DeviceScene.from_host(hs)
            out, = render_step(hs, ds, W.step(name, rb, world), schedule, frames=1)
            check(out, name, "%s row_block %d world %d %s" % (name, rb, world, schedule))
            ds.close()


@pytest.mark.parametrize("name,rb", [(W.BIG, 48), ("bh_64_d4_spp2", 48), (W.A, 80), ("c4_mount_low_96_d6_spp2", 80)])
def test_device_planes_of_res_y_rows_with_a_row_block_that_is_no_power_of_two(name, rb):
    """world == 1: a caller's device planes hold res_y rows, the compact buffer local_rows(res_y, row_block) > res_y.  The
    canary rows behind the image cover all of that padding and stay intact; spp 0 and 2 (sum_samples_kernel)."""
    torch = pytest.importorskip("torch")
    hs = P.HostScene(scene_path(W.META[name]["scene"]))
    st = W.step(name, rb)
    Wd, H = W.META[name]["res"]
    pad = W.local_rows(H, rb) - H + 4
    assert pad > 4
    ref = fx(name)
    for schedule in ("tile", "wavefront", "tree"):
        ds = P.DeviceScene.from_host(hs)
        cam, kw, _ = request(hs, st, schedule)
        dev8 = torch.full((H + pad, Wd, 3), 0xA5, dtype=torch.uint8, device="cuda")
        devf = torch.full((H + pad, Wd, 3), -7.0, dtype=torch.float32, device="cuda")
        devh = torch.full((H + pad, Wd), -99, dtype=torch.int32, device="cuda")
        ds.render_device(cam, rgb8_ptr=dev8.data_ptr(), rgb32f_ptr=devf.data_ptr(), hit_ptr=devh.data_ptr(), **kw)
        ds.sync()
        assert ds.last_schedule() == schedule
        assert (dev8[H:] == 0xA5).all() and (devf[H:] == -7.0).all() and (devh[H:] == -99).all(), (name, schedule)
        same_frame({"rgb8": dev8[:H].cpu().numpy(), "rgb32f": devf[:H].cpu().numpy(), "hit_id": devh[:H].cpu().numpy()}, ref,
                   "%s device planes %s" % (name, schedule))
        ds.close()


# ---- d. de-interleave

@pytest.mark.parametrize("width", [64, 50])      # 192-byte rows take the 16-byte path, 150-byte rows the byte path
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("rb", [48, 80])
def test_deinterleave_with_row_blocks_that_are_no_power_of_two(rb, world, width):
    """p3d_deinterleave_frames and p3d_deinterleave against the row mapping restated in numpy (handle_walks.shard_rows), on
    random bytes; 200 rows end in a ragged block (8 rows of 48, 40 of 80)."""
    import torch
    H, B = 200, 2
    assert H % rb
    rows = W.local_rows(H, rb, world)
    rng = np.random.default_rng(rb * 1000 + world * 10 + width)
    host = rng.integers(0, 256, (world, B, rows, width, 3), dtype=np.uint8)
    want = np.zeros((B, H, width, 3), np.uint8)
    for r in range(world):
        for lr, y in W.shard_rows(H, rb, world, r):
            want[:, y] = host[r, :, lr]
    hs, ds = open_scene(W.ML_SCENE)
    gathered = torch.from_numpy(host).cuda()
    tile = rows * width * 3
    frames = torch.full((B, H, width, 3), 0x5A, dtype=torch.uint8, device="cuda")
    ds.deinterleave_frames(gathered.data_ptr(), frames.data_ptr(), width, H, rb, world, 3, B, rank_stride_bytes=B * tile, tile_stride_bytes=tile)
    ds.sync()
    assert np.array_equal(frames.cpu().numpy(), want)
    single = torch.full((H + 4, width, 3), 0x5A, dtype=torch.uint8, device="cuda")
    for f in range(B):
        ds.deinterleave(gathered[0, f].data_ptr(), single.data_ptr(), width, H, rb, world, 3, rank_stride_bytes=B * tile)
        ds.sync()
        assert np.array_equal(single[:H].cpu().numpy(), want[f]) and (single[H:] == 0x5A).all()
    ds.close()


# ---- e. the other entries between frames of one handle

def entry_refs():
    """What the oracle says of the other entries' calls on balls_high at 200x150, computed once: three orbit frames, the
    primary rays with the hit primitive's t and normal (oracle_py.intersect) and albedo (materials), rayTracing() of every
    7th of them, BVH::Traverse(Ray&) restated on 400 segments (tests/occlusion_refs.py), and the host's sample array."""
    if not _refs:
        src = scene_path(W.BH_SCENE)
        res = tuple(W.META[W.BIG]["res"])
        Wd, H = res
        with tempfile.TemporaryDirectory() as td:
            cams, orbit = [], []
            for e in eyes_around(src, 3):
                p = p3f_with_eye(src, e, td)
                hs = P.HostScene(p)
                hs.set_resolution(*res)
                cams.append(hs.camera())
                sc = O.Scene(p)
                sc.set_resolution(*res)
                orbit.append(sc.render(max_depth=4, accel=2, threads=THREADS))
        osc = O.Scene(src)
        osc.set_resolution(*res)
        hid = fx(W.BIG)["hit_id"]
        assert (hid >= 0).all()                                   # the floor fills the frame
        ptype, prim, pmat = osc.prims()
        rays = [osc.primary_ray(x + 0.5, y + 0.5) for y in range(H) for x in range(Wd)]       # rows bottom-up, pixel centres
        o, d = np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays])
        some = np.arange(0, H * Wd, 3)
        t, nrm = np.zeros(len(some), np.float32), np.zeros((len(some), 3), np.float32)
        for k, i in enumerate(some):
            j = int(hid.flat[i])
            h, t[k], nrm[k] = O.intersect(ptype[j], prim[j], o[i], d[i])
            assert h, i
        stream = np.arange(0, H * Wd, 7)
        colors = np.stack([osc.trace(2, o[i], d[i], max_depth=4) for i in stream])
        _, so, sd = R.segments(W.BH_SCENE, 400)
        shadow = np.array([osc.refbvh_shadow(so[i], sd[i]) for i in range(len(so))], np.uint8)
        assert 40 <= int(shadow.sum()) <= 360
        hs = P.HostScene(src)
        hs.set_resolution(*res)
        _refs.update(cams=cams, orbit=orbit, o=o, d=d, some=some, t=t, normal=nrm, albedo=osc.materials()[pmat[hid]][..., 0:3],
                     stream=stream, colors=colors, hit_id=hid, so=so, sd=sd, shadow=shadow, aperture=hs.camera().aperture,
                     samples=hs.samples(97, 2))
    return _refs


@pytest.mark.parametrize("schedule", SCHEDULES, ids=IDS)
def test_entries_alternate_on_one_handle(schedule):
    torch = pytest.importorskip("torch")
    ref = entry_refs()
    hs, ds = open_scene(W.BH_SCENE)
    cam, kw, forced = request(hs, W.step(W.BIG), schedule)
    force = {forced: True} if forced else {}
    Wd, H = W.META[W.BIG]["res"]
    n_frames = [0]

    def frame(after):
        out = ds.render(cam, **kw)
        if forced:
            assert ds.last_schedule() == forced
        check(out, W.BIG, "%s frame %d, after %s" % (schedule, n_frames[0], after))
        n_frames[0] += 1

    for rnd in range(2):
        frame("the start of round %d" % rnd)
        batch = ds.render_frames(ref["cams"], max_depth=4, accel=2, counters=True, **force)
        for f, want in enumerate(ref["orbit"]):
            same_frame({k: batch[k][f] for k in ("rgb8", "rgb32f", "hit_id")}, want, "render_frames round %d frame %d" % (rnd, f))
        for k in ("closest_queries", "shadow_queries", "rays"):
            assert batch["counters"][k] == sum(w["counters"][k] for w in ref["orbit"]), k
        frame("render_frames")

        aov = ds.render_aov(cam, max_depth=4, accel=2, **force)
        same_frame({k: aov[k][0] for k in ("rgb8", "rgb32f", "hit_id")}, fx(W.BIG), "render_aov round %d" % rnd)
        assert np.array_equal(bits(aov["depth"][0]).ravel()[ref["some"]], bits(ref["t"]))
        assert np.array_equal(bits(aov["normal"][0]).reshape(-1, 3)[ref["some"]], bits(ref["normal"]))
        assert np.array_equal(bits(aov["albedo"][0]), bits(ref["albedo"]))
        frame("render_aov")

        s = ref["stream"]
        got = ds.trace_rays(ref["o"][s], ref["d"][s], max_depth=4, accel=2)
        assert np.array_equal(bits(got["rgb32f"]), bits(ref["colors"])), int((bits(got["rgb32f"]) != bits(ref["colors"])).any(-1).sum())
        assert np.array_equal(got["hit_id"], ref["hit_id"].ravel()[s])
        both = np.intersect1d(s, ref["some"], return_indices=True)
        assert len(both[0]) > 1000
        assert np.array_equal(bits(got["t"])[both[1]], bits(ref["t"])[both[2]])
        assert np.array_equal(bits(got["normal"])[both[1]], bits(ref["normal"])[both[2]])
        frame("trace_rays")

        occ = ds.occluded(ref["so"], ref["sd"], accel=2)
        assert np.array_equal(occ, ref["shadow"]), int((occ != ref["shadow"]).sum())
        frame("occluded")

        n = ref["samples"].size
        buf = torch.full((n + 1024,), float("nan"), dtype=torch.float32, device="cuda")
        ds.generate_samples_device(buf.data_ptr(), 97, Wd, H, 2, ref["aperture"])
        host = buf.cpu().numpy()
        assert np.array_equal(bits(host[:n]), bits(ref["samples"]).ravel()) and np.isnan(host[n:]).all()
        frame("generate_samples")
    ds.close()


# ---- f. tuning changes mid-life

@pytest.mark.parametrize("schedule", SCHEDULES, ids=IDS)
def test_tuning_changes_between_frames(schedule):
    """p3d_set_tuning and p3d_set_primary_tiles on a live handle, two frames after each change.  xcd_chunk 4 turns the
    learned order of the wave-tile schedules off and back on.  workspace_mib 8: the wavefront queues of this frame (about
    780 bytes per pixel at depth 4, 160 x 208 padded pixels: 26 MB) are cut into bands, and the tile schedule's slots (0.2 MB
    each) are too few, so a forced tile frame runs banded too -- last_schedule() says wavefront; 65536 is the default budget."""
    hs, ds = open_scene(W.BH_SCENE)
    cam, kw, forced = request(hs, W.step(W.BIG), schedule)
    changes = [("as created", lambda: None),
               ("xcd_chunk 4", lambda: ds.set_tuning(xcd_chunk=4)), ("xcd_chunk 1", lambda: ds.set_tuning(xcd_chunk=1)),
               ("workspace 8 MiB", lambda: ds.set_tuning(workspace_mib=8)), ("workspace 64 GiB", lambda: ds.set_tuning(workspace_mib=65536)),
               ("primary_tiles 1", lambda: ds.set_primary_tiles(1)), ("primary_tiles 3", lambda: ds.set_primary_tiles(3)),
               ("primary_tiles 1 again", lambda: ds.set_primary_tiles(1))]
    for what, change in changes:
        change()
        for k in range(2):
            out = ds.render(cam, **kw)
            if forced:
                assert ds.last_schedule() == ("wavefront" if what == "workspace 8 MiB" and forced == "tile" else forced), what
            check(out, W.BIG, "%s, %s, frame %d" % (schedule, what, k))
    ds.close()
