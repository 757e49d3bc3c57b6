"""p3d_render_aov on the GPU: the depth, normal and albedo planes of a frame's primary hits.

The yardstick is never the new code: `depth` and `normal` must equal, as uint32 bit patterns, the `t` and `normal` that
p3d_trace_rays -- pinned bit for bit to the reference's object code (tests/test_gpu_trace_rays.py) -- returns for the same
primary rays, built with the oracle's primary_ray / primary_ray_lens at the pixel convention that test uses for frames
(x + 0.5, y + 0.5; rows bottom-up).  Independently of the stream, 200 pixels per case go through the oracle's intersect() of
the hit primitive.  `albedo` must equal floats 0..2 of the oracle's materials() row of the hit primitive.  Colours and
hit ids must be those of p3d_render_frames.  Tolerance 0 everywhere; nothing here is random but the fixed-seed pixel draw.
"""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

from conftest import RGB_TOL
from extra_scenes import scene_path
from oracle import oracle_py as O
import scene_motion as M
import u_4a_2s_p3d_raytracer_template2_amd as P
from u_4a_2s_p3d_raytracer_template2_amd import api

pytestmark = pytest.mark.gpu

assert RGB_TOL == 0.0
RES = (72, 40)          # a partial 16-pixel tile in x; 40 rows are no multiple of 16: the tile padding is exercised
DEPTH = 3
PAD = 16
SCHEDULES = {"wavefront": dict(wavefront=True), "tile": dict(tile=True), "tree": dict(tree=True)}
COLOUR = ("rgb8", "rgb32f", "hit_id")
PLANES = COLOUR + api.AOV_PLANES
WIDTH = {"rgb8": 3, "rgb32f": 3, "hit_id": 1, "depth": 1, "normal": 3, "albedo": 3}
DTYPE = {"rgb8": np.uint8, "rgb32f": np.float32, "hit_id": np.int32, "depth": np.float32, "normal": np.float32, "albedo": np.float32}
SENTINEL = {"rgb8": np.uint8(201), "rgb32f": np.float32(-12345.5), "hit_id": np.int32(-77), "depth": np.float32(-54321.25),
            "normal": np.float32(7.75), "albedo": np.float32(-3.125)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def same_bits(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = bits(got) != bits(ref)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %s vs %s" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])


def cams_of(cam_or_cams):
    return [cam_or_cams] if isinstance(cam_or_cams, api.Camera) else list(cam_or_cams)


def raw_aov(ds, cam_or_cams, aov=api.AOV_PLANES, colour=COLOUR, spp=0, samples=None, rank=0, world=1, max_depth=DEPTH,
            device=False, **switches):
    """p3d_render_aov through ctypes into planes PAD entries longer than the call may write, pre-filled with a sentinel;
    planes not named are passed as NULL (aov=None: the whole p3d_aov_outputs pointer is NULL).  device: the planes are
    caller-allocated device buffers (memory = 1), uploaded with the sentinel before and downloaded after the call.
    -> {plane: (n, rows, W[, 3])} of every plane, written or not; asserts that the sentinel survives past the end of each."""
    cams = cams_of(cam_or_cams)
    arr, n = api._camera_array(cams)
    W, H = cams[0].res_x, cams[0].res_y
    rows = H if world == 1 else P.local_rows(H, 16, world)
    npx = n * rows * W
    buf = {k: np.full((npx + PAD) * WIDTH[k], SENTINEL[k], DTYPE[k]) for k in PLANES}
    named = set(colour) | set(aov or ())
    L = P.lib()
    dev = {}
    if device:
        for k in named:
            p = C.c_void_p()
            assert L.p3d_device_alloc(ds.h, buf[k].nbytes, C.byref(p)) == 0
            assert L.p3d_upload(ds.h, p, buf[k].ctypes.data, buf[k].nbytes) == 0
            dev[k] = p.value
    ptr = lambda k: (dev[k] if device else buf[k].ctypes.data) if k in named else None
    if samples is not None:
        samples = np.ascontiguousarray(samples, np.float32)
    prm = ds._params(max_depth, api.ACCEL_BVH, spp, samples, rank, world, 16, False, **switches)
    out = api.Outputs(ptr("rgb8"), ptr("rgb32f"), ptr("hit_id"), 1 if device else 0)
    a = api.AovOutputs(*[ptr(k) for k in api.AOV_PLANES])
    rc = L.p3d_render_aov(ds.h, arr, n, C.byref(prm), C.byref(out), C.byref(a) if aov is not None else None)
    assert rc == 0, L.p3d_last_error()
    if device:
        ds.sync()
        for k in named:
            assert L.p3d_download(ds.h, buf[k].ctypes.data, dev[k], buf[k].nbytes) == 0
            L.p3d_device_free(ds.h, C.c_void_p(dev[k]))
    res = {}
    for k in PLANES:
        assert (buf[k][npx * WIDTH[k]:] == SENTINEL[k]).all(), "%s was written past its end" % k
        if k not in named:
            assert (buf[k] == SENTINEL[k]).all(), "%s was passed as NULL and written" % k
        res[k] = buf[k][:npx * WIDTH[k]].reshape((n, rows, W) + ((3,) if WIDTH[k] == 3 else ()))
    return res


_cache = {}
# The eye of balls_low and balls_medium (2.1 1.3 1.7) looks down at their floor, which fills the frame: no pixel misses.
# Every case needs hit AND miss pixels, so these two are rendered through a copy of the file whose eye sits lower and sees
# the horizon; the oracle and the host layer both load that copy, so both build the same camera.
LOW_EYE = {"balls_low": "from 2.1 1.3 0.1", "balls_medium": "from 2.1 1.3 0.1"}


def scene_file(name):
    if name not in LOW_EYE:
        return scene_path(name)
    if "tmp" not in _cache:                  # (made by the first test that needs a copy, removed with the process)
        _cache["tmp"] = tempfile.TemporaryDirectory()
    out = os.path.join(_cache["tmp"].name, name + "_low_eye.p3f")
    if not os.path.exists(out):
        with open(scene_path(name)) as f:
            lines = [LOW_EYE[name] if l.startswith("from ") else l for l in f.read().splitlines()]
        assert LOW_EYE[name] in lines
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return out


def handles(name, res=RES):
    """(HostScene at res, oracle scene at res, one device handle) of a scene, made once."""
    key = ("scene", name, res)
    if key not in _cache:
        hs = P.HostScene(scene_file(name))
        hs.set_resolution(*res)
        osc = O.Scene(scene_file(name))
        osc.set_resolution(*res)
        _cache[key] = (hs, osc, P.DeviceScene.from_host(hs))
    return _cache[key]


def primary_rays(osc, res, samples=None):
    """Every pixel's primary ray from the oracle, rows bottom-up: pixel centres, or sample 0 of the given sample array."""
    key = ("rays", id(osc), res, None if samples is None else samples.tobytes())
    if key not in _cache:
        W, H = res
        if samples is None:
            rays = [osc.primary_ray(x + 0.5, y + 0.5) for y in range(H) for x in range(W)]
        else:
            s0 = samples[:, :, 0, :]            # pixel x, y, lens x, lens y
            rays = [osc.primary_ray_lens(s0[y, x, 2], s0[y, x, 3], s0[y, x, 0], s0[y, x, 1]) for y in range(H) for x in range(W)]
        _cache[key] = (np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays]))
    return _cache[key]


def stream_reference(name, res=RES, samples=None, ds=None, **mode):
    """What p3d_trace_rays returns for the frame's primary rays, as (H, W[, 3]) planes, computed once per configuration."""
    key = ("stream", name, res, tuple(sorted(mode.items())), None if samples is None else samples.tobytes(), id(ds))
    if key not in _cache:
        _, osc, own = handles(name, res)
        o, d = primary_rays(osc, res, samples)
        got = (ds or own).trace_rays(o, d, max_depth=DEPTH, accel=api.ACCEL_BVH, want=("hit_id", "t", "normal"), **mode)
        W, H = res
        _cache[key] = {"hit_id": got["hit_id"].reshape(H, W), "t": got["t"].reshape(H, W), "normal": got["normal"].reshape(H, W, 3),
                       "o": o.reshape(H, W, 3), "d": d.reshape(H, W, 3)}
        for v in _cache[key].values():
            v.setflags(write=False)
    return _cache[key]


def check_planes(got, ref, osc, what, frame=0, pixels=200):
    """The checks of case 1 on frame `frame` of `got` against the stream's `ref` and the oracle's tables."""
    hid, depth, normal, albedo = got["hit_id"][frame], got["depth"][frame], got["normal"][frame], got["albedo"][frame]
    hit = hid >= 0
    assert hit.sum() >= 50 and (~hit).sum() >= 50, "%s: hit and miss pixels are both needed (%d / %d)" % (what, hit.sum(), (~hit).sum())
    assert ((hid == -1) | hit).all()
    same_bits(hid, ref["hit_id"], what + " hit_id against the stream's")
    same_bits(depth, ref["t"], what + " depth against the stream's t")
    assert np.isposinf(depth[~hit]).all() and np.isfinite(depth[hit]).all()
    same_bits(normal, ref["normal"], what + " normal against the stream's")
    assert (bits(normal[~hit]) == 0).all()
    ptype, prim, pmat = osc.prims()
    mats = osc.materials()
    want = np.zeros(albedo.shape, np.float32)
    want[hit] = mats[pmat[hid[hit]]][:, 0:3]
    same_bits(albedo, want, what + " albedo against materials[prim_material[hit_id]][0:3]")
    assert len(np.unique(want[hit], axis=0)) >= 2, "one colour everywhere shows little"
    # independently of the stream: the oracle's intersector on the hit primitive
    H, W = hid.shape
    rng = np.random.default_rng(2024)
    n_hit = 0
    for i in rng.choice(H * W, pixels, replace=False):
        y, x = divmod(int(i), W)
        if not hit[y, x]:
            continue
        j = int(hid[y, x])
        h, t, n = O.intersect(ptype[j], prim[j], ref["o"][y, x], ref["d"][y, x])
        assert h, (what, x, y, j)
        assert bits(np.float32(t)) == bits(depth[y, x]), (what, x, y, j, t, depth[y, x])
        assert (bits(n) == bits(normal[y, x])).all(), (what, x, y, j, n, normal[y, x])
        n_hit += 1
    assert n_hit >= 20, n_hit


# ---- 1. the planes against the ray stream and the oracle's intersectors

@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("name", ["balls_low", "balls_box", "balls_medium", "mount_low"])
def test_planes_equal_the_ray_stream(name, sched):
    hs, osc, ds = handles(name)
    got = raw_aov(ds, hs.camera(), **SCHEDULES[sched])
    assert ds.last_schedule() == sched
    check_planes(got, stream_reference(name), osc, "%s %s" % (name, sched))


def test_scenes_cover_every_primitive_kind():
    kinds = set()
    for name in ("balls_low", "balls_box", "balls_medium", "mount_low"):
        hs, osc, ds = handles(name)
        hid = raw_aov(ds, hs.camera(), aov=("depth",), wavefront=True)["hit_id"][0]
        kinds |= set(int(k) for k in osc.prims()[0][hid[hid >= 0]])
    assert kinds == {O.SPHERE, O.TRIANGLE, O.BOX, O.PLANE}, kinds


# ---- 2. colours untouched, NULL planes untouched, nothing written past the end

@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("name", ["balls_low", "balls_box", "balls_medium", "mount_low"])
def test_colours_are_those_of_render_frames(name, sched):
    hs, _, ds = handles(name)
    cam = hs.camera()
    ref = ds.render_frames([cam], max_depth=DEPTH, **SCHEDULES[sched])
    full = raw_aov(ds, cam, **SCHEDULES[sched])
    for aov in (None, ("depth",), ("albedo",), api.AOV_PLANES):
        got = full if aov == api.AOV_PLANES else raw_aov(ds, cam, aov=aov, **SCHEDULES[sched])
        for k in COLOUR:
            same_bits(got[k], ref[k], "%s %s aov=%s: %s" % (name, sched, aov, k))
        for k in aov or ():
            same_bits(got[k], full[k], "%s %s aov=%s: %s" % (name, sched, aov, k))
    # the Python entry is the same call
    py = ds.render_aov(cam, max_depth=DEPTH, **SCHEDULES[sched])
    for k in PLANES:
        same_bits(py[k], full[k], "render_aov %s" % k)
    only = ds.render_aov(cam, max_depth=DEPTH, want=("normal",), **SCHEDULES[sched])
    assert set(only) == set(COLOUR) | {"normal"}


# ---- 3. a scene read from HBM: shared (Hit merged through LDS) and private walks

@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("private_walk", [False, True], ids=["shared", "private"])
def test_scene_read_from_hbm(private_walk, sched):
    hs, osc, ds = handles("mount_low")
    got = raw_aov(ds, hs.camera(), no_lds=True, private_walk=private_walk, **SCHEDULES[sched])
    assert ds.last_schedule() == sched
    ref = stream_reference("mount_low", no_lds=True, private_walk=private_walk)
    check_planes(got, ref, osc, "mount_low from HBM private=%s %s" % (private_walk, sched))
    for k in ("hit_id", "t", "normal"):
        same_bits(ref[k], stream_reference("mount_low")[k], "the stream itself, HBM against LDS: " + k)


# ---- 4. samples: the planes describe sample 0's primary ray

@pytest.mark.parametrize("sched", ["tile", "wavefront"])
def test_samples_describe_sample_0(sched):
    res = (48, 32)
    hs, osc, ds = handles("dof", res)
    assert hs.camera().aperture > 0
    samples = hs.samples(31, 2)
    got = raw_aov(ds, hs.camera(), spp=2, samples=samples, **SCHEDULES[sched])
    assert ds.last_schedule() == sched
    ref = stream_reference("dof", res, samples)
    assert (bits(ref["o"]) != bits(stream_reference("dof", res)["o"])).any(), "the lens must move the ray origins"
    check_planes(got, ref, osc, "dof spp 2 %s" % sched)
    frames = ds.render_frames([hs.camera()], max_depth=DEPTH, spp=2, samples=samples[None], **SCHEDULES[sched])
    for k in COLOUR:
        same_bits(got[k], frames[k], "dof spp 2 %s: %s" % (sched, k))


# ---- 5. sharding and batches

def stitch(ds, shards, res, world, n=1):
    """p3d_deinterleave[_frames] of the ranks' planes (each (n, rows, W[, 3])) on the device -> (n, H, W[, 3])."""
    W, H = res
    L = P.lib()
    out = {}
    for k in shards[0]:
        bpp = WIDTH[k] * DTYPE[k]().itemsize
        tile = np.ascontiguousarray(np.stack([s[k] for s in shards]))         # [rank][frame][rows][W]: ranks back to back
        full = np.full((n, H, W) + ((3,) if WIDTH[k] == 3 else ()), SENTINEL[k], DTYPE[k])
        g, f = C.c_void_p(), C.c_void_p()
        assert L.p3d_device_alloc(ds.h, tile.nbytes, C.byref(g)) == 0 and L.p3d_device_alloc(ds.h, full.nbytes, C.byref(f)) == 0
        assert L.p3d_upload(ds.h, g, tile.ctypes.data, tile.nbytes) == 0
        if n == 1:
            ds.deinterleave(g.value, f.value, W, H, 16, world, bpp)
        else:
            ds.deinterleave_frames(g.value, f.value, W, H, 16, world, bpp, n, rank_stride_bytes=tile[0].nbytes,
                                   tile_stride_bytes=tile[0, 0].nbytes)
        ds.sync()
        assert L.p3d_download(ds.h, full.ctypes.data, f, full.nbytes) == 0
        L.p3d_device_free(ds.h, g); L.p3d_device_free(ds.h, f)
        out[k] = full
    return out


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
def test_two_ranks_stitch_to_the_whole_frame(sched):
    hs, _, ds = handles("balls_box")
    whole = raw_aov(ds, hs.camera(), **SCHEDULES[sched])
    assert P.local_rows(RES[1], 16, 2) == 32
    # (caller-allocated device planes: the kernels' own stores are what is seen; a host plane is copied back whole)
    shards = [raw_aov(ds, hs.camera(), rank=r, world=2, device=True, **SCHEDULES[sched]) for r in range(2)]
    # rank 1's second row block lies past the image: never written
    for k in PLANES:
        assert (shards[1][k][0, 16:] == SENTINEL[k]).all(), "rows past the image were written: " + k
    got = stitch(ds, shards, RES, 2)
    for k in PLANES:
        same_bits(got[k], whole[k], "world 2 stitched %s: %s" % (sched, k))


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
def test_batch_of_an_orbit(sched):
    hs, _, ds = handles("balls_box")
    cams = hs.orbit_cameras(3, 25.0)
    batch = raw_aov(ds, cams, **SCHEDULES[sched])
    for f, cam in enumerate(cams):
        one = raw_aov(ds, cam, **SCHEDULES[sched])
        for k in PLANES:
            same_bits(batch[k][f], one[k][0], "frame %d of the batch %s: %s" % (f, sched, k))
    assert (bits(batch["depth"][0]) != bits(batch["depth"][2])).any(), "the orbit must show"
    if sched == "wavefront":
        shards = [raw_aov(ds, cams, rank=r, world=2, **SCHEDULES[sched]) for r in range(2)]
        got = stitch(ds, shards, RES, 2, n=3)
        for k in PLANES:
            same_bits(got[k], batch[k], "the batch on two ranks, stitched: " + k)


# ---- 6. device memory equals host memory

@pytest.mark.parametrize("sched", sorted(SCHEDULES))
def test_device_planes_equal_host_planes(sched):
    hs, _, ds = handles("balls_medium")
    host = raw_aov(ds, hs.camera(), **SCHEDULES[sched])
    devp = raw_aov(ds, hs.camera(), device=True, **SCHEDULES[sched])
    for k in PLANES:
        same_bits(devp[k], host[k], "memory 1 against memory 0 %s: %s" % (sched, k))
    part = raw_aov(ds, hs.camera(), device=True, aov=("normal",), colour=("rgb8",), **SCHEDULES[sched])
    same_bits(part["normal"], host["normal"], "normal alone")
    same_bits(part["rgb8"], host["rgb8"], "rgb8 alone")


# ---- 7. a frame in bands (the budget and resolution of test_gpu_parity.test_wavefront_bands_do_not_change_the_image)

def test_banded_frame():
    hs = P.HostScene(scene_path("mount_low"))
    hs.set_resolution(256, 144)
    ds = P.DeviceScene.from_host(hs)
    full = raw_aov(ds, hs.camera(), max_depth=4, wavefront=True)
    ds.set_tuning(workspace_mib=8)          # a row of 16x16 tiles needs 3.2 MB at depth 4: two tile rows per band
    banded = raw_aov(ds, hs.camera(), max_depth=4, wavefront=True)
    assert ds.last_schedule() == "wavefront"
    hit = full["hit_id"] >= 0
    assert hit[0, :72].any() and hit[0, 72:].any() and (~hit).any(), "hits in more than one band are needed"
    for k in PLANES:
        same_bits(banded[k], full[k], "banded " + k)
    ds.close()


# ---- 8. after p3d_scene_update

def test_planes_follow_a_scene_update(tmp_path):
    a, b = scene_path("balls_low"), str(tmp_path / "moved.p3f")
    ha = P.HostScene(a)
    ptype, data = ha.arrays()[:2]
    lo, hi, bounded = M.bounds(ptype, data)
    spheres = np.flatnonzero((ptype == 0) & bounded)
    three = set(int(i) for i in spheres[np.argsort(-(hi - lo).prod(-1)[spheres])[:3]])       # the three largest: they show
    M.rewrite_p3f(a, b, lambda kind, k, v: M.shift_out_of_own_box(kind, v) if kind == "s" and k in three else None)
    hb = P.HostScene(b)
    ha.set_resolution(*RES); hb.set_resolution(*RES)
    data_b = hb.arrays()[1]
    moved = np.flatnonzero((bits(data) != bits(data_b)).any(-1))
    assert set(int(i) for i in moved) == three
    M.assert_boxes_disjoint(ptype, data, data_b, moved)
    ds, fresh = P.DeviceScene.from_host(ha), P.DeviceScene.from_host(hb)
    before = raw_aov(ds, ha.camera(), wavefront=True)
    ds.update(data_b[moved], indices=moved)
    for sched in sorted(SCHEDULES):
        got, ref = raw_aov(ds, ha.camera(), **SCHEDULES[sched]), raw_aov(fresh, hb.camera(), **SCHEDULES[sched])
        for k in PLANES:
            same_bits(got[k], ref[k], "updated handle against a fresh one %s: %s" % (sched, k))
        assert (bits(before["depth"]) != bits(got["depth"])).mean() >= 0.02, "the move must show in the depth plane"
        assert (bits(before["normal"]) != bits(got["normal"])).any() and (before["hit_id"] != got["hit_id"]).any()
    ds.close(); fresh.close()


# ---- 9. handle state: AOV planes are part of no cache key

def test_aov_calls_share_the_measured_schedule_choice():
    hs = P.HostScene(scene_path("mount_low"))
    hs.set_resolution(*RES)
    ds, plain = P.DeviceScene.from_host(hs), P.DeviceScene.from_host(hs)
    cam = hs.camera()
    for k in range(14):                     # 2 x 6 measuring frames of the configuration, then the choice
        settled = ds.render(cam, max_depth=DEPTH, no_lds=True)
    chosen = ds.last_schedule()
    for k in range(3):
        got = raw_aov(ds, cam, no_lds=True)
        assert ds.last_schedule() == chosen, "an AOV call re-measured or re-keyed the schedule choice"
        for p in COLOUR:
            same_bits(got[p][0], settled[p], "the AOV call's colours: " + p)
        again = ds.render(cam, max_depth=DEPTH, no_lds=True)
        assert ds.last_schedule() == chosen
        for p in COLOUR:
            same_bits(again[p], settled[p], "the frame after an AOV call: " + p)
    # ... and while a handle is still measuring: only the frames WITHOUT planes measure.  They run the fixed sequence of
    # candidates (each twice) whatever happens in between; a call with planes in between uses the choice already made --
    # none yet: the tile schedule -- and advances nothing.
    for j in range(12):
        plain.render(cam, max_depth=DEPTH, no_lds=True)
        assert plain.last_schedule() == ("wavefront", "tree", "tile")[(j // 2) % 3], (j, plain.last_schedule())
        if j < 11:
            during = raw_aov(plain, cam, no_lds=True)
            assert plain.last_schedule() == "tile", (j, plain.last_schedule())
            for p in PLANES:
                same_bits(during[p], got[p], "a call with planes between measuring frames: " + p)
    check_planes(got, stream_reference("mount_low", no_lds=True), handles("mount_low")[1], "measured schedule " + chosen)
    ds.close(); plain.close()


def test_primary_tiles_report_the_truth():
    """The multi-tile level-1 kernels have no build that writes the planes: a frame with planes runs one tile per workgroup
    and says so; the frames around it keep what was set."""
    hs, osc, _ = handles("balls_box")
    ds = P.DeviceScene.from_host(hs)
    ref = raw_aov(ds, hs.camera(), wavefront=True)
    for tiles in (1, 2, 3):
        ds.set_primary_tiles(tiles)
        ds.render(hs.camera(), max_depth=DEPTH, wavefront=True)
        plain = ds.last_primary_tiles()
        got = raw_aov(ds, hs.camera(), wavefront=True)
        assert plain == tiles and ds.last_primary_tiles() == 1
        ds.render(hs.camera(), max_depth=DEPTH, wavefront=True)
        assert ds.last_primary_tiles() == tiles
        assert raw_aov(ds, hs.camera(), aov=None, wavefront=True) and ds.last_primary_tiles() == tiles, "no planes: p3d_render_frames exactly"
        for k in PLANES:
            same_bits(got[k], ref[k], "%d tiles per workgroup: %s" % (tiles, k))
    ds.close()


# ---- 10. the host layer and the command line: p3d_render --aov PREFIX

def test_cli_writes_the_planes_as_npy(tmp_path):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(P.__file__), "p3d_render")
    hs, _, ds = handles("balls_box")
    r = subprocess.run([exe, scene_path("balls_box"), "--res", str(RES[0]), str(RES[1]), "--depth", str(DEPTH), "--out",
                        str(tmp_path / "img.ppm"), "--aov", str(tmp_path / "box")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert hs.spp == 0
    ref = ds.render_aov(hs.camera(), max_depth=DEPTH, accel=hs.accel)
    for k in api.AOV_PLANES:
        got = np.load(tmp_path / ("box_%s.npy" % k))
        assert got.dtype == np.float32
        same_bits(got, ref[k][0], "p3d_render --aov: " + k)
