"""p3d_ambient_occlusion on the GPU: the fused kernel against the unfused pipeline the definition names -- the NumPy segments
(tests/ao_reference.py) fed to DeviceScene.occluded on the same handle, counted with NumPy, resolved by the restatement -- and
against the reference's own traversals through the oracle.  Every pixel comparison is an equality of bits; every output is
allocated with PAD elements of sentinel on either side, which must stay untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ao_reference as R                                   # noqa: E402
import occlusion_refs as OR                                # noqa: E402
import test_gpu_scene_update as SU                         # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P            # noqa: E402
from extra_scenes import scene_path                        # noqa: E402
from plane_memory import check_host_device_split          # noqa: E402
from oracle import oracle_py as O                          # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api        # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT, ERR_STATE = -1, -4, -5
F = np.float32
MODES = {"lds": dict(), "hbm": dict(no_lds=True), "hbm_private": dict(no_lds=True, private_walk=True)}
RES = (24, 16)
RADIUS, BIAS, SEED = 0.5, 0.001, 77
PAD = 16
SENTINEL = F(-12345.0)


def same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = got.view(np.uint32) != ref.view(np.uint32) if got.dtype == np.float32 else got != ref
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


@pytest.fixture(scope="module")
def scenes():
    """scenes(name, res=RES, n=1) -> (handle, cameras, planes): one device handle per scene for the whole module, and the
    frames of render_aov through n orbit cameras (n == 1: the scene's own) at res, rendered once and never modified."""
    made, frames = {}, {}

    def get(name, res=RES, n=1):
        if name not in made:
            made[name] = P.DeviceScene.from_host(P.HostScene(scene_path(name)))
        k = (name, res, n)
        if k not in frames:
            hs = P.HostScene(scene_path(name))
            hs.set_resolution(*res)
            cams = [hs.camera()] if n == 1 else hs.orbit_cameras(n, 7.0)
            f = made[name].render_aov(cams, max_depth=2, accel=api.ACCEL_BVH)
            for a in f.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            frames[k] = (cams, f)
        return (made[name],) + frames[k]
    yield get
    for ds in made.values():
        ds.close()


def padded(shape):
    a = np.full(int(np.prod(shape)) + 2 * PAD, SENTINEL, F)
    return a, a[PAD:-PAD].reshape(shape)


def untouched(whole):
    return bool((whole[:PAD] == SENTINEL).all() and (whole[-PAD:] == SENTINEL).all())


def fused(ds, cams, depth, normal, rgb=None, samples=8, seed=SEED, accel=api.ACCEL_BVH, want=("ao", "rgb32f"), radius=RADIUS, bias=BIAS,
          prm_edit=None, ao_edit=None, in_edit=None, out_edit=None, n=None, **mode):
    """p3d_ambient_occlusion through ctypes on host planes, outputs padded with SENTINEL -> (status, {"ao", "rgb32f"}); the
    padding is checked here."""
    arr, n_cams = api._camera_array(cams)
    H, W = arr[0].res_y, arr[0].res_x
    depth = np.ascontiguousarray(depth, F).reshape(n_cams, H, W)
    normal = np.ascontiguousarray(normal, F).reshape(n_cams, H, W, 3)
    rgb = None if rgb is None else np.ascontiguousarray(rgb, F).reshape(n_cams, H, W, 3)
    whole_ao, ao = padded((n_cams, H, W))
    whole_rgb, out_rgb = padded((n_cams, H, W, 3))
    prm = ds._ray_params(1, accel, mode.get("no_lds", False), mode.get("private_walk", False), False)
    a = api.AoParams(int(samples), radius, bias, int(seed) & 0xFFFFFFFF)
    i = api.AoInputs(depth.ctypes.data, normal.ctypes.data, rgb.ctypes.data if rgb is not None else None, 0)
    o = api.AoOutputs(ao.ctypes.data if "ao" in want else None, out_rgb.ctypes.data if "rgb32f" in want else None, 0)
    for edit, x in ((prm_edit, prm), (ao_edit, a), (in_edit, i), (out_edit, o)):
        if edit:
            edit(x)
    rc = P.lib().p3d_ambient_occlusion(ds.h, arr, n_cams if n is None else n, C.byref(prm), C.byref(a), C.byref(i), C.byref(o))
    assert untouched(whole_ao) and untouched(whole_rgb), "written outside an output plane"
    return rc, {"ao": ao, "rgb32f": out_rgb}


def fused_ok(*args, **kw):
    rc, out = fused(*args, **kw)
    assert rc == 0, P.lib().p3d_last_error()
    return out


def frame_segments(cams, depth, normal, samples, seed, radius=RADIUS, bias=BIAS):
    """The NumPy segments of every frame: [(origin, dir, valid)] with frame f keyed by seed + f."""
    return [R.segments(cams[f], depth[f], normal[f], samples, radius, bias, seed, f) for f in range(len(cams))]


def counts_from(answer, segs, samples):
    """Per-pixel counts (n, H, W) from answer(o [m, 3], d [m, 3]) -> m answers, asked for the segments of valid pixels only."""
    out = []
    for o, d, v in segs:
        m = v.astype(bool)
        full = np.zeros(m.shape + (samples,), np.int32)
        if m.any():
            full[m] = np.asarray(answer(o[m].reshape(-1, 3), d[m].reshape(-1, 3))).reshape(-1, samples)
        out.append(full.sum(-1).astype(np.int32))
    return np.stack(out)


def unfused(ds, cams, depth, normal, rgb=None, samples=8, seed=SEED, accel=api.ACCEL_BVH, radius=RADIUS, bias=BIAS, **mode):
    segs = frame_segments(cams, depth, normal, samples, seed, radius, bias)
    occ = counts_from(lambda o, d: ds.occluded(o, d, accel=accel, **mode), segs, samples)
    return R.resolve(occ, samples, rgb), occ


def same_result(got, ref, what):
    same_bits(got["ao"], ref["ao"], what + " ao")
    same_bits(got["rgb32f"], ref["rgb32f"], what + " rgb32f")


# ---- 1. fused equals unfused

@pytest.mark.parametrize("samples", [1, 8, 64])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("name", ["balls_box", "mount_low", "balls_low"])
def test_fused_equals_unfused(name, accel, mode, samples, scenes):
    ds, cams, f = scenes(name)
    ref, occ = unfused(ds, cams, f["depth"], f["normal"], f["rgb32f"], samples, accel=accel, **MODES[mode])
    got = fused_ok(ds, cams, f["depth"], f["normal"], f["rgb32f"], samples, accel=accel, **MODES[mode])
    same_result(got, ref, "%s accel %d %s S=%d" % (name, accel, mode, samples))
    hit = np.isfinite(f["depth"])
    assert hit.any() and (got["ao"][~hit] == 1).all()
    if samples >= 8:
        assert occ.max() > 0 and (occ[hit] == 0).any(), "occluded and open pixels must both occur"


# ---- 2. against the reference's traversals directly

def oracle_counts(name, accel, segs, samples=8):
    osc = O.Scene(scene_path(name))
    if accel == 0:
        ptype, prim, _ = osc.prims()
        answer = lambda o, d: OR.brute_force(ptype, prim, o, d, bounded=False)
    else:
        fn = osc.refbvh_shadow if accel == 2 else osc.refgrid_shadow
        answer = lambda o, d: np.array([fn(a, b) for a, b in zip(o, d)], np.uint8)
    return counts_from(answer, segs, samples)


@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("name", ["balls_box", "mount_low", "balls_low"])
def test_counts_equal_the_references_traversals(name, accel, scenes):
    ds, cams, f = scenes(name)
    segs = frame_segments(cams, f["depth"], f["normal"], 8, SEED)
    occ = oracle_counts(name, accel, segs)
    got = fused_ok(ds, cams, f["depth"], f["normal"], None, 8, accel=accel)
    same_result(got, R.resolve(occ, 8), "%s accel %d against the oracle" % (name, accel))


def test_balls_box_is_not_trivial(scenes):
    """The conditions of the issue, on the reference's answers alone (accel 2, S = 8, radius 0.5, bias 0.001), and NONE mode's
    missing distance bound showing on at least 30 samples."""
    ds, cams, f = scenes("balls_box")
    segs = frame_segments(cams, f["depth"], f["normal"], 8, SEED)
    hit = segs[0][2].astype(bool)
    bvh, none = oracle_counts("balls_box", 2, segs)[0], oracle_counts("balls_box", 0, segs)[0]
    assert (~hit).any() and hit.any(), "some pixels miss"
    share = bvh[hit].sum() / (8.0 * hit.sum())
    assert 0.1 < share < 0.35, share
    assert len(np.unique(bvh[hit])) >= 5
    got = {a: fused_ok(ds, cams, f["depth"], f["normal"], None, 8, accel=a, want=("ao",))["ao"][0] for a in (0, 2)}
    open_ = lambda ao: np.rint(ao * 8).astype(np.int64)
    assert np.abs(open_(got[2]) - open_(got[0]))[hit].sum() >= 30 and np.abs(none - bvh).sum() >= 30


# ---- 3. scenes read from HBM natively

@pytest.mark.parametrize("private_walk", [False, True], ids=["shared", "private"])
@pytest.mark.parametrize("accel", [1, 2])
def test_mount_high_equals_the_references_traversals(accel, private_walk, scenes):
    ds, cams, f = scenes("mount_high")
    assert ds.stats()["n_triangles"] > 2000
    segs = frame_segments(cams, f["depth"], f["normal"], 8, SEED)
    occ = oracle_counts("mount_high", accel, segs)
    assert occ.max() > 0
    got = fused_ok(ds, cams, f["depth"], f["normal"], None, 8, accel=accel, private_walk=private_walk)
    same_result(got, R.resolve(occ, 8), "mount_high accel %d private %s" % (accel, private_walk))


def test_dragon_equals_p3d_occluded(scenes):
    """Against DeviceScene.occluded only.  At 24 x 16 the dragon is a few pixels on a large floor and segments of 0.5 find
    nothing to hit, so the longer radius is what makes the walks return both answers; only the equality is asserted."""
    ds, cams, f = scenes("dragon")
    assert np.isfinite(f["depth"]).any(), "the frame must hold queries"
    for radius in (0.5, 4.0):
        for private_walk in (False, True):
            ref, occ = unfused(ds, cams, f["depth"], f["normal"], f["rgb32f"], 8, radius=radius, private_walk=private_walk)
            print("dragon radius %g private %s: %d of %d samples occluded" % (radius, private_walk, int(occ.sum()), 8 * int(np.isfinite(f["depth"]).sum())))
            assert radius < 4.0 or 0 < occ.sum() < 8 * int(np.isfinite(f["depth"]).sum()), "p3d_occluded must give both answers at radius 4"
            got = fused_ok(ds, cams, f["depth"], f["normal"], f["rgb32f"], 8, radius=radius, private_walk=private_walk)
            same_result(got, ref, "dragon radius %g private %s" % (radius, private_walk))


# ---- 4. shapes: res_x below 64 / S, no multiple of it, one row; a batch

@pytest.mark.parametrize("samples", [1, 16, 64])
@pytest.mark.parametrize("res", [(1, 1), (7, 3), (9, 2), (63, 1), (65, 2), (23, 5)], ids=lambda r: "%dx%d" % r)
def test_shapes(res, samples, scenes):
    ds, cams, f = scenes("balls_low", res)                 # every pixel of balls_low hits: row tails hold queries
    for mode in ("lds", "hbm"):
        ref, _ = unfused(ds, cams, f["depth"], f["normal"], f["rgb32f"], samples, **MODES[mode])
        same_result(fused_ok(ds, cams, f["depth"], f["normal"], f["rgb32f"], samples, **MODES[mode]), ref, "%dx%d S=%d %s" % (res + (samples, mode)))


@pytest.mark.parametrize("mode", ["lds", "hbm"])
def test_a_batch_is_its_frames_with_seed_plus_f(mode, scenes):
    ds, cams, f = scenes("balls_box", (23, 5), 3)
    assert (f["depth"][0].view(np.uint32) != f["depth"][2].view(np.uint32)).any(), "the orbit must show"
    batch = fused_ok(ds, cams, f["depth"], f["normal"], f["rgb32f"], 16, **MODES[mode])
    ref, _ = unfused(ds, cams, f["depth"], f["normal"], f["rgb32f"], 16, **MODES[mode])
    same_result(batch, ref, "batch")
    for k in range(3):
        one = fused_ok(ds, [cams[k]], f["depth"][k], f["normal"][k], f["rgb32f"][k], 16, seed=SEED + k, **MODES[mode])
        same_bits(one["ao"][0], batch["ao"][k], "frame %d alone: ao" % k)
        same_bits(one["rgb32f"][0], batch["rgb32f"][k], "frame %d alone: rgb32f" % k)
    assert (batch["ao"][0].view(np.uint32) != fused_ok(ds, [cams[0]], f["depth"][0], f["normal"][0], None, 16, seed=SEED + 1)["ao"][0].view(np.uint32)).any()


# ---- 5. outputs, memory, capture

def test_output_planes_and_the_denoiser(scenes):
    ds, cams, f = scenes("balls_box")
    ref_c, _ = unfused(ds, cams, f["depth"], f["normal"], f["rgb32f"], 8)
    ref_n, _ = unfused(ds, cams, f["depth"], f["normal"], None, 8)
    for rgb, ref in ((f["rgb32f"], ref_c), (None, ref_n)):
        for want in (("ao",), ("rgb32f",), ("ao", "rgb32f")):
            got = fused_ok(ds, cams, f["depth"], f["normal"], rgb, 8, want=want)
            for k in ("ao", "rgb32f"):
                if k in want:
                    same_bits(got[k], ref[k], "want %s colour %s: %s" % (want, rgb is not None, k))
                else:
                    assert (got[k] == SENTINEL).all(), "a plane that was not asked for was written"
    same_bits(ref_n["rgb32f"], np.repeat(ref_n["ao"][..., None], 3, -1), "(ao, ao, ao)")
    # the pipeline connects: the plane is a colour p3d_denoise takes
    plane = fused_ok(ds, cams, f["depth"], f["normal"], None, 8)["rgb32f"]
    got = ds.denoise(plane, f["depth"], f["normal"], f["albedo"], iterations=2)
    ref = api.host_denoise(plane, f["depth"], f["normal"], f["albedo"], iterations=2)
    same_bits(got["rgb32f"], ref["rgb32f"], "denoised ambient occlusion")


def test_host_and_device_memory_give_equal_bits(scenes):
    import torch
    ds, cams, f = scenes("balls_box", (23, 5), 3)
    ref = fused_ok(ds, cams, f["depth"], f["normal"], f["rgb32f"], 16)
    arr, n = api._camera_array(cams)
    px = n * 23 * 5
    host = {k: np.array(f[k], F) for k in ("depth", "normal", "rgb32f")}
    dev = {k: torch.from_numpy(host[k]).cuda() for k in host}
    prm = ds._ray_params(1, api.ACCEL_BVH, False, False, False)
    a = api.AoParams(16, RADIUS, BIAS, SEED)
    for im in (0, 1):
        for om in (0, 1):
            src = {k: (dev[k].data_ptr() if im else host[k].ctypes.data) for k in host}
            whole_ao, ao = padded((n, 5, 23))
            whole_rgb, rgb = padded((n, 5, 23, 3))
            d_ao, d_rgb = torch.from_numpy(whole_ao.copy()).cuda(), torch.from_numpy(whole_rgb.copy()).cuda()
            i = api.AoInputs(src["depth"], src["normal"], src["rgb32f"], im)
            o = api.AoOutputs(d_ao.data_ptr() + 4 * PAD if om else ao.ctypes.data, d_rgb.data_ptr() + 4 * PAD if om else rgb.ctypes.data, om)
            assert P.lib().p3d_ambient_occlusion(ds.h, arr, n, C.byref(prm), C.byref(a), C.byref(i), C.byref(o)) == 0, P.lib().p3d_last_error()
            ds.sync()
            if om:
                whole_ao, whole_rgb = d_ao.cpu().numpy(), d_rgb.cpu().numpy()
            assert untouched(whole_ao) and untouched(whole_rgb)
            same_bits(whole_ao[PAD:-PAD].reshape(ref["ao"].shape), ref["ao"], "in %d out %d: ao" % (im, om))
            same_bits(whole_rgb[PAD:-PAD].reshape(ref["rgb32f"].shape), ref["rgb32f"], "in %d out %d: rgb32f" % (im, om))
    for k in host:
        same_bits(dev[k].cpu().numpy(), host[k], "an input plane changed: " + k)
    assert px == ref["ao"].size



def test_host_or_device_memory_on_either_side(scenes):
    """Host inputs with device outputs, device inputs with host outputs: the all-device bits.  Two frames of 70 x 5 at 4
    samples: 16 pixels a wave, so a row is more than one workgroup of an LDS scene and ends in a tail."""
    ds, cams, f = scenes("balls_box", (70, 5), 2)
    arr, n = api._camera_array(cams)
    planes = {k: np.array(f[k], F) for k in ("depth", "normal", "rgb32f")}
    prm = ds._ray_params(1, api.ACCEL_BVH, False, False, False)
    a = api.AoParams(4, RADIUS, BIAS, SEED)

    def call(i, in_memory, o, out_memory):
        ai = api.AoInputs(i["depth"], i["normal"], i["rgb32f"], in_memory)
        ao = api.AoOutputs(o["ao"], o["rgb32f"], out_memory)
        assert P.lib().p3d_ambient_occlusion(ds.h, arr, n, C.byref(prm), C.byref(a), C.byref(ai), C.byref(ao)) == 0, P.lib().p3d_last_error()

    ref = check_host_device_split(ds, planes, dict(ao=np.zeros((n, 5, 70), F), rgb32f=np.zeros((n, 5, 70, 3), F)), call)
    same_result(ref, fused_ok(ds, cams, f["depth"], f["normal"], f["rgb32f"], 4), "the all-device call and the host call")
    assert (ref["ao"] < 1).any()


def test_staging_is_counted_in_device_bytes():
    hs = P.HostScene(scene_path("balls_box"))
    hs.set_resolution(64, 16)
    ds = P.DeviceScene.from_host(hs)
    f = ds.render_aov(hs.camera(), max_depth=1)
    before = ds.stats()["device_bytes"]
    fused_ok(ds, [hs.camera()], f["depth"], f["normal"], f["rgb32f"], 4)
    grown = ds.stats()["device_bytes"] - before
    assert grown == 64 * 16 * (4 + 12 + 12 + 4 + 12) + 128, grown          # the planes in and out, one camera record
    fused_ok(ds, [hs.camera()], f["depth"], f["normal"], f["rgb32f"], 4)
    assert ds.stats()["device_bytes"] - before == grown
    ds.close()


def test_stream_capture():
    import torch
    hs = P.HostScene(scene_path("balls_box"))
    hs.set_resolution(*RES)
    ds = P.DeviceScene.from_host(hs)
    cams = hs.orbit_cameras(2, 7.0)
    f = ds.render_aov(cams, max_depth=2)
    ref = fused_ok(ds, cams[:1], f["depth"][0], f["normal"][0], None, 8)       # (one camera: the buffer holds one record)
    ref2, _ = unfused(ds, cams, f["depth"], f["normal"], None, 8)
    dev = {k: torch.from_numpy(np.ascontiguousarray(f[k])).cuda() for k in ("depth", "normal")}
    out = torch.zeros(2 * RES[0] * RES[1], dtype=torch.float32, device="cuda:0")
    run = lambda: ds.ambient_occlusion_device(cams, dev["depth"].data_ptr(), dev["normal"].data_ptr(), out_ao_ptr=out.data_ptr(),
                                              samples=8, radius=RADIUS, bias=BIAS, seed=SEED)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        ds.set_stream(torch.cuda.current_stream().cuda_stream)
        with pytest.raises(P.P3DError, match=r"\(%d\).*before the capture" % ERR_STATE):
            run()                                                               # two cameras: the buffer would have to grow
        with pytest.raises(P.P3DError, match=r"\(%d\).*host planes" % ERR_STATE):
            ds.ambient_occlusion(cams, f["depth"], f["normal"], samples=8)
        ds.ambient_occlusion_device(cams[:1], dev["depth"].data_ptr(), dev["normal"].data_ptr(), out_ao_ptr=out.data_ptr(),
                                    samples=8, radius=RADIUS, bias=BIAS, seed=SEED)
    ds.set_stream(0)
    assert not out.any(), "a captured call must not run"
    g.replay()
    torch.cuda.synchronize()
    same_bits(out.cpu().numpy()[:RES[0] * RES[1]].reshape(ref["ao"].shape), ref["ao"], "the capture survived the refusals")
    # after a call of the same shape: captured, and the replay gives the same bits
    run()
    ds.sync()
    out.zero_()
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side, capture_error_mode="thread_local"):
        ds.set_stream(torch.cuda.current_stream().cuda_stream)
        run()
    ds.set_stream(0)
    assert not out.any(), "a captured call must not run"
    g2.replay()
    torch.cuda.synchronize()
    same_bits(out.cpu().numpy().reshape(ref2["ao"].shape), ref2["ao"], "replayed graph")
    del g, g2
    ds.close()


# ---- 6. refusals

def set_(**kw):
    def edit(x):
        for k, v in kw.items():
            setattr(x, k, v)
    return edit


_one_float = (C.c_float * 4)()
# name -> (status, text p3d_last_error must hold, prm / ao / in / out edits)
REFUSED = {
    "flag_tree": (ERR_ARG, "flags", set_(flags=api.FLAG_TREE_KERNEL), None, None, None),
    "flag_tile": (ERR_ARG, "flags", set_(flags=api.FLAG_TILE_KERNEL), None, None, None),
    "flag_counters": (ERR_ARG, "flags", set_(flags=api.FLAG_COUNTERS), None, None, None),
    "flag_profile": (ERR_ARG, "flags", set_(flags=api.FLAG_PROFILE), None, None, None),
    "flag_packet": (ERR_ARG, "flags", set_(flags=api.FLAG_PACKET_WALK), None, None, None),
    "flag_device_samples": (ERR_ARG, "flags", set_(flags=api.FLAG_DEVICE_SAMPLES), None, None, None),
    "flag_unknown": (ERR_ARG, "flags", set_(flags=1 << 20), None, None, None),
    "feature_soft_shadow": (ERR_ARG, "features", set_(features=api.FEATURE_SOFT_SHADOW), None, None, None),
    "feature_schlick": (ERR_ARG, "features", set_(features=api.FEATURE_SCHLICK), None, None, None),
    "spp": (ERR_ARG, "spp", set_(spp=1), None, None, None),
    "samples_pointer": (ERR_ARG, "samples", set_(samples=C.cast(_one_float, C.POINTER(C.c_float))), None, None, None),
    "world": (ERR_ARG, "world", set_(world=2), None, None, None),
    "rank": (ERR_ARG, "rank", set_(rank=1), None, None, None),
    "accel_3": (ERR_ARG, "accel", set_(accel=3), None, None, None),
    "depth_null": (ERR_ARG, "depth", None, None, set_(depth=None), None),
    "normal_null": (ERR_ARG, "normal", None, None, set_(normal=None), None),
    "inputs_memory_2": (ERR_ARG, "p3d_ao_inputs::memory", None, None, set_(memory=2), None),
    "outputs_memory_negative": (ERR_ARG, "p3d_ao_outputs::memory", None, None, None, set_(memory=-1)),
    "both_outputs_null": (ERR_ARG, "ao and rgb32f", None, None, None, set_(ao=None, rgb32f=None)),
}
for _s in (0, 3, 5, 12, 65, 128, -8):
    REFUSED["samples_%d" % _s] = (ERR_ARG, "p3d_ao_params::samples", None, set_(samples=_s), None, None)
for _k, _v in (("zero", 0.0), ("negative", -0.5), ("inf", np.inf), ("nan", np.nan)):
    REFUSED["radius_" + _k] = (ERR_ARG, "radius", None, set_(radius=_v), None, None)
for _k, _v in (("negative", -0.001), ("inf", np.inf), ("nan", np.nan)):
    REFUSED["bias_" + _k] = (ERR_ARG, "bias", None, set_(bias=_v), None, None)


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_leave_the_outputs_and_the_handle_alone(case, scenes):
    ds, cams, f = scenes("balls_box")
    status, text, prm_edit, ao_edit, in_edit, out_edit = REFUSED[case]
    before = ds.stats()["device_bytes"]
    rc, out = fused(ds, cams, f["depth"], f["normal"], f["rgb32f"], 8, prm_edit=prm_edit, ao_edit=ao_edit, in_edit=in_edit, out_edit=out_edit)
    assert rc == status, (case, rc, P.lib().p3d_last_error())
    assert text in P.lib().p3d_last_error().decode(), P.lib().p3d_last_error()
    assert (out["ao"] == SENTINEL).all() and (out["rgb32f"] == SENTINEL).all(), "a refused call wrote"
    assert ds.stats()["device_bytes"] == before, "a refused call grew the handle"


def test_more_refusals(scenes):
    import torch
    ds, cams, f = scenes("balls_box")
    L = P.lib()
    # aliases: an output plane that is an input plane, or the other output plane
    for name in ("depth", "normal", "rgb32f"):
        for which in ("ao", "rgb32f"):
            keep = np.ascontiguousarray(f[name]).copy()

            def edit_in(i, keep=keep, name=name):
                setattr(i, name, keep.ctypes.data)

            def edit_out(o, keep=keep, which=which):
                setattr(o, which, keep.ctypes.data)
            rc, out = fused(ds, cams, f["depth"], f["normal"], f["rgb32f"], 8, in_edit=edit_in, out_edit=edit_out)
            assert rc == ERR_ARG and b"alias" in L.p3d_last_error(), (name, which)
            same_bits(keep, np.ascontiguousarray(f[name]), "a refused call wrote")
    rc, out = fused(ds, cams, f["depth"], f["normal"], None, 8, out_edit=lambda o: setattr(o, "rgb32f", o.ao))
    assert rc == ERR_ARG and b"alias" in L.p3d_last_error()
    # n below 1, cameras that differ, NULL structs
    rc, out = fused(ds, cams, f["depth"], f["normal"], None, 8, n=0)
    assert rc == ERR_ARG and b"n must" in L.p3d_last_error() and (out["ao"] == SENTINEL).all()
    other = api.Camera.from_buffer_copy(cams[0])
    other.res_x += 1
    prm = ds._ray_params(1, api.ACCEL_BVH, False, False, False)
    a = api.AoParams(8, RADIUS, BIAS, SEED)
    d2, n2 = np.zeros((2,) + f["depth"].shape[1:], F), np.zeros((2,) + f["normal"].shape[1:], F)
    o2 = np.full(d2.shape, SENTINEL, F)
    arr, _ = api._camera_array([cams[0], other])
    i, o = api.AoInputs(d2.ctypes.data, n2.ctypes.data, None, 0), api.AoOutputs(o2.ctypes.data, None, 0)
    assert L.p3d_ambient_occlusion(ds.h, arr, 2, C.byref(prm), C.byref(a), C.byref(i), C.byref(o)) == ERR_ARG and b"res_x" in L.p3d_last_error()
    for args in ((None, C.byref(prm), C.byref(a), C.byref(i), C.byref(o)), (arr, None, C.byref(a), C.byref(i), C.byref(o)),
                 (arr, C.byref(prm), None, C.byref(i), C.byref(o)), (arr, C.byref(prm), C.byref(a), None, C.byref(o)),
                 (arr, C.byref(prm), C.byref(a), C.byref(i), None)):
        assert L.p3d_ambient_occlusion(ds.h, args[0], 1, *args[1:]) == ERR_ARG and L.p3d_last_error()
    # the limit, before anything is allocated: 32768 x 32768 pixels fit 31 bits, their 2 samples each do not; 46341^2 pixels do not
    torch.cuda.synchronize()
    free0, before = torch.cuda.mem_get_info()[0], ds.stats()["device_bytes"]
    big = api.Camera.from_buffer_copy(cams[0])
    big.res_x, big.res_y = 32768, 32768
    arr1, _ = api._camera_array([big])
    a2 = api.AoParams(2, RADIUS, BIAS, SEED)
    assert L.p3d_ambient_occlusion(ds.h, arr1, 1, C.byref(prm), C.byref(a2), C.byref(i), C.byref(o)) == ERR_LIMIT
    assert b"31 bits" in L.p3d_last_error() and torch.cuda.mem_get_info()[0] == free0 and ds.stats()["device_bytes"] == before
    a1 = api.AoParams(1, RADIUS, BIAS, SEED)
    big.res_x, big.res_y = 46341, 46341
    arr1, _ = api._camera_array([big])
    assert L.p3d_ambient_occlusion(ds.h, arr1, 1, C.byref(prm), C.byref(a1), C.byref(i), C.byref(o)) == ERR_LIMIT
    assert (o2 == SENTINEL).all()
    # accepted: P3D_FLAG_WAVEFRONT does nothing, max_depth is not read
    ref = fused_ok(ds, cams, f["depth"], f["normal"], None, 8)
    got = fused_ok(ds, cams, f["depth"], f["normal"], None, 8, prm_edit=set_(flags=api.FLAG_WAVEFRONT, max_depth=0))
    same_result(got, ref, "P3D_FLAG_WAVEFRONT")


def test_a_cull_never_hit_scene_is_served_in_bvh_mode_only(scenes):
    _, cams, f = scenes("balls_box")
    ds = P.DeviceScene.from_host(P.HostScene(scene_path("balls_box")), cull_never_hit=True)
    for accel in (api.ACCEL_NONE, api.ACCEL_GRID):
        rc, out = fused(ds, cams, f["depth"], f["normal"], None, 8, accel=accel)
        assert rc == ERR_STATE and b"cull_never_hit" in P.lib().p3d_last_error() and (out["ao"] == SENTINEL).all()
    ref, _ = unfused(ds, cams, f["depth"], f["normal"], None, 8)
    same_result(fused_ok(ds, cams, f["depth"], f["normal"], None, 8), ref, "BVH mode on a cull_never_hit handle")
    ds.close()


# ---- 7. scene motion, handle state

def test_queries_follow_an_update_and_a_rebuild(tmp_path):
    m = SU.lattice(tmp_path)
    hs = P.HostScene(m.path["B"])
    hs.set_resolution(*RES)
    cams = [hs.camera()]
    fresh = m.fresh("B")
    f = fresh.render_aov(cams, max_depth=1)
    assert np.isfinite(f["depth"]).mean() > 0.3
    ds = m.fresh("A")
    stale = fused_ok(ds, cams, f["depth"], f["normal"], None, 8)
    ds.update(m.data["B"])
    moved = fused_ok(ds, cams, f["depth"], f["normal"], None, 8)
    assert (stale["ao"].view(np.uint32) != moved["ao"].view(np.uint32)).any(), "the update must show"
    for accel in (0, 1, 2):
        ref, occ = unfused(ds, cams, f["depth"], f["normal"], None, 8, accel=accel)
        assert occ.max() > 0
        same_result(fused_ok(ds, cams, f["depth"], f["normal"], None, 8, accel=accel), ref, "after the update, accel %d" % accel)
        same_result(fused_ok(fresh, cams, f["depth"], f["normal"], None, 8, accel=accel), ref, "a fresh handle on the moved scene, accel %d" % accel)
    assert ds.rebuild()["rebuilt"] == 1
    for accel in (0, 1, 2):
        for private_walk in (False, True):
            ref, _ = unfused(ds, cams, f["depth"], f["normal"], None, 8, accel=accel, private_walk=private_walk)
            same_result(fused_ok(ds, cams, f["depth"], f["normal"], None, 8, accel=accel, private_walk=private_walk), ref,
                        "after the rebuild, accel %d private %s" % (accel, private_walk))
    ds.close(); fresh.close()


def test_handle_state_is_left_alone():
    hs = P.HostScene(scene_path("balls_box"))
    hs.set_resolution(64, 48)
    ds = P.DeviceScene.from_host(hs)
    cam = hs.camera()
    f = ds.render_aov(cam, max_depth=2)
    a = ds.render(cam, max_depth=4)
    sched, tiles = ds.last_schedule(), ds.last_primary_tiles()
    ds.ambient_occlusion(cam, f["depth"], f["normal"], f["rgb32f"], samples=8, seed=SEED)
    ds.ambient_occlusion(cam, f["depth"], f["normal"], f["rgb32f"], samples=8, seed=SEED, accel=api.ACCEL_NONE, no_lds=True)
    assert ds.last_schedule() == sched and ds.last_primary_tiles() == tiles
    b = ds.render(cam, max_depth=4)
    assert ds.last_schedule() == sched and ds.last_primary_tiles() == tiles
    same_bits(a["rgb32f"], b["rgb32f"], "the frame after ambient occlusion")
    assert np.array_equal(a["hit_id"], b["hit_id"])
    ds.close()


# ---- 8. the command line

def test_cli_ao_denoise(tmp_path, scenes):
    import subprocess
    ds, cams, f = scenes("balls_box", (64, 48))
    exe = os.path.join(os.path.dirname(P.__file__), "p3d_render")
    out, prefix = tmp_path / "ao.ppm", tmp_path / "planes"
    common = [exe, scene_path("balls_box"), "--res", "64", "48", "--seed", str(SEED)]
    r = subprocess.run(common + ["--ao", "8", "0.5", "--denoise", "2", "--ao-out", str(prefix), "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    hs = P.HostScene(scene_path("balls_box"))
    frame = ds.render_aov(cams, max_depth=4, accel=hs.accel)
    lit = fused_ok(ds, cams, frame["depth"], frame["normal"], frame["rgb32f"], 8, accel=hs.accel)
    ref = api.host_denoise(lit["rgb32f"], frame["depth"], frame["normal"], frame["albedo"], iterations=2)
    head = b"P6\n64 48\n255\n"
    data = out.read_bytes()
    assert data.startswith(head)
    got = np.frombuffer(data[len(head):], np.uint8).reshape(48, 64, 3)[::-1]                  # the file is top row first
    same_bits(np.ascontiguousarray(got), ref["rgb8"][0], "p3d_render --ao 8 0.5 --denoise 2")
    same_bits(np.load(str(prefix) + "_ao.npy"), lit["ao"][0], "--ao-out")
    assert (lit["ao"] < 1).any() and not np.array_equal(ref["rgb8"], frame["rgb8"])
    r = subprocess.run(common + ["--ao", "8", "0.5", "--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--ao" in r.stderr
    r = subprocess.run(common + ["--ao", "6", "0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--ao" in r.stderr
