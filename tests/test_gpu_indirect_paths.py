"""p3d_indirect_paths on the GPU: the fused kernel against the unfused pipeline the definition names -- B rounds of
DeviceScene.trace_rays(max_depth = 1) on the same handle, driven by the NumPy restatement (tests/path_reference.py) -- against
p3d_indirect_diffuse at one bounce, and against the reference's own rayTracing() through the oracle.  Every pixel comparison
is an equality of bits; every output is allocated with PAD elements of sentinel on either side, which must stay untouched.
The helpers are those of tests/test_gpu_indirect.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ao_reference as AO                                  # noqa: E402
import path_reference as PR                                # noqa: E402
import test_gpu_indirect as TI                             # noqa: E402
import test_gpu_scene_update as SU                         # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P            # noqa: E402
from extra_scenes import scene_path                        # noqa: E402
from plane_memory import check_host_device_split          # noqa: E402
from oracle import oracle_py as O                          # noqa: E402
from test_gpu_indirect import BIAS, ERR_ARG, ERR_STATE, MODES, PLANES, RES, SEED, SENTINEL, padded, same_bits, same_result, set_, untouched  # noqa: E402
from test_gpu_indirect import scenes                      # noqa: E402,F401  (the module's fixture: one handle per scene)
from u_4a_2s_p3d_raytracer_template2_amd import api        # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
_materials = {}


def materials(path):
    """(prim_material, materials12) of a scene file's description."""
    if path not in _materials:
        a = P.HostScene(path).arrays()
        _materials[path] = (a[2], a[3])
    return _materials[path]


def fused(ds, cams, depth, normal, albedo=None, rgb=None, samples=8, bounces=3, seed=SEED, accel=api.ACCEL_BVH, want=PLANES, bias=BIAS,
          prm_edit=None, ind_edit=None, in_edit=None, out_edit=None, n=None, **mode):
    """p3d_indirect_paths through ctypes on host planes, outputs padded with SENTINEL -> (status, {"indirect", "rgb32f"}); the
    padding is checked here."""
    arr, n_cams = api._camera_array(cams)
    H, W = arr[0].res_y, arr[0].res_x
    depth = np.ascontiguousarray(depth, F).reshape(n_cams, H, W)
    normal = np.ascontiguousarray(normal, F).reshape(n_cams, H, W, 3)
    albedo = None if albedo is None else np.ascontiguousarray(albedo, F).reshape(n_cams, H, W, 3)
    rgb = None if rgb is None else np.ascontiguousarray(rgb, F).reshape(n_cams, H, W, 3)
    whole_ind, ind = padded((n_cams, H, W, 3))
    whole_rgb, out_rgb = padded((n_cams, H, W, 3))
    prm = ds._ray_params(1, accel, mode.get("no_lds", False), mode.get("private_walk", False), False)
    g = api.PathParams(int(samples), int(bounces), bias, int(seed) & 0xFFFFFFFF)
    i = api.IndirectInputs(depth.ctypes.data, normal.ctypes.data, albedo.ctypes.data if albedo is not None else None,
                           rgb.ctypes.data if rgb is not None else None, 0)
    o = api.IndirectOutputs(ind.ctypes.data if "indirect" in want else None, out_rgb.ctypes.data if "rgb32f" in want else None, 0)
    for edit, x in ((prm_edit, prm), (ind_edit, g), (in_edit, i), (out_edit, o)):
        if edit:
            edit(x)
    rc = P.lib().p3d_indirect_paths(ds.h, arr, n_cams if n is None else n, C.byref(prm), C.byref(g), C.byref(i), C.byref(o))
    assert untouched(whole_ind) and untouched(whole_rgb), "written outside an output plane"
    return rc, {"indirect": ind, "rgb32f": out_rgb}


def fused_ok(*args, **kw):
    rc, out = fused(*args, **kw)
    assert rc == 0, P.lib().p3d_last_error()
    return out


def unfused(ds, mats, cams, depth, normal, albedo=None, rgb=None, samples=8, bounces=3, seed=SEED, accel=api.ACCEL_BVH, bias=BIAS, **mode):
    """path_reference.paths with B rounds of DeviceScene.trace_rays(max_depth = 1) as the answer."""
    n = len(cams)
    planes = dict(depth=np.asarray(depth, F).reshape((n,) + np.shape(depth)[-2:]), normal=np.asarray(normal, F).reshape((n,) + np.shape(normal)[-3:]))
    if albedo is not None:
        planes["albedo"] = np.asarray(albedo, F).reshape(planes["normal"].shape)
    if rgb is not None:
        planes["rgb32f"] = np.asarray(rgb, F).reshape(planes["normal"].shape)
    return PR.paths(PR.device_answer(ds, accel, **mode), cams, planes, samples, bounces, bias, seed, mats)


# ---- 1. fused equals unfused

@pytest.mark.parametrize("sb", [(1, 2), (8, 3), (64, 2), (4, 8)], ids=lambda sb: "S%d_B%d" % sb)
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("name", ["balls_box", "balls_low", "mount_low"])
def test_fused_equals_unfused(name, accel, mode, sb, scenes):
    S, B = sb
    ds, cams, f = scenes(name)
    ref = unfused(ds, materials(scene_path(name)), cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], S, B, accel=accel, **MODES[mode])
    got = fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], S, B, accel=accel, **MODES[mode])
    same_result(got, ref, "%s accel %d %s S=%d B=%d" % (name, accel, mode, S, B))
    q = ref["valid"].astype(bool)
    assert np.array_equal(q, np.isfinite(f["depth"])) and q.any()
    assert not got["indirect"][~q].any()
    same_bits(got["rgb32f"][~q], np.ascontiguousarray(f["rgb32f"][~q]), "a pixel without a path keeps its colour")


@pytest.mark.parametrize("private_walk", [False, True], ids=["shared", "private"])
def test_dragon_equals_trace_rays(private_walk, scenes):
    ds, cams, f = scenes("dragon")
    assert ds.stats()["n_triangles"] > 2000 and np.isfinite(f["depth"]).any(), "a scene read from HBM natively, with paths"
    ref = unfused(ds, materials(scene_path("dragon")), cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 8, 3, private_walk=private_walk)
    got = fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 8, 3, private_walk=private_walk)
    same_result(got, ref, "dragon private %s" % private_walk)
    assert ref["traced"][1] > 0


# ---- 2. one bounce is p3d_indirect_diffuse

@pytest.mark.parametrize("mode", ["lds", "hbm"])
@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("name", ["balls_box", "balls_low", "mount_low"])
def test_one_bounce_is_indirect_diffuse(name, accel, mode, scenes):
    ds, cams, f = scenes(name)
    for S in (1, 16):
        ref = TI.fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], S, accel=accel, **MODES[mode])
        got = fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], S, 1, accel=accel, **MODES[mode])
        same_result(got, ref, "%s accel %d %s S=%d, bounces 1" % (name, accel, mode, S))


# ---- 3. the anchor to the reference: the oracle's closest hits and its rayTracing() at MAX_DEPTH 1

@pytest.mark.parametrize("accel", [0, 1, 2])
def test_planes_equal_the_references_paths(accel):
    hs = P.HostScene(scene_path("balls_box"))
    hs.set_resolution(12, 8)
    cams = [hs.camera()]
    ds = P.DeviceScene.from_host(hs)
    f = ds.render_aov(cams, max_depth=2, accel=api.ACCEL_BVH)
    osc = O.Scene(scene_path("balls_box"))
    _, _, pm = osc.prims()
    ref = PR.paths(PR.oracle_answer(osc, O.lib(), accel), cams, f, 4, 3, BIAS, SEED, (pm.astype(np.uint32), osc.materials()))
    got = fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 4, 3, accel=accel)
    same_result(got, ref, "balls_box accel %d against the oracle" % accel)
    assert ref["traced"][2] > 0
    ds.close()


# ---- 4. shapes: res_x below 64 / S, no multiple of it, one row, one pixel and 64 pixels per wave

def with_surface_everywhere(cams, f):
    """Where the frame shows the sky, a point 3 units along the pixel's ray whose normal is the view axis (test_shapes')."""
    sky = ~np.isfinite(f["depth"])
    depth = np.where(sky, F(3.0), f["depth"]).astype(F)
    normal = np.where(sky[..., None], np.array(list(cams[0].n), F), f["normal"]).astype(F)
    return depth, normal


@pytest.mark.parametrize("samples", [1, 16, 64])
@pytest.mark.parametrize("res", [(1, 1), (7, 3), (63, 1), (65, 2)], ids=lambda r: "%dx%d" % r)
def test_shapes(res, samples, scenes):
    ds, cams, f = scenes("balls_low", res)
    mats = materials(scene_path("balls_low"))
    depth, normal = with_surface_everywhere(cams, f)
    for mode in ("lds", "hbm"):
        ref = unfused(ds, mats, cams, depth, normal, f["albedo"], f["rgb32f"], samples, 3, **MODES[mode])
        assert ref["valid"].all()
        got = fused_ok(ds, cams, depth, normal, f["albedo"], f["rgb32f"], samples, 3, **MODES[mode])
        same_result(got, ref, "%dx%d S=%d %s" % (res + (samples, mode)))


def aimed_camera(cam, x, y, res):
    """A copy of cam turned so that its axis is the ray through pixel (x, y) of cam, with a window of 1 % of cam's at
    resolution res: every pixel of it, the last of a row included, sees what that one pixel saw."""
    eye, uw, vh, vz = AO.camera_fields(cam)
    fx, fy = (F(x) + F(0.5)) / F(cam.res_x) - F(0.5), (F(y) + F(0.5)) / F(cam.res_y) - F(0.5)
    d = ((uw * fx + vh * fy) + vz).astype(np.float64)
    n = -d / np.linalg.norm(d)
    u = np.cross(np.array(list(cam.v), np.float64), n)
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    c = api.Camera.from_buffer_copy(cam)
    for k in range(3):
        c.u[k], c.v[k], c.n[k] = u[k], v[k], n[k]
    c.w, c.h = c.w * 0.01, c.h * 0.01
    c.res_x, c.res_y = res
    return c


def test_one_lane_alone_stays_alive(scenes):
    """65 x 2 at S = 1: the second wave of a row holds pixel 64 alone, and only that pixel of the top row is valid.  The row's
    ends show the sky in the committed scenes' own views, so the camera is aimed at what pixel (9, 2) of balls_box at
    24 x 16 sees -- inside the box, where a fifth of the paths trace three rays (test_indirect_paths_host.py) -- and the
    seed is the first for which the reference says this path does."""
    ds, cams, _ = scenes("balls_box")
    cam = aimed_camera(cams[0], 9, 2, (65, 2))
    f = ds.render_aov([cam], max_depth=1, accel=api.ACCEL_BVH)
    mats = materials(scene_path("balls_box"))
    assert np.isfinite(f["depth"][0, 1, 64])
    depth = np.full(f["depth"].shape, np.inf, F)
    depth[0, 1, 64] = f["depth"][0, 1, 64]
    seeds = [s for s in range(64) if unfused(ds, mats, [cam], depth, f["normal"], None, f["rgb32f"], 1, 3, seed=s)["traced"][2] == 1]
    assert seeds, "no seed below 64 keeps the path alive for three rays"
    for mode in ("lds", "hbm"):
        ref = unfused(ds, mats, [cam], depth, f["normal"], None, f["rgb32f"], 1, 3, seed=seeds[0], **MODES[mode])
        got = fused_ok(ds, [cam], depth, f["normal"], None, f["rgb32f"], 1, 3, seed=seeds[0], **MODES[mode])
        same_result(got, ref, "one live lane, %s, seed %d" % (mode, seeds[0]))
        assert ref["valid"].sum() == 1 and ref["traced"].tolist() == [1, 1, 1]


def test_a_frame_without_a_valid_pixel(scenes):
    ds, cams, f = scenes("balls_low", (65, 2))
    depth = np.full(f["depth"].shape, np.inf, F)
    depth[0, 0, 3], depth[0, 1, 7] = F(np.nan), F(-1.0)
    for mode in ("lds", "hbm"):
        for S in (1, 16):
            got = fused_ok(ds, cams, depth, f["normal"], f["albedo"], f["rgb32f"], S, 3, **MODES[mode])
            assert not got["indirect"].any() and not np.signbit(got["indirect"]).any()
            same_bits(got["rgb32f"], np.ascontiguousarray(f["rgb32f"]), "no path anywhere: the colour")


# ---- 5. path prefixes

def test_sample_s_is_the_same_path_and_fewer_bounces_are_a_prefix(scenes):
    ds, cams, f = scenes("balls_box")
    ref = unfused(ds, materials(scene_path("balls_box")), cams, f["depth"], f["normal"], None, None, 8, 3)
    q = ref["valid"].astype(bool)
    for B in (1, 2, 3):
        one = fused_ok(ds, cams, f["depth"], f["normal"], None, None, 1, B)
        same_bits(one["indirect"][q], np.ascontiguousarray(ref["prefix"][B - 1][..., 0, :][q]),
                  "S = 1, B = %d is sample 0 of S = 8 after %d rays of B = 3" % (B, B))
    assert (ref["prefix"][1].view(np.uint32) != ref["prefix"][2].view(np.uint32)).any(), "the third ray must show"
    assert (ref["prefix"][0].view(np.uint32) != ref["prefix"][1].view(np.uint32)).any(), "the second ray must show"


# ---- 6. batch

@pytest.mark.parametrize("mode", ["lds", "hbm"])
def test_a_batch_is_its_frames_with_seed_plus_f(mode, scenes):
    ds, cams, f = scenes("balls_box", (23, 5), 3)
    assert (f["depth"][0].view(np.uint32) != f["depth"][2].view(np.uint32)).any(), "the orbit must show"
    batch = fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 16, 3, **MODES[mode])
    ref = unfused(ds, materials(scene_path("balls_box")), cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 16, 3, **MODES[mode])
    same_result(batch, ref, "batch")
    for k in range(3):
        one = fused_ok(ds, [cams[k]], f["depth"][k], f["normal"][k], f["albedo"][k], f["rgb32f"][k], 16, 3, seed=SEED + k, **MODES[mode])
        for p in PLANES:
            same_bits(one[p][0], batch[p][k], "frame %d alone: %s" % (k, p))
    other = fused_ok(ds, [cams[0]], f["depth"][0], f["normal"][0], None, None, 16, 3, seed=SEED + 1)
    assert (batch["indirect"][0].view(np.uint32) != other["indirect"][0].view(np.uint32)).any(), "the seed must show"


# ---- 7. outputs, memory

def test_output_planes_with_and_without_albedo_and_colour(scenes):
    ds, cams, f = scenes("balls_box")
    mats = materials(scene_path("balls_box"))
    for albedo in (None, f["albedo"]):
        for rgb in (None, f["rgb32f"]):
            ref = unfused(ds, mats, cams, f["depth"], f["normal"], albedo, rgb, 8, 3)
            for want in (("indirect",), ("rgb32f",), PLANES):
                got = fused_ok(ds, cams, f["depth"], f["normal"], albedo, rgb, 8, 3, want=want)
                for k in PLANES:
                    if k in want:
                        same_bits(got[k], ref[k], "want %s albedo %s colour %s: %s" % (want, albedo is not None, rgb is not None, k))
                    else:
                        assert (got[k] == SENTINEL).all(), "a plane that was not asked for was written"


def test_host_or_device_memory_on_either_side(scenes):
    """Two frames of 70 x 5 at 4 samples: 16 pixels a wave, so a row is more than one workgroup of an LDS scene and ends in a
    tail."""
    ds, cams, f = scenes("balls_box", (70, 5), 2)
    arr, n = api._camera_array(cams)
    planes = {k: np.array(f[k], F) for k in ("depth", "normal", "albedo", "rgb32f")}
    prm = ds._ray_params(1, api.ACCEL_BVH, False, False, False)
    g = api.PathParams(4, 3, BIAS, SEED)

    def call(i, in_memory, o, out_memory):
        ii = api.IndirectInputs(i["depth"], i["normal"], i["albedo"], i["rgb32f"], in_memory)
        io = api.IndirectOutputs(o["indirect"], o["rgb32f"], out_memory)
        assert P.lib().p3d_indirect_paths(ds.h, arr, n, C.byref(prm), C.byref(g), C.byref(ii), C.byref(io)) == 0, P.lib().p3d_last_error()

    ref = check_host_device_split(ds, planes, dict(indirect=np.zeros((n, 5, 70, 3), F), rgb32f=np.zeros((n, 5, 70, 3), F)), call)
    same_result(ref, fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 4, 3), "the all-device call and the host call")
    assert (ref["indirect"] > 0).any()


def test_alternating_with_indirect_diffuse_grows_nothing():
    hs = P.HostScene(scene_path("balls_box"))
    hs.set_resolution(64, 16)
    ds = P.DeviceScene.from_host(hs)
    cams = [hs.camera()]
    f = ds.render_aov(cams, max_depth=1)
    before = ds.stats()["device_bytes"]
    fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 4, 3)
    grown = ds.stats()["device_bytes"] - before
    assert grown == 64 * 16 * (4 + 12 + 12 + 12 + 12 + 12) + 128, grown          # the planes in and out, one camera record
    for _ in range(2):
        TI.fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 4)
        assert ds.stats()["device_bytes"] - before == grown, "p3d_indirect_diffuse stages in the same buffers"
        fused_ok(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 4, 2)
        assert ds.stats()["device_bytes"] - before == grown
    ds.close()


# ---- 8. stream capture

def test_stream_capture():
    import torch
    hs = P.HostScene(scene_path("balls_box"))
    hs.set_resolution(*RES)
    ds = P.DeviceScene.from_host(hs)
    mats = materials(scene_path("balls_box"))
    cams = hs.orbit_cameras(2, 7.0)
    f = ds.render_aov(cams, max_depth=2)
    ref = fused_ok(ds, cams[:1], f["depth"][0], f["normal"][0], None, None, 8, 3)       # (one camera: the buffer holds one record)
    ref2 = unfused(ds, mats, cams, f["depth"], f["normal"], None, None, 8, 3)
    dev = {k: torch.from_numpy(np.ascontiguousarray(f[k])).cuda() for k in ("depth", "normal")}
    out = torch.zeros(2 * RES[0] * RES[1] * 3, dtype=torch.float32, device="cuda:0")
    run = lambda c=cams: ds.indirect_paths_device(c, dev["depth"].data_ptr(), dev["normal"].data_ptr(), out_indirect_ptr=out.data_ptr(),
                                                  samples=8, bounces=3, bias=BIAS, seed=SEED)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        ds.set_stream(torch.cuda.current_stream().cuda_stream)
        with pytest.raises(P.P3DError, match=r"\(%d\).*before the capture" % ERR_STATE):
            run()                                                               # two cameras: the buffer would have to grow
        with pytest.raises(P.P3DError, match=r"\(%d\).*host planes" % ERR_STATE):
            ds.indirect_paths(cams, f["depth"], f["normal"], samples=8, bounces=3)
        run(cams[:1])
    ds.set_stream(0)
    assert not out.any(), "a captured call must not run"
    g.replay()
    torch.cuda.synchronize()
    same_bits(out.cpu().numpy()[:RES[0] * RES[1] * 3].reshape(ref["indirect"].shape), ref["indirect"], "the capture survived the refusals")
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
    same_bits(out.cpu().numpy().reshape(ref2["indirect"].shape), ref2["indirect"], "replayed graph")
    del g, g2
    ds.close()


# ---- 9. refusals: p3d_indirect_diffuse's table with this entry's parameter struct, and bounces

REFUSED = {k: (v[0], v[1].replace("p3d_indirect_params", "p3d_path_params")) + v[2:] for k, v in TI.REFUSED.items()}
for _b in (0, -1, 9):
    REFUSED["bounces_%d" % _b] = (ERR_ARG, "p3d_path_params::bounces", None, set_(bounces=_b), None, None)


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_leave_the_outputs_and_the_handle_alone(case, scenes):
    ds, cams, f = scenes("balls_box")
    status, text, prm_edit, ind_edit, in_edit, out_edit = REFUSED[case]
    before, sched = ds.stats()["device_bytes"], ds.last_schedule()
    rc, out = fused(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 8, 3, prm_edit=prm_edit, ind_edit=ind_edit, in_edit=in_edit,
                    out_edit=out_edit)
    assert rc == status, (case, rc, P.lib().p3d_last_error())
    assert text in P.lib().p3d_last_error().decode(), P.lib().p3d_last_error()
    assert (out["indirect"] == SENTINEL).all() and (out["rgb32f"] == SENTINEL).all(), "a refused call wrote"
    assert ds.stats()["device_bytes"] == before, "a refused call grew the handle"
    assert ds.last_schedule() == sched, "a refused call changed p3d_last_schedule"


def test_a_frame_after_refusals_is_bit_identical(scenes):
    ds, cams, f = scenes("balls_box")
    first = ds.render(cams[0], max_depth=4)
    sched = ds.last_schedule()
    for case in ("bounces_0", "bounces_9", "samples_3", "flag_tree", "bias_nan", "both_outputs_null"):
        status, _, prm_edit, ind_edit, in_edit, out_edit = REFUSED[case]
        rc, _ = fused(ds, cams, f["depth"], f["normal"], None, None, 8, 3, prm_edit=prm_edit, ind_edit=ind_edit, in_edit=in_edit, out_edit=out_edit)
        assert rc == status
    again = ds.render(cams[0], max_depth=4)
    assert ds.last_schedule() == sched
    same_bits(again["rgb32f"], first["rgb32f"], "the frame after the refusals")
    assert np.array_equal(again["hit_id"], first["hit_id"])


def test_null_structs_and_a_culled_scene_are_refused(scenes):
    ds, cams, f = scenes("balls_box")
    L = P.lib()
    prm = ds._ray_params(1, api.ACCEL_BVH, False, False, False)
    g = api.PathParams(8, 3, BIAS, SEED)
    d2, n2 = np.array(f["depth"], F), np.array(f["normal"], F)
    o2 = np.full(n2.shape, SENTINEL, F)
    arr, _ = api._camera_array(cams)
    i, o = api.IndirectInputs(d2.ctypes.data, n2.ctypes.data, None, None, 0), api.IndirectOutputs(o2.ctypes.data, None, 0)
    for args in ((None, C.byref(prm), C.byref(g), C.byref(i), C.byref(o)), (arr, None, C.byref(g), C.byref(i), C.byref(o)),
                 (arr, C.byref(prm), None, C.byref(i), C.byref(o)), (arr, C.byref(prm), C.byref(g), None, C.byref(o)),
                 (arr, C.byref(prm), C.byref(g), C.byref(i), None)):
        assert L.p3d_indirect_paths(ds.h, args[0], 1, *args[1:]) == ERR_ARG and L.p3d_last_error()
    assert (o2 == SENTINEL).all()
    # aliases: an output plane that is an input plane, or the other output plane
    for name in ("depth", "normal", "albedo", "rgb32f"):
        keep = np.ascontiguousarray(f[name]).copy()
        rc, out = fused(ds, cams, f["depth"], f["normal"], f["albedo"], f["rgb32f"], 8, 3, in_edit=lambda i: setattr(i, name, keep.ctypes.data),
                        out_edit=lambda o: setattr(o, "rgb32f", keep.ctypes.data))
        assert rc == ERR_ARG and b"alias" in L.p3d_last_error(), name
        same_bits(keep, np.ascontiguousarray(f[name]), "a refused call wrote")
    rc, out = fused(ds, cams, f["depth"], f["normal"], None, None, 8, 3, out_edit=lambda o: setattr(o, "rgb32f", o.indirect))
    assert rc == ERR_ARG and b"alias" in L.p3d_last_error()
    rc, out = fused(ds, cams, f["depth"], f["normal"], None, None, 8, 3, n=0)
    assert rc == ERR_ARG and b"n must" in L.p3d_last_error() and (out["indirect"] == SENTINEL).all()
    # the limit is still on n * res_y * res_x * samples, before anything is allocated: 32768 x 32768 pixels fit 31 bits, 2 paths each do not
    before = ds.stats()["device_bytes"]
    big = api.Camera.from_buffer_copy(cams[0])
    big.res_x, big.res_y = 32768, 32768
    arr1, _ = api._camera_array([big])
    g2 = api.PathParams(2, 8, BIAS, SEED)
    assert L.p3d_indirect_paths(ds.h, arr1, 1, C.byref(prm), C.byref(g2), C.byref(i), C.byref(o)) == TI.ERR_LIMIT
    assert b"31 bits" in L.p3d_last_error() and ds.stats()["device_bytes"] == before and (o2 == SENTINEL).all()
    culled = P.DeviceScene.from_host(P.HostScene(scene_path("balls_box")), cull_never_hit=True)
    for accel in (api.ACCEL_NONE, api.ACCEL_GRID, api.ACCEL_BVH):
        rc, out = fused(culled, cams, f["depth"], f["normal"], None, None, 8, 3, accel=accel)
        assert rc == ERR_STATE and b"cull_never_hit" in L.p3d_last_error() and (out["indirect"] == SENTINEL).all()
    culled.close()


# ---- 10. scene motion

def test_paths_follow_an_update_and_a_rebuild(tmp_path):
    m = SU.lattice(tmp_path)
    hs = P.HostScene(m.path["B"])
    hs.set_resolution(*RES)
    cams = [hs.camera()]
    mats = materials(m.path["B"])
    fresh = m.fresh("B")
    f = fresh.render_aov(cams, max_depth=1)
    assert np.isfinite(f["depth"]).mean() > 0.3
    ds = m.fresh("A")
    stale = fused_ok(ds, cams, f["depth"], f["normal"], None, None, 8, 2)
    ds.update(m.data["B"])
    moved = fused_ok(ds, cams, f["depth"], f["normal"], None, None, 8, 2)
    assert (stale["indirect"].view(np.uint32) != moved["indirect"].view(np.uint32)).any(), "the update must show"
    for accel in (0, 1, 2):
        ref = unfused(ds, mats, cams, f["depth"], f["normal"], None, None, 8, 2, accel=accel)
        assert ref["traced"][1] > 0
        same_result(fused_ok(ds, cams, f["depth"], f["normal"], None, None, 8, 2, accel=accel), ref, "after the update, accel %d" % accel)
        same_result(fused_ok(fresh, cams, f["depth"], f["normal"], None, None, 8, 2, accel=accel), ref, "a fresh handle on the moved scene, accel %d" % accel)
    assert ds.rebuild()["rebuilt"] == 1
    for accel in (0, 1, 2):
        for private_walk in (False, True):
            ref = unfused(ds, mats, cams, f["depth"], f["normal"], None, None, 8, 2, accel=accel, private_walk=private_walk)
            same_result(fused_ok(ds, cams, f["depth"], f["normal"], None, None, 8, 2, accel=accel, private_walk=private_walk), ref,
                        "after the rebuild, accel %d private %s" % (accel, private_walk))
    ds.close(); fresh.close()


# ---- 11. the command line

def test_cli_gi_bounces(tmp_path, scenes):
    ds, cams, f = scenes("balls_box", (64, 48))
    exe = os.path.join(os.path.dirname(P.__file__), "p3d_render")
    common = [exe, scene_path("balls_box"), "--res", "64", "48", "--seed", str(SEED)]

    def run(*flags):
        out = tmp_path / ("_".join(flags).replace("-", "") + ".ppm")
        r = subprocess.run(common + list(flags) + ["--out", str(out)], capture_output=True, text=True, timeout=120)
        return r, (out.read_bytes() if r.returncode == 0 else b"")

    r, two = run("--gi", "8", "--gi-bounces", "2", "--denoise", "2")
    assert r.returncode == 0, r.stderr
    hs = P.HostScene(scene_path("balls_box"))
    frame = ds.render_aov(cams, max_depth=4, accel=hs.accel)
    lit = fused_ok(ds, cams, frame["depth"], frame["normal"], frame["albedo"], frame["rgb32f"], 8, 2, accel=hs.accel)
    ref = api.host_denoise(lit["rgb32f"], frame["depth"], frame["normal"], frame["albedo"], iterations=2)
    head = b"P6\n64 48\n255\n"
    assert two.startswith(head)
    got = np.frombuffer(two[len(head):], np.uint8).reshape(48, 64, 3)[::-1]                  # the file is top row first
    same_bits(np.ascontiguousarray(got), ref["rgb8"][0], "p3d_render --gi 8 --gi-bounces 2 --denoise 2")
    r, one = run("--gi", "8", "--gi-bounces", "1")
    assert r.returncode == 0, r.stderr
    r, plain = run("--gi", "8")
    assert r.returncode == 0, r.stderr
    assert one == plain, "--gi-bounces 1 writes the bytes of --gi alone"
    r, two_plain = run("--gi", "8", "--gi-bounces", "2")
    assert r.returncode == 0 and two_plain != plain, "the second bounce must show in the file"
    r, _ = run("--gi-bounces", "2")
    assert r.returncode == 2 and "--gi-bounces" in r.stderr
    for b in ("0", "9"):
        r, _ = run("--gi", "8", "--gi-bounces", b)
        assert r.returncode == 2 and "--gi-bounces" in r.stderr
