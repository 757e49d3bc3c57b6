"""Sampled frames on the GPU at every sample count from 1 to 8, in accel NONE, GRID and BVH, against
tests/golden/sample_counts.npz: frames of the reference's own object code (tests/golden/make_sample_counts_golden.py;
tests/test_sample_counts_pinned.py shows on the CPU that a sum in another order, a lost clamp or a wrong sample index
gives another frame).

Everything that depends on ns = spp * spp is run: the wavefront schedule's ns passes over min(4, ns) lane streams and
their sum kernel, the tile kernel's LDS accumulator, the tree kernels' per-lane sums, / 16 above 1.0, bands x samples,
shards, samples made on the device, batches and the AOV planes.  Every comparison is exact: rgb32f as uint32 bit patterns,
rgb8 and primary hit ids equal, the ray count equal.  Samples are HostScene.samples(seed, spp) unless a test says otherwise.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, RGB_TOL, assert_rgb8_equal
from extra_scenes import scene_path
from test_gpu_aov import check_planes, handles, raw_aov, stream_reference
from test_gpu_render_frames import eyes_around, frame, same, set_eye_cams
import u_4a_2s_p3d_raytracer_template2_amd as P
from u_4a_2s_p3d_raytracer_template2_amd import multigpu as MG

pytestmark = pytest.mark.gpu

assert RGB_TOL == 0.0
FRAMES = np.load(os.path.join(GOLDEN, "sample_counts.npz"))
with open(os.path.join(GOLDEN, "sample_counts.json")) as _f:
    CASES = json.load(_f)
SCHEDULES = ["tile", "wavefront", "tree"]
BANDED = "bl_16x160_d3_spp3"
DEFAULT_WORKSPACE_MIB = 64 << 10            # p3d_scene::workspace_budget as a handle starts: 64 GiB


def handle(m):
    hs = P.HostScene(scene_path(m["scene"]))
    hs.set_resolution(*m["res"])
    return hs, P.DeviceScene.from_host(hs)


def render_args(m, hs, **over):
    kw = dict(max_depth=m["max_depth"], accel=m["accel"], spp=m["spp"], soft_shadow=m["soft_shadow"], counters=True,
              samples=hs.samples(m["seed"], m["spp"]))
    kw.update(over)
    return kw


def assert_planes(out, name, what):
    hit_id, rgb32f = FRAMES[name + "/hit_id"], FRAMES[name + "/rgb32f"]
    assert np.array_equal(out["hit_id"], hit_id), "%s: primary hit ids differ in %d px, first at %s" % (
        what, int((out["hit_id"] != hit_id).sum()), np.argwhere(out["hit_id"] != hit_id)[:1].tolist())
    bad = (np.ascontiguousarray(out["rgb32f"]).view(np.uint32) != rgb32f.view(np.uint32)).any(-1)
    assert not bad.any(), "%s: rgb32f differs in %d px, first at %s: %s vs %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:1].tolist(), out["rgb32f"][bad][:1].tolist(), rgb32f[bad][:1].tolist())
    assert_rgb8_equal(out["rgb8"], FRAMES[name + "/rgb8"], what)


def assert_fixture(out, name, what):
    assert_planes(out, name, what)
    assert out["counters"]["rays"] == int(FRAMES[name + "/rays"]) == CASES[name]["rays"], what


# ---- a. every case, every way of running it

@pytest.mark.parametrize("name", sorted(CASES))
def test_sampled_frame_is_the_reference_frame(name):
    """One handle, every schedule forced and the handle's own choice, from the LDS copy of the scene and from HBM with
    shared and private walks.  balls_high does not fit LDS: it is read from HBM without a flag, and with it."""
    m = CASES[name]
    hs, ds = handle(m)
    kw = render_args(m, hs)
    lds = m["scene"] != "balls_high"
    for place in (dict(), dict(no_lds=True), dict(no_lds=True, private_walk=True)):
        for sched in SCHEDULES + [None]:
            what = "%s %s %s" % (name, sched or "default", place)
            out = ds.render(hs.camera(), **dict(kw, **place, **({sched: True} if sched else {})))
            if sched:
                assert ds.last_schedule() == sched, what
            elif lds and not place:
                assert ds.last_schedule() == "tile", what            # scenes served from LDS: sampled frames by rule
            assert_fixture(out, name, what)
    ds.close()


# ---- b. bands x samples

@pytest.mark.parametrize("place", [dict(), dict(no_lds=True)], ids=["lds", "no_lds"])
def test_bands_times_samples(place):
    """A sampled wavefront frame under a workspace budget.  plan_wavefront_bands: the 9 sample passes run on
    min(kLanes = 4, 9) = 4 lane streams, which split the budget: 1 MiB / 4 = 262 144 B a lane.  wavefront_bytes_per_pixel(3)
    is (2 + 4) * sizeof(RayRec) + (1 + 2) * sizeof(NodeRec) = 6 * 32 + 3 * 48 = 336 B; a tile row of this frame is one
    16x16 tile, 256 px, so 86 016 B; 262 144 / 86 016 = 3 tile rows a band.  The frame's 10 tile rows make 4 bands
    (3 + 3 + 3 + 1) a sample pass, 9 x 4 = 36 passes over the 4 lanes' workspaces."""
    m = CASES[BANDED]
    assert m["res"] == [16, 160] and m["max_depth"] == 3 and m["spp"] == 3
    lane_bytes, row_bytes = (1 << 20) // 4, (6 * 32 + 3 * 48) * 256
    assert lane_bytes // row_bytes == 3 and -(-(160 // 16) // 3) == 4
    hs, ds = handle(m)
    kw = render_args(m, hs, wavefront=True, **place)
    ds.set_tuning(workspace_mib=1)
    out = ds.render(hs.camera(), **kw)
    assert ds.last_schedule() == "wavefront"           # a band that does not fit would show as another schedule
    assert_fixture(out, BANDED, "banded %s" % place)
    ds.set_tuning(workspace_mib=DEFAULT_WORKSPACE_MIB)
    out = ds.render(hs.camera(), **kw)
    assert ds.last_schedule() == "wavefront"
    assert_fixture(out, BANDED, "unbanded after the banded frame %s" % place)
    ds.close()


# ---- c. shards

@pytest.mark.parametrize("sched", ["tile", "wavefront"])
@pytest.mark.parametrize("world", [2, 3])
def test_shards_stitch_to_the_reference_frame(world, sched):
    m = CASES[BANDED]
    W, H = m["res"]
    hs, ds = handle(m)
    kw = render_args(m, hs, world=world, row_block=16, **{sched: True})
    parts = []
    for r in range(world):
        parts.append(ds.render(hs.camera(), rank=r, **kw))
        assert ds.last_schedule() == sched
        assert parts[-1]["rgb8"].shape[0] == P.local_rows(H, 16, world)
    ds.close()
    st = {k: MG.stitch_reference([p[k] for p in parts], H, 16) for k in ("rgb8", "rgb32f", "hit_id")}
    assert_planes(st, BANDED, "world %d %s" % (world, sched))
    assert sum(p["counters"]["rays"] for p in parts) == CASES[BANDED]["rays"]


# ---- d. samples made on the device

@pytest.mark.parametrize("spp", [5, 8])
def test_device_samples_and_their_frame(spp):
    import torch
    name = "dof_40x24_d4_spp%d" % spp
    m = CASES[name]
    W, H = m["res"]
    hs, ds = handle(m)
    cam = hs.camera()
    host = hs.samples(m["seed"], spp)
    got = ds.generate_samples(m["seed"], W, H, spp, cam.aperture)
    assert got.shape == host.shape == (H, W, spp * spp, 4)
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32)), "generate_samples differs from HostScene.samples"
    smp = torch.zeros(host.size, dtype=torch.float32, device="cuda:0")
    ds.generate_samples_device(smp.data_ptr(), m["seed"], W, H, spp, cam.aperture)
    assert np.array_equal(smp.cpu().numpy().view(np.uint32), host.ravel().view(np.uint32))
    for sched in ("tile", "wavefront"):
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
        f32 = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
        hid = torch.full((H, W), -2, dtype=torch.int32, device="cuda:0")
        ds.render_device(cam, rgb8.data_ptr(), f32.data_ptr(), hid.data_ptr(), max_depth=m["max_depth"], accel=m["accel"], spp=spp,
                         samples_ptr=smp.data_ptr(), counters=True, **{sched: True})
        ds.sync()
        assert ds.last_schedule() == sched
        out = {"rgb8": rgb8.cpu().numpy(), "rgb32f": f32.cpu().numpy(), "hit_id": hid.cpu().numpy(), "counters": ds.counters()}
        assert_fixture(out, name, "%s from device samples, %s" % (name, sched))
    ds.close()


# ---- e. batches and AOV planes at an odd sample count

@pytest.mark.parametrize("sched", ["tile", "wavefront"])
def test_batch_of_three_cameras_at_spp_3(sched):
    name = "dof_40x24_d4_spp3"
    m = CASES[name]
    hs, ds = handle(m)
    samples = np.stack([hs.samples(m["seed"] + f, 3) for f in range(3)])            # seeds 101 to 103
    own = hs.camera()
    eyes = eyes_around(scene_path("dof"), 3)
    cams = [own] + set_eye_cams(hs, [eyes[0], eyes[2]])                             # frame 0: the scene's own camera
    kw = dict(max_depth=m["max_depth"], accel=m["accel"], spp=3, **{sched: True})
    batch = ds.render_frames(cams, samples=samples, **kw)
    assert ds.last_schedule() == sched
    one = P.DeviceScene.from_host(hs)
    for f in range(3):
        same(frame(batch, f), one.render(cams[f], samples=samples[f], **kw), "frame %d of the batch, %s" % (f, sched))
    assert (batch["rgb32f"][0].view(np.uint32) != batch["rgb32f"][2].view(np.uint32)).any(), "the cameras must show"
    assert_planes(frame(batch, 0), name, "frame 0 of the batch, %s" % sched)
    ds.close(); one.close()


@pytest.mark.parametrize("sched", ["tile", "wavefront"])
def test_aov_planes_describe_sample_0_at_spp_3(sched):
    name = "dof_40x24_d4_spp3"
    m = CASES[name]
    res = tuple(m["res"])
    hs, osc, ds = handles("dof", res)
    samples = hs.samples(m["seed"], 3)
    got = raw_aov(ds, hs.camera(), spp=3, samples=samples, max_depth=m["max_depth"], **{sched: True})
    assert ds.last_schedule() == sched
    # depth and normal: the bits p3d_trace_rays returns for the rays of sample 0 (samples[y][x][0])
    check_planes(got, stream_reference("dof", res, samples), osc, "dof spp 3 %s" % sched, pixels=400)
    assert_planes({k: got[k][0] for k in ("rgb8", "rgb32f", "hit_id")}, name, "the colours of the AOV call, %s" % sched)


# ---- g. arguments

@pytest.mark.parametrize("spp", [9, -1])
def test_sample_counts_outside_0_to_8_are_refused(spp):
    m = CASES["dof_40x24_d4_spp8"]
    hs, ds = handle(m)
    cam = hs.camera()
    samples = np.zeros((1, 24, 40, 81, 4), np.float32)           # large enough for whatever a call would read
    for call in (lambda: ds.render(cam, spp=spp, samples=samples[0]),
                 lambda: ds.render_frames([cam], spp=spp, samples=samples),
                 lambda: ds.render_aov(cam, spp=spp, samples=samples)):
        with pytest.raises(P.P3DError, match=r"\(-1\): spp must be in 0\.\.8"):         # P3D_ERR_ARG
            call()
    out = ds.render(cam, spp=8, samples=hs.samples(m["seed"], 8), counters=True)       # the handle is none the worse
    assert_fixture(out, "dof_40x24_d4_spp8", "after the refused calls")
    ds.close()
