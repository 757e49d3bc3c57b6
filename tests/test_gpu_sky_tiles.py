"""The tile coverage mask of the multi-tile level-1 kernels (p3d_set_sky_tiles, csrc/p3d_tile_coverage.h): a frame rendered
with the mask equals the frame rendered without it -- rgb8, rgb32f bit for bit and the hit-id plane -- and the oracle's, and
p3d_last_sky_tiles() reports what the host restatement of the mask says: the same number of empty tiles, or "no mask" where a
primitive is not in front of the eye.

Views (sky_tile_views.gpu_views) are chosen so that the workgroups of a launch meet every combination the kernel
distinguishes -- all of a workgroup's tiles empty (no scene copy, no barrier), the first empty and the second not, the
first not and the second empty, none empty -- which the test checks on the host mask before it renders; plus an all-sky
view and two that must run without a mask.  Frames the mask does not serve report so and equal the knob-off frame."""
import numpy as np
import pytest

from conftest import assert_rgb8_equal, scene_path, synthetic_cube_map
from oracle import oracle_py as O
import scene_gen
import sky_tile_views as V
import u_4a_2s_p3d_raytracer_template2_amd as P

pytestmark = pytest.mark.gpu

SIZES = [(160, 96), (100, 52)]           # 10 x 6 whole tiles; a partial last column and last row
NO_MASK = (False, 0)


def same(a, b, what):
    assert np.array_equal(a["hit_id"], b["hit_id"]), what + ": hit ids differ in %d px" % int((a["hit_id"] != b["hit_id"]).sum())
    assert np.array_equal(a["rgb32f"].view(np.uint32), b["rgb32f"].view(np.uint32)), what + ": rgb32f differs"
    assert_rgb8_equal(a["rgb8"], b["rgb8"], what)


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(path):
        if path not in made:
            hs = P.HostScene(path)
            made[path] = (hs, P.DeviceScene.from_host(hs))
        return made[path]
    yield get
    for _, ds in made.values():
        ds.close()


@pytest.fixture(scope="module")
def views(tmp_path_factory):
    """(scene) -> [(name, path of the scene file seen through that view)]"""
    d = tmp_path_factory.mktemp("sky_tiles_views")
    out = {}
    for scene in ("mount_low", "balls_low"):
        src = scene_path(scene)
        ptype, data12 = P.HostScene(src).arrays()[:2]
        out[scene] = [(name, V.write_view(src, V.view_path(d, scene, name), eye, at, angle))
                      for name, eye, at, angle in V.gpu_views(ptype, data12, V.file_view(src))]
    return out


def camera_of(path, w, h):
    hs = P.HostScene(path)
    hs.set_resolution(w, h)
    return hs, hs.camera()


def oracle_frame(path, w, h, depth=4):
    sc = O.Scene(path)
    sc.set_resolution(w, h)
    return sc.render(max_depth=depth, accel=2, spp=0, threads=8)


def on_and_off(ds, cam, **kw):
    ds.set_sky_tiles(0)
    off = ds.render(cam, **kw)
    assert ds.last_sky_tiles() == NO_MASK
    ds.set_sky_tiles(1)
    on = ds.render(cam, **kw)
    return on, off


@pytest.mark.parametrize("tiles", [2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("scene", ["mount_low", "balls_low"])
def test_masked_frames_equal_unmasked_frames_and_the_oracle(handles, views, scene, size, tiles):
    w, h = size
    _, ds = handles(scene_path(scene))
    ds.set_primary_tiles(tiles)
    patterns = set()
    for name, path in views[scene]:
        vhs, cam = camera_of(path, w, h)
        active, fell_back = P.host_tile_coverage(cam, vhs.desc())
        if not fell_back:
            patterns |= V.workgroup_patterns(active, tiles)
        what = "%s %dx%d %s, %d tiles" % (scene, w, h, name, tiles)
        ref = oracle_frame(path, w, h)
        for frame in range(2):                               # back to back: the second frame runs on the other counter set
            on, off = on_and_off(ds, cam)
            assert ds.last_schedule() == "wavefront" and ds.last_primary_tiles() == tiles
            used, empty = ds.last_sky_tiles()
            same(on, off, what + ", mask on against off, frame %d" % frame)
            same(on, ref, what + ", mask on against the oracle")
            # the device's mask is the host's: the same statements over the same scene
            assert (used, empty) == ((False, 0) if fell_back else (True, int(active.size - active.sum()))), what
        if name == "all_sky":
            assert not fell_back and not active.any() and not (ref["hit_id"] >= 0).any()
        if name in ("inside_bounds", "behind_eye"):
            assert fell_back, what + ": must run without a mask"
    # every combination of a workgroup's first two tiles, and a workgroup with nothing to trace
    assert {p[:2] for p in patterns} >= {(False, False), (False, True), (True, False), (True, True)}, patterns
    assert any(not any(p) for p in patterns)
    ds.set_primary_tiles(0)
    ds.set_sky_tiles(1)


def test_the_mask_follows_a_moved_sphere(handles, views):
    """p3d_scene_update moves a sphere into a region the mask had marked empty: the next frame's mask has it."""
    w, h = 160, 96
    path = dict(views["mount_low"])["middle"]
    vhs, cam = camera_of(path, w, h)
    ptype, data12 = vhs.arrays()[:2]
    i = int(np.argmax(ptype == V.SPHERE))
    assert ptype[i] == V.SPHERE
    ds = P.DeviceScene.from_host(vhs)
    try:
        ds.set_sky_tiles(1)
        before = ds.render(cam)
        used, empty_before = ds.last_sky_tiles()
        assert used
        # towards the frame's lower left corner pixel's ray: a place the 'middle' view shows as sky
        o, d = vhs.primary_ray(8.5, 8.5)
        assert before["hit_id"][:16, :16].max() < 0
        moved = data12[i].copy()
        moved[:3] = o + d * np.float32(np.linalg.norm(data12[i][:3] - o))
        ds.update(moved[None, :], [i])
        on, off = on_and_off(ds, cam)
        same(on, off, "after the update, mask on against off")
        assert (on["hit_id"][:16, :16] >= 0).any(), "the moved sphere is not in the frame"
        used, empty_after = ds.last_sky_tiles()
        assert used and empty_after != empty_before
    finally:
        ds.close()


def test_frames_the_mask_does_not_serve_say_so_and_are_unchanged(handles, views, tmp_path):
    w, h = 160, 96
    hs, ds = handles(scene_path("mount_low"))
    path = dict(views["mount_low"])["middle"]
    vhs, cam = camera_of(path, w, h)
    ds.set_primary_tiles(2)
    ds.set_skybox(synthetic_cube_map())
    smp = vhs.samples(12345, 2)
    cases = [("skybox", "render", dict(skybox=True, seed=3)), ("spp 2", "render", dict(spp=2, samples=smp)),
             ("counters", "render", dict(counters=True)), ("frame batch", "render_frames", {}), ("AOV planes", "render_aov", {}),
             ("tile schedule", "render", dict(tile=True)), ("scene read from HBM", "render", dict(no_lds=True, wavefront=True))]
    for what, entry, kw in cases:
        outs = []
        for knob in (0, 1):
            ds.set_sky_tiles(knob)
            out = getattr(ds, entry)(cam if entry == "render" else [cam, cam], **kw)
            assert ds.last_sky_tiles() == NO_MASK, what
            outs.append(out)
        same(outs[1], outs[0], what)
        if what == "counters":                               # the counting build: the same rays whatever the knob says
            assert outs[1]["counters"] == outs[0]["counters"] and outs[0]["counters"]["rays"] > 0
    ds.set_sky_tiles(1)
    ds.render(cam)
    assert ds.last_sky_tiles()[0]                            # ... and the plain frame has one again
    # a scene with a plane: every camera ray can meet it
    src = str(tmp_path / "with_plane.p3f")
    scene_gen.write_scene(src, np.random.default_rng(21), 3, 3, 1, 1, 1, 2)
    phs, pcam = camera_of(src, w, h)
    pds = P.DeviceScene.from_host(phs)
    try:
        pds.set_primary_tiles(2)
        on, off = on_and_off(pds, pcam)
        assert pds.last_sky_tiles() == NO_MASK
        same(on, off, "scene with a plane")
    finally:
        pds.close()
    ds.set_primary_tiles(0)
    assert P.lib().p3d_set_sky_tiles(ds.h, 2) != 0           # the C entry takes 0 or 1


@pytest.mark.parametrize("row_block", [16, 32])
def test_both_shares_of_a_frame_sharded_over_two_ranks(handles, views, row_block):
    """world = 2: a tile's compact rows are mapped to image rows exactly, so each rank's mask is its own rows'.  (row_block
    must be a multiple of 16 -- p3d_render refuses 8 -- so the second case is 32: row blocks of two tile rows.)"""
    w, h = 160, 96
    _, ds = handles(scene_path("mount_low"))
    ds.set_primary_tiles(2)
    for name in ("middle", "upper", "file"):
        vhs, cam = camera_of(dict(views["mount_low"])[name], w, h)
        ref = oracle_frame(dict(views["mount_low"])[name], w, h)
        for rank in (0, 1):
            on, off = on_and_off(ds, cam, rank=rank, world=2, row_block=row_block)
            what = "%s, rank %d of 2, row_block %d" % (name, rank, row_block)
            same(on, off, what)
            active, fell_back = P.host_tile_coverage(cam, vhs.desc(), row_block=row_block, rank=rank, world=2)
            rows = P.local_rows(h, row_block, 2)
            image_rows = np.array([((r // row_block) * 2 + rank) * row_block + r % row_block for r in range(rows)])
            real = image_rows < h
            assert np.array_equal(on["hit_id"][real], ref["hit_id"][image_rows[real]]), what + ": not the oracle's rows"
            real_tiles = real.reshape(-1, 16).any(axis=1)
            assert not fell_back and ds.last_sky_tiles() == (True, int((~active[real_tiles]).sum())), what
    with pytest.raises(P.P3DError):
        ds.render(cam, world=2, row_block=8)
    ds.set_primary_tiles(0)
