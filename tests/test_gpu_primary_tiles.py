"""Several tiles per workgroup in the wavefront schedule's level-1 launch (p3d_set_primary_tiles, wf_primary_kernel_tiles):
a frame rendered with 2 or 3 tiles per workgroup equals the one-tile render of the same handle -- rgb8, rgb32f bit for
bit, the hit-id plane, and the work counters -- at the shapes where the loop over tiles can go wrong, at depth 1 (only the
first-block clearing feeds the next pass) and depth 4, two frames back to back (the counter-parity flip).

The counting builds have no such kernel (p3d_kernel_variant.h), so a render made with counters runs one tile per
workgroup whatever is forced: the counters are compared all the same, and the test checks that the handle says so."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_rgb8_equal, scene_path
import u_4a_2s_p3d_raytracer_template2_amd as P

pytestmark = pytest.mark.gpu

# (res_x, res_y, rank, world): one tile (trailing iterations empty); ragged right edge and three tile rows; seven tile rows
# (a remainder for 2 and for 3); interleaved row blocks of rank 1 of 3
SHAPES = [(16, 16, 0, 1), (50, 36, 0, 1), (64, 112, 0, 1), (64, 112, 1, 3)]


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(name):
        if name not in made:
            hs = P.HostScene(scene_path(name))
            made[name] = (hs, P.DeviceScene.from_host(hs))
        return made[name]
    yield get
    for _, ds in made.values():
        ds.close()


def same(a, b, what):
    assert np.array_equal(a["hit_id"], b["hit_id"]), what + ": hit ids differ"
    assert np.array_equal(a["rgb32f"].view(np.uint32), b["rgb32f"].view(np.uint32)), what + ": rgb32f differs"
    assert_rgb8_equal(a["rgb8"], b["rgb8"], what)


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("res_x,res_y,rank,world", SHAPES)
@pytest.mark.parametrize("scene", ["mount_low", "balls_low"])
def test_forced_tiles_equal_one_tile(handles, scene, res_x, res_y, rank, world, depth):
    hs, ds = handles(scene)
    hs.set_resolution(res_x, res_y)
    cam = hs.camera()
    kw = dict(max_depth=depth, rank=rank, world=world, row_block=16)
    ds.set_primary_tiles(1)
    ref = ds.render(cam, **kw)
    assert ds.last_schedule() == "wavefront" and ds.last_primary_tiles() == 1
    same(ds.render(cam, **kw), ref, "one tile, second frame")
    ref_counters = ds.render(cam, counters=True, **kw)["counters"]
    assert ref_counters["rays"] > 0
    for tiles in (2, 3):
        ds.set_primary_tiles(tiles)
        for frame in range(2):                               # back to back: the second frame runs on the other counter set
            out = ds.render(cam, **kw)
            assert ds.last_schedule() == "wavefront" and ds.last_primary_tiles() == tiles
            same(out, ref, "%s %dx%d rank %d/%d depth %d, %d tiles, frame %d" % (scene, res_x, res_y, rank, world, depth, tiles, frame))
        counted = ds.render(cam, counters=True, **kw)
        assert ds.last_primary_tiles() == 1                  # the counting build: one tile per workgroup, and it says so
        assert counted["counters"] == ref_counters
        same(counted, ref, "counting build")
        same(ds.render(cam, **kw), ref, "after the counting build")
    ds.set_primary_tiles(0)


@pytest.mark.parametrize("name,res", [("c2_mount_low_256x144_d4_bvh", (256, 144)), ("mount_low_37x23_d4_bvh", (37, 23))])
@pytest.mark.parametrize("tiles", [2, 3])
def test_forced_tiles_equal_the_golden_frame(handles, tiles, name, res):
    """The golden frames of an LDS scene on this schedule with more than one tile row: nine (a remainder for 2), and two
    with ragged edges on both sides (a remainder for 3)."""
    frames = np.load(os.path.join(GOLDEN, "frames.npz"))
    hs, ds = handles("mount_low")
    hs.set_resolution(*res)
    ds.set_primary_tiles(tiles)
    for frame in range(2):
        out = ds.render(hs.camera(), max_depth=4)
        assert ds.last_schedule() == "wavefront" and ds.last_primary_tiles() == tiles
        same(out, {k: frames[name + "/" + k] for k in ("rgb8", "rgb32f", "hit_id")}, "%s, %d tiles, frame %d" % (name, tiles, frame))
    ds.set_primary_tiles(0)


def test_a_forced_value_without_a_kernel_runs_one_tile_and_says_so(handles):
    hs, ds = handles("mount_low")
    hs.set_resolution(64, 112)
    cam = hs.camera()
    ds.set_primary_tiles(3)
    plain = ds.render(cam)
    assert ds.last_primary_tiles() == 3
    for what, kw in [("random draws", dict(fuzzy_reflection=True, seed=7)), ("Schlick", dict(schlick=True)), ("counters", dict(counters=True)),
                     ("scene read from HBM", dict(no_lds=True, wavefront=True)),
                     ("tile schedule", dict(tile=True)), ("tree schedule", dict(tree=True))]:
        out = ds.render(cam, **kw)
        assert ds.last_primary_tiles() == 1, what
        if what not in ("random draws", "Schlick"):
            same(out, plain, what)
    cams = [cam, cam]
    batch = ds.render_frames(cams)
    assert ds.last_primary_tiles() == 1
    same({k: batch[k][0] for k in ("rgb8", "rgb32f", "hit_id")}, plain, "frame batch")
    ds.set_tuning(xcd_chunk=4)                               # a chunked tile map is a 1-D launch
    same(ds.render(cam), plain, "xcd_chunk 4")
    assert ds.last_primary_tiles() == 1
    ds.set_tuning(xcd_chunk=1)
    same(ds.render(cam), plain, "back on the 2-D launch")
    assert ds.last_primary_tiles() == 3
    with pytest.raises(P.P3DError):
        ds.set_primary_tiles(4)
    ds.set_primary_tiles(0)
    ds.render(cam)
    assert 1 <= ds.last_primary_tiles() <= 3                 # the default
