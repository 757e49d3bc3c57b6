"""The walks of tests/handle_walks.py, checked without a GPU: they hold the transitions tests/test_gpu_handle_walks.py is
there to render, and the tile-order key of csrc/p3d_frame_config.h -- compiled for the host, as tests/test_schedule_pick.py
does -- decides the tile count of every pair of their steps.  Two mutants of the header (the key without row_block, the
key without world) are compiled the same way and must be caught by that pair check; they run on the CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import handle_walks as W
import u_4a_2s_p3d_raytracer_template2_amd as P
from u_4a_2s_p3d_raytracer_template2_amd import api

SCHEDULES = (W.SCHED_TILE, W.SCHED_TREE, W.SCHED_WAVEFRONT)
HEADER = os.path.join(W.CSRC, "p3d_frame_config.h")

SRC = r"""
#include "p3d_frame_config.h"
using namespace p3d;
// v: res_x, res_y, max_depth, accel, spp, rank, world, row_block, flags, features, n_frames, schedule, n_tiles
static FrameConfig cfg_of(const int* v) {
    FrameConfig c;
    c.res_x = v[0]; c.res_y = v[1]; c.max_depth = v[2]; c.accel = v[3]; c.spp = v[4]; c.rank = v[5]; c.world = v[6]; c.row_block = v[7];
    c.flags = (uint32_t)v[8] & kConfigFlags; c.features = (uint32_t)v[9]; c.n_frames = v[10];
    return c;
}
extern "C" {
int tile_order_key_equal(const int* a, const int* b) { return tile_order_key(cfg_of(a), a[11], a[12]) == tile_order_key(cfg_of(b), b[11], b[12]); }
int pick_key_equal(const int* a, const int* b) { return pick_key(cfg_of(a)) == pick_key(cfg_of(b)); }
int budget_key_equal(const int* a, const int* b) { return budget_key(cfg_of(a)) == budget_key(cfg_of(b)); }
}
"""


def build_keys(d, header_text=None):
    """The harness over csrc/p3d_frame_config.h, or over header_text written next to the source (quoted includes look there first)."""
    d.mkdir(exist_ok=True)
    (d / "keys.cpp").write_text(SRC)
    if header_text is not None:
        (d / "p3d_frame_config.h").write_text(header_text)
    inc = ["-I" + os.path.join(W.REPO, "include"), "-I" + W.CSRC]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC"] + inc + [str(d / "keys.cpp"), "-o", str(d / "keys.so")])
    L = C.CDLL(str(d / "keys.so"))
    for fn in (L.tile_order_key_equal, L.pick_key_equal, L.budget_key_equal):
        fn.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    return build_keys(tmp_path_factory.mktemp("keys") / "real")


def ints(v):
    return (C.c_int * len(v))(*v)


def key_violations(L, walk):
    """Ordered pairs of the walk's calls whose TileOrderKeys are equal and whose tile counts differ, per schedule; the wave
    tiles only where their order is used: frames of a scene not in LDS (run_tree, run_wavefront).  -> (violations, equal pairs)"""
    bad, equal = [], 0
    for s in SCHEDULES:
        cs = [c for c in W.calls(walk) if s == W.SCHED_TILE or not W.lds_scene(c)]
        cfg = [ints(W.frame_config(c, s)) for c in cs]
        for i, a in enumerate(cs):
            for j, b in enumerate(cs):
                if i != j and L.tile_order_key_equal(cfg[i], cfg[j]):
                    equal += 1
                    if W.tiles_of(a, s) != W.tiles_of(b, s):
                        bad.append((s, a, b, W.tiles_of(a, s), W.tiles_of(b, s)))
    return bad, equal


# ---- the arithmetic

def test_restated_constants_and_rows_are_the_librarys():
    assert (W.FLAG_NO_LDS_SCENE, W.FEATURE_SOFT_SHADOW) == (api.FLAG_NO_LDS_SCENE, api.FEATURE_SOFT_SHADOW)
    assert W.SCHEDULE_ID == {n: i for i, n in enumerate(("wavefront", "tree", "tile"))}       # DeviceScene.last_schedule
    for res_y in (1, 15, 16, 17, 23, 64, 96, 144, 150, 200, 1080):
        for rb in (0, 16, 32, 48, 80, 112):
            for world in (0, 1, 2, 3, 8):
                assert W.local_rows(res_y, rb, world) == P.local_rows(res_y, rb, world), (res_y, rb, world)
    assert W.tile_order_period() == 64


def test_shard_rows_deal_every_image_row_once_and_stitch_inverts_them():
    rng = np.random.default_rng(3)
    for H, rb, world in ((150, 16, 3), (150, 48, 2), (150, 80, 3), (144, 112, 3), (23, 16, 2), (1, 16, 1)):
        Wd = 5
        full = {"rgb8": rng.integers(0, 256, (H, Wd, 3), dtype=np.uint8), "rgb32f": rng.random((H, Wd, 3), dtype=np.float32),
                "hit_id": rng.integers(-1, 99, (H, Wd), dtype=np.int32)}
        seen, parts = [], []
        for r in range(world):
            rows = W.shard_rows(H, rb, world, r)
            seen += [y for _, y in rows]
            n = W.local_rows(H, rb, world)
            part = {"rgb8": np.full((n, Wd, 3), 7, np.uint8), "rgb32f": np.full((n, Wd, 3), -1, np.float32), "hit_id": np.full((n, Wd), -9, np.int32),
                    "counters": dict(closest_queries=1, shadow_queries=2, rays=3, pixels=len(rows) * Wd)}
            for lr, y in rows:
                for k in full:
                    part[k][lr] = full[k][y]
            parts.append(part)
        assert sorted(seen) == list(range(H)), (H, rb, world)
        st = W.stitch(parts, H, Wd, world, rb)
        for k in full:
            assert np.array_equal(st[k], full[k]), (H, rb, world, k)
        assert st["counters"] == dict(closest_queries=world, shadow_queries=2 * world, rays=3 * world, pixels=H * Wd)
    assert W.shard_rows(150, 80, 3, 2) == []              # a rank whose row blocks all lie past the image


def test_tile_counts_at_200x150():
    want = {(16, 1): (130, 520), (32, 1): (130, 520), (48, 1): (156, 624), (112, 1): (182, 728), (16, 2): (65, 260),
            (48, 2): (78, 312), (16, 3): (52, 208)}
    got = {(s["row_block"], s["world"]): (W.tiles16(s), W.tiles_wave(s, 1)) for s in W.BH if s["fixture"] == W.BIG}
    assert got == want
    low = W.step(W.BIG, 16, 3)
    assert not W.order_used(low, W.SCHED_TILE) and W.order_used(low, W.SCHED_TREE) and W.order_used(low, W.SCHED_WAVEFRONT)
    assert W.tiles16(W.step("bh_128_d4_grid")) == 64 and W.tiles_wave(W.step("bh_128_d4_grid")) == 256
    a = W.step(W.A)
    assert (W.tiles16(a), W.tiles_wave(a), W.tiles_wave(W.step(W.A, no_lds=True))) == (144, 144, 576)


# ---- the walks have the transitions they are for

def pairs(walk):
    return list(zip(walk[:-1], walk[1:]))


def moves(walk, what, where=lambda a, b: True):
    """{(what(a), what(b))} over consecutive steps that differ in it."""
    return {(what(a), what(b)) for a, b in pairs(walk) if what(a) != what(b) and where(a, b)}


def meta(key):
    return lambda s: W.META[s["fixture"]][key]


def shard(s):
    return (s["row_block"], s["world"])


def both_ways(got, want):
    return all((a, b) in got and (b, a) in got for a, b in want)


@pytest.mark.parametrize("name", sorted(W.WALKS))
def test_walk_fixtures_and_tile_count_transitions(name):
    scene, walk = W.WALKS[name]
    assert all(W.META[s["fixture"]]["scene"] == scene for s in walk)
    want = {"BH": {"bh_200x150_d4_bvh", "bh_128_d4_grid", "bh_128_d4_none", "bh_64_d4_spp2", "bh_96_d6_bvh", "bh_96x64_d4_bvh_soft"},
            "ML": {"c2_mount_low_256x144_d4_bvh", "mount_low_256x144_d4_grid", "mount_low_256x144_d4_none", "c4_mount_low_96_d6_spp2",
                   "mount_low_37x23_d4_bvh", "mount_low_1x1_d1"}}[name]
    assert {s["fixture"] for s in walk} == want
    big = walk[0]["fixture"]
    assert {shard(s) for s in walk if s["fixture"] == big and not s["no_lds"]} == {(16, 1), (32, 1), (48, 1), (112, 1), (16, 2), (48, 2), (16, 3)}
    for tiles in (W.tiles16, W.tiles_wave):
        same_res = [(a, b) for a, b in pairs(walk) if a["fixture"] == b["fixture"] == big and a["no_lds"] == b["no_lds"] and shard(a) != shard(b)]
        kinds = {(tiles(b) > tiles(a)) - (tiles(b) < tiles(a)) for a, b in same_res}
        assert kinds == {1, -1, 0}, "the tile count must grow, shrink and stay equal under another key"
        grown = {(shard(a), shard(b)) for a, b in same_res if tiles(b) > tiles(a)}
        assert any((b, a) in {(shard(x), shard(y)) for x, y in same_res} for a, b in grown)
        equal = {(shard(a), shard(b)) for a, b in same_res if tiles(b) == tiles(a)}
        assert any((b, a) in equal for a, b in equal), "equal counts under another key, both ways"
    # row blocks that are no power of two, on one and on several ranks
    assert {(48, 1), (112, 1), (48, 2)} <= {shard(s) for s in walk}
    # the first configuration again, after everything else
    assert walk[-1] == walk[0] and walk[0] == W.step(big)
    assert all(s in walk[:-1] for s in walk)


@pytest.mark.parametrize("name", sorted(W.WALKS))
def test_walk_configuration_transitions(name):
    _, walk = W.WALKS[name]
    # accel BVH, GRID, NONE, BVH, and the same the other way round
    assert both_ways(moves(walk, meta("accel")), [(2, 1), (1, 0), (0, 2)])
    # depth and spp up and down
    deep = 6
    assert both_ways(moves(walk, meta("max_depth")), [(4, deep)])
    assert both_ways(moves(walk, meta("spp")), [(0, 2)])
    # into and out of "no order" on the tile schedule
    assert both_ways(moves(walk, lambda s: W.order_used(s, W.SCHED_TILE)), [(True, False)])
    # every rank of a sharded step is rendered
    assert all(len({c["rank"] for c in W.calls([s])}) == s["world"] for s in walk)
    assert not any(W.tree_refuses(s) for s in walk), "every step of these walks can run on the tree schedule"


def test_bh_walk_transitions_of_a_scene_read_from_hbm():
    walk = W.BH
    assert not any(W.lds_scene(s) for s in walk)
    # two resolutions of 64 tiles or more on both sides, there and back
    enough = lambda a, b: min(W.tiles16(a), W.tiles16(b)) >= W.MIN_ORDER_TILES
    assert both_ways(moves(walk, lambda s: tuple(meta("res")(s)), enough), [((200, 150), (128, 128))])
    # soft shadow on and off
    assert both_ways(moves(walk, meta("soft_shadow")), [(False, True)])
    # "no order" on the wave-tile schedules too, and the tile schedule's order off while theirs is on
    for s in (W.SCHED_TREE, W.SCHED_WAVEFRONT):
        assert both_ways(moves(walk, lambda st: W.order_used(st, s)), [(True, False)])
    assert any(not W.order_used(st, W.SCHED_TILE) and W.order_used(st, W.SCHED_TREE) for st in walk)


def test_ml_walk_moves_the_scene_out_of_lds_and_back():
    walk = W.ML
    flips = [(a, b) for a, b in pairs(walk) if a["no_lds"] != b["no_lds"]]
    same_request = [(a, b) for a, b in flips if dict(a, no_lds=False) == dict(b, no_lds=False)]
    assert {(a["no_lds"], b["no_lds"]) for a, b in same_request} == {(False, True), (True, False)}
    assert all(W.tiles_wave(a) != W.tiles_wave(b) and W.tiles16(a) == W.tiles16(b) for a, b in same_request)
    # out of LDS the wave tiles learn an order, and the walk changes their count there
    hbm = [s for s in walk if s["no_lds"]]
    assert len({W.tiles_wave(s) for s in hbm if W.order_used(s, W.SCHED_TREE)}) >= 2
    assert both_ways(moves(walk, meta("max_depth")), [(4, 1)])


# ---- the keys

@pytest.mark.parametrize("name", sorted(W.WALKS))
def test_equal_tile_order_keys_mean_equal_tile_counts(keys, name):
    bad, equal = key_violations(keys, W.WALKS[name][1])
    assert equal > 0, "the walk returns to configurations: some keys must be equal"
    assert not bad, bad[:3]


@pytest.mark.parametrize("name", sorted(W.WALKS))
def test_pick_and_budget_keys_hold_what_they_say(keys, name):
    """BudgetKey: resolution, depth and spp, what sizes the workspaces per pixel.  PickKey: everything of the request but
    row_block (it owns no buffer).  TileOrderKey: everything of PickKey but the flags, and row_block."""
    cs = W.calls(W.WALKS[name][1])
    cfg = [ints(W.frame_config(c, W.SCHED_TILE)) for c in cs]
    for i, a in enumerate(cs):
        for j, b in enumerate(cs):
            ma, mb = W.META[a["fixture"]], W.META[b["fixture"]]
            sized = lambda m: (m["res"], m["max_depth"], m["spp"])
            request = lambda c, m: (sized(m), m["accel"], m["soft_shadow"], c["rank"], c["world"])
            assert bool(keys.budget_key_equal(cfg[i], cfg[j])) == (sized(ma) == sized(mb))
            assert bool(keys.pick_key_equal(cfg[i], cfg[j])) == ((request(a, ma), a["no_lds"]) == (request(b, mb), b["no_lds"]))
            assert bool(keys.tile_order_key_equal(cfg[i], cfg[j])) == ((request(a, ma), a["row_block"]) == (request(b, mb), b["row_block"]))


def mutant(field):
    """The header with TileOrderKey::operator== no longer comparing `field`."""
    with open(HEADER) as f:
        text = f.read()
    head, tail = text.split("struct TileOrderKey", 1)
    new, n = re.subn(r"\b%s == o\.%s &&\s*" % (field, field), "", tail, count=1)
    assert n == 1 and new != tail
    return head + "struct TileOrderKey" + new


@pytest.mark.parametrize("field", ["row_block", "world"])
def test_the_pair_check_catches_a_key_that_forgets_a_field(tmp_path, field):
    """CPU only: a library with such a key is never run on a GPU (a stale tile order is an out-of-bounds access)."""
    L = build_keys(tmp_path / field, mutant(field))
    bad, _ = key_violations(L, W.BH)
    assert bad, "a TileOrderKey without %s went unnoticed" % field
    s, a, b, ta, tb = bad[0]
    assert a[field] != b[field] and ta != tb
