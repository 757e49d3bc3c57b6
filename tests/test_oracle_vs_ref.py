"""Oracle restatement vs the REFERENCE'S OWN object code (oracle/_ref/libp3d_ref[_dN].so).

oracle/_ref is built by oracle/Makefile from the reference's sources compiled unchanged where they
lie: RT/vector.cpp, RT/boundingBox.cpp, RT/bvh.cpp, RT/grid.cpp, RT/scene.cpp:1-331 (the four
intercepts()/getNormal(), Scene accessors) and RT/main.cpp:471-730 (processLight, rayTracing,
sampleUnitDisk, with the globals of :40-103), one library per compile-time MAX_DEPTH.  Everything
compared here must agree BIT FOR BIT: vector/AABB/camera/quantiser/rand helpers, BVH and grid build
and traversals, the intersectors, single rayTracing() calls, whole frames (float bits, rgb8,
Ray::nextId) incl. the jittered/thin-lens sample loop and the SOFT_SHADOW / FUZZY_REFLECTION
branches, and the committed golden fixtures.

What the reference returns comes from `reference(key)`: computed live where the _ref libraries are
built, and then also checked against tests/golden/ref_vectors.npz; read from that file everywhere
else (tests/golden/make_ref_vectors.py writes it from the live functions below).  Arrays too large
to commit are stored as a sha256 digest of their shape, dtype and bytes.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, scene_path, synthetic_cube_map
from oracle import oracle_py as O
from oracle import ref_py as R
from oracle.ref_py import F, I
from scene_gen import write_scene

REF_VECTORS = os.path.join(GOLDEN, "ref_vectors.npz")
DIGEST_ABOVE_BYTES = 256 << 10       # make_ref_vectors.py: larger arrays are committed as a digest


def canon(a):
    """Integers as int64 (the two sides' C int widths differ), floats and uint8 as they are."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind in "bi" or (a.dtype.kind == "u" and a.dtype != np.uint8):
        a = a.astype(np.int64)
    return a


def digest(a):
    a = canon(a)
    return np.frombuffer(hashlib.sha256(("%s %s|" % (a.shape, a.dtype.str)).encode() + a.tobytes()).digest(), np.uint8)


class Digest:
    def __init__(self, d):
        self.d = np.asarray(d, np.uint8)


def same(ref, mine):
    """Bit-for-bit equality of the reference's array (or its committed digest) and ours."""
    if isinstance(ref, Digest):
        return np.array_equal(ref.d, digest(mine))
    a, b = canon(ref), canon(mine)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_stored = None


def stored(key):
    global _stored
    if _stored is None:
        with np.load(REF_VECTORS) as z:
            _stored = {k: z[k] for k in z.files}
    pre = key + "/"
    out = {}
    for k, v in _stored.items():
        if k.startswith(pre):
            name = k[len(pre):]
            if name.endswith("#sha256"):
                out[name[:-7]] = Digest(v)
            else:
                out[name] = v
    assert out, "no reference vectors for %s in %s" % (key, REF_VECTORS)
    return out


def reference(key, depth, live):
    """{name: array} the reference's object code returns for `key`: live() where oracle/_ref has the `depth` build,
    checked against the committed vectors; else the committed vectors (digests for the large arrays)."""
    if R.available(depth):
        got = live()
        for name, v in stored(key).items():
            assert name in got and same(v, got[name]), "%s/%s: live reference differs from %s" % (key, name, REF_VECTORS)
        return got
    return stored(key)


def rand_vecs(rng, n, scale=3.0):
    v = (rng.standard_normal((n, 3)) * scale).astype(np.float32)
    # sprinkle exact zeros / axis-aligned directions: the slab tests divide by them
    z = rng.random((n, 3)) < 0.05
    v[z] = 0.0
    return v


# ------------------------------------------------------------------ helpers (RT/vector.cpp, boundingBox.cpp, main.cpp)
def vector_ops_inputs():
    rng = np.random.default_rng(1)
    return rand_vecs(rng, 2000), rand_vecs(rng, 2000)


def live_vector_ops():
    ref = R.lib(4)
    a, b = vector_ops_inputs()
    out = np.zeros(20, np.float32)
    norm = np.zeros((len(a), 3), np.float32)
    for i in range(len(a)):
        ref.ref_vec_ops(F(a[i]), F(b[i]), F(out))
        norm[i] = out[17:20]
    return {"normalize": norm}


def test_vector_ops_bitexact():
    norm = reference("vector_ops", 4, live_vector_ops)["normalize"]
    a, _ = vector_ops_inputs()
    for i in range(len(a)):
        n = O.normalize(a[i])
        assert np.array_equal(norm[i].view(np.uint32), n.view(np.uint32))


def aabb_inputs():
    rng = np.random.default_rng(2)
    n = 20000
    lo = rand_vecs(rng, n, 2.0)
    hi = lo + np.abs(rand_vecs(rng, n, 1.5)) + np.float32(1e-3)
    o, d = rand_vecs(rng, n, 4.0), rand_vecs(rng, n, 1.0)
    return lo, hi, o, d


def live_aabb():
    ref = R.lib(4)
    lo, hi, o, d = aabb_inputs()
    t = np.zeros(1, np.float32)
    hit = np.zeros(len(lo), np.uint8)
    tt = np.zeros(len(lo), np.float32)
    for i in range(len(lo)):
        hit[i] = bool(ref.ref_aabb_intercepts(F(lo[i]), F(hi[i]), F(o[i]), F(d[i]), F(t)))
        tt[i] = t[0]
    return {"hit": hit, "t": tt}


def test_aabb_intercepts_bitexact():
    r = reference("aabb", 4, live_aabb)
    lo, hi, o, d = aabb_inputs()
    n = len(lo)
    hits = 0
    for i in range(n):
        h_or, t_or = O.aabb_intercepts(lo[i], hi[i], o[i], d[i])
        assert bool(r["hit"][i]) == h_or
        a, b = np.float32(r["t"][i]), np.float32(t_or)
        assert a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b))
        hits += h_or
    assert 0 < hits < n


def u8_inputs():
    xs = np.concatenate([np.linspace(-0.5, 1.5, 4001), np.arange(0, 256) / 255.99,
                         np.nextafter(np.arange(0, 256, dtype=np.float32) / np.float32(255.99), 2)])
    return xs.astype(np.float32)


def live_u8_rand():
    ref = R.lib(4)
    a = np.zeros(1000, np.float32)
    ref.ref_rand_floats(12345, 1000, F(a))
    return {"u8": np.array([ref.ref_u8fromfloat(float(x)) for x in u8_inputs()], np.uint8), "rand": a}


def test_u8fromfloat_and_rand():
    r = reference("u8_rand", 4, live_u8_rand)
    for x, u in zip(u8_inputs(), r["u8"]):
        assert int(u) == O.u8fromfloat(x)
    # RT/RT_Output.png is uniformly (19,92,192) = u8fromfloat of mount_low's bclr
    assert [O.u8fromfloat(v) for v in (0.078, 0.361, 0.753)] == [19, 92, 192]
    assert np.array_equal(r["rand"], O.rand_floats(12345, 1000))


# ------------------------------------------------------------------ camera (RT/main.cpp camera set-up, primary rays)
CAMERA_SCENES = ["mount_low", "balls_low", "dof", "dragon"]


def camera_setup(name):
    """[(w, h, cam6, [(px, py, lx, ly)] x 300)] for the scene's own resolution, 1920x1080 and 97x61; and cam9."""
    sc = O.Scene(scene_path(name))
    lines = open(scene_path(name)).read().split()
    k = lines.index("from")
    cam9 = np.array([float(lines[k + 1 + j]) for j in (0, 1, 2)] +
                    [float(lines[k + 5 + j]) for j in (0, 1, 2)] +
                    [float(lines[k + 9 + j]) for j in (0, 1, 2)], np.float32)
    g = lambda key: float(lines[lines.index(key, k) + 1])
    out = []
    for (w, h) in ((sc.res_x, sc.res_y), (1920, 1080), (97, 61)):
        cam6 = np.array([g("angle"), g("hither"), w, h, g("aperture"), g("focal")], np.float32)
        rng = np.random.default_rng(3)
        pts = []
        for _ in range(300):
            px, py = np.float32(rng.random() * w), np.float32(rng.random() * h)
            lx, ly = np.float32(rng.random() - .5), np.float32(rng.random() - .5)
            pts.append((px, py, lx, ly))
        out.append((w, h, cam6, pts))
    return cam9, out


def live_camera(name):
    ref = R.lib(4)
    cam9, setups = camera_setup(name)
    d19 = np.zeros((3, 19), np.float32)
    rays = np.zeros((3, 300, 4, 3), np.float32)            # o, d, o through the lens, d through the lens
    o = np.zeros(3, np.float32)
    d = np.zeros(3, np.float32)
    for s, (w, h, cam6, pts) in enumerate(setups):
        cam = ref.ref_camera_new(F(cam9), F(cam6), F(d19[s]))
        for j, (px, py, lx, ly) in enumerate(pts):
            ref.ref_camera_ray(cam, px, py, F(o), F(d))
            rays[s, j, 0], rays[s, j, 1] = o, d
            ref.ref_camera_ray_lens(cam, lx, ly, px, py, F(o), F(d))
            rays[s, j, 2], rays[s, j, 3] = o, d
        ref.ref_camera_free(cam)
    return {"d19": d19, "rays": rays}


@pytest.mark.parametrize("name", CAMERA_SCENES)
def test_camera_bitexact(name):
    r = reference("camera/" + name, 4, lambda: live_camera(name))
    sc = O.Scene(scene_path(name))
    _, setups = camera_setup(name)
    for s, (w, h, _, pts) in enumerate(setups):
        sc.set_resolution(w, h)
        assert np.array_equal(r["d19"][s].view(np.uint32), sc.camera().view(np.uint32))
        for j, (px, py, lx, ly) in enumerate(pts):
            o, d, ol, dl = r["rays"][s, j]
            oo, dd = sc.primary_ray(px, py)
            assert np.array_equal(o, oo) and np.array_equal(d.view(np.uint32), dd.view(np.uint32))
            oo, dd = sc.primary_ray_lens(lx, ly, px, py)
            assert np.array_equal(ol.view(np.uint32), oo.view(np.uint32))
            assert np.array_equal(dl.view(np.uint32), dd.view(np.uint32))


# ------------------------------------------------------------------ BVH / grid (RT/bvh.cpp, RT/grid.cpp)
def scene_rays(sc, rng, n):
    """Rays that exercise the accel structures: primary rays + rays between scene points."""
    t, d, _ = sc.prims()
    pts = d[:, :3]
    rays = []
    for _ in range(n // 2):
        rays.append(sc.primary_ray(np.float32(rng.random() * sc.res_x), np.float32(rng.random() * sc.res_y)))
    for _ in range(n - n // 2):
        a = pts[rng.integers(len(pts))] + rng.standard_normal(3).astype(np.float32) * np.float32(0.3)
        b = pts[rng.integers(len(pts))] + rng.standard_normal(3).astype(np.float32) * np.float32(0.3)
        rays.append((a.astype(np.float32), (b - a).astype(np.float32)))
    return [(O.f3(o), O.f3(dr)) for (o, dr) in rays]


ACCEL_CASES = [("mount_low", 3000), ("balls_low", 3000), ("balls_medium", 2000), ("balls_box", 2000),
               ("mount_high", 1500), ("dragon", 400)]


def live_accel(name, nrays):
    ref = R.lib(4)
    sc = O.Scene(scene_path(name))
    t, d, _ = sc.prims()
    t = np.ascontiguousarray(t, np.int32)
    acc = ref.ref_accel_new(len(t), I(t), F(d))
    n_nodes = ref.ref_bvh_build(acc)
    nodes = np.zeros((n_nodes, 8), np.float32)
    nobj = np.zeros(n_nodes, np.int32)
    order = np.zeros(len(t), np.int32)
    ref.ref_bvh_dump(acc, F(nodes), I(nobj), I(order))
    dims = np.zeros(3, np.int32)
    ref.ref_grid_build(acc, I(dims))
    cells = np.zeros(int(np.prod(dims.astype(np.int64))), np.int32)
    ref.ref_grid_cell_counts(acc, I(cells))
    # traversals, interleaved so the persistent hit_stack evolves as in the oracle
    rays = scene_rays(sc, np.random.default_rng(7), nrays)
    hits = np.zeros((len(rays), 6), np.int32)              # bvh ok, bvh obj, bvh shadow, grid shadow, grid ok, grid obj
    bvh_t = np.zeros(len(rays), np.float32)
    obj = np.zeros(1, np.int32)
    tt = np.zeros(1, np.float32)
    for i, (o, dr) in enumerate(rays):
        obj[0] = -1
        hits[i, 0] = bool(ref.ref_bvh_closest(acc, F(o), F(dr), I(obj), F(tt)))
        hits[i, 1], bvh_t[i] = obj[0], tt[0]
        hits[i, 2] = bool(ref.ref_bvh_shadow(acc, F(o), F(dr)))
        hits[i, 3] = bool(ref.ref_grid_shadow(acc, F(o), F(dr)))
        obj[0] = -1
        hits[i, 4] = bool(ref.ref_grid_closest(acc, F(o), F(dr), I(obj), F(tt)))
        hits[i, 5] = obj[0]
    ref.ref_accel_free(acc)
    return {"n_nodes": np.array([n_nodes]), "nodes": nodes, "nobj": nobj, "order": order, "dims": dims, "cells": cells,
            "hits": hits, "bvh_t": bvh_t}


@pytest.mark.parametrize("name,nrays", ACCEL_CASES)
def test_bvh_and_grid_restatement_match_reference_objects(name, nrays):
    r = reference("accel/" + name, 4, lambda: live_accel(name, nrays))
    sc = O.Scene(scene_path(name))
    # ---- BVH::Build: identical node array and object permutation
    nodes_o, nobj_o, order_o = sc.refbvh_dump()
    assert int(r["n_nodes"][0]) == len(nodes_o)
    assert same(r["nodes"], nodes_o)
    assert same(r["nobj"], nobj_o) and same(r["order"], order_o)
    # ---- Grid::Build: identical dimensions and cell populations
    dims_o, cells_o = sc.refgrid_dims(with_cells=True)
    assert same(r["dims"], dims_o)
    assert same(r["cells"], cells_o)
    # ---- traversals, in the same order as the reference's
    hits, bvh_t = r["hits"], r["bvh_t"]
    n_hit = n_shadow = 0
    for i, (o, dr) in enumerate(scene_rays(sc, np.random.default_rng(7), nrays)):
        ok_o, obj_o, t_o = sc.refbvh_closest(o, dr)
        assert bool(hits[i, 0]) == ok_o and int(hits[i, 1]) == obj_o
        if obj_o >= 0:
            assert np.float32(bvh_t[i]) == np.float32(t_o)
            n_hit += 1
        s_o = sc.refbvh_shadow(o, dr)
        assert bool(hits[i, 2]) == s_o
        n_shadow += s_o
        assert bool(hits[i, 3]) == sc.refgrid_shadow(o, dr)
        ok_o, obj_o, t_o = sc.refgrid_closest(o, dr)
        assert bool(hits[i, 4]) == ok_o and int(hits[i, 5]) == obj_o
    assert n_hit > 0 and n_shadow > 0


# ------------------------------------------------------------------ intersectors (RT/scene.cpp:55-283)
def load_kat():
    with np.load(os.path.join(GOLDEN, "kat.npz")) as z:
        return {name: z[name] for name in z.files}


def live_prim_bbox():
    k = load_kat()
    return {"bbox": np.stack([np.stack(R.prim_bbox(int(k["type"][i]), k["prim12"][i])) for i in range(0, len(k["type"]), 16)])}


def test_intersectors_and_bboxes_bitexact_vs_reference_objects():
    """The committed known-answer table (16 000 rays over the four primitive kinds) is what the
    reference's own intercepts()/getNormal() return, and the oracle agrees bit for bit."""
    k = load_kat()
    n = len(k["type"])
    assert n == 16000
    bbox = reference("prim_bbox", 4, live_prim_bbox)["bbox"]
    live = R.available(4)
    hits = 0
    for i in range(n):
        ty, p, o, d = int(k["type"][i]), k["prim12"][i], k["origin"][i], k["dir"][i]
        h_o, t_o, n_o = O.intersect(ty, p, o, d)
        assert h_o == bool(k["hit"][i]), i
        if live:
            h_r, t_r, n_r = R.intersect(ty, p, o, d)
            assert h_r == h_o, i
            if h_r:
                assert np.float32(t_r).view(np.uint32) == k["t"][i].view(np.uint32), i
                assert np.array_equal(n_r.view(np.uint32), k["normal"][i].view(np.uint32)), i
        if h_o:
            hits += 1
            assert np.float32(t_o).view(np.uint32) == k["t"][i].view(np.uint32), i
            assert np.array_equal(n_o.view(np.uint32), k["normal"][i].view(np.uint32)), i
        if i % 16 == 0:
            b = O.prim_bbox(ty, p)
            assert np.array_equal(bbox[i // 16][0].view(np.uint32), b[0].view(np.uint32))
            assert np.array_equal(bbox[i // 16][1].view(np.uint32), b[1].view(np.uint32))
    assert 3000 < hits < 13000


# ------------------------------------------------------------------ whole frames (RT/main.cpp:471-805)
CASES = json.load(open(os.path.join(GOLDEN, "cases.json")))


def _pair(case, res=None):
    path = scene_path(case["scene"])
    osc = O.Scene(path)
    osc.set_resolution(*(res or case["res"]))
    return osc, (R.RefScene.from_oracle_scene(osc, path, res=res or case["res"], depth=case["max_depth"])
                 if R.available(case["max_depth"]) else None)


def _same_frame(a, b, rows=slice(None)):
    assert same(b["hit_id"], a["hit_id"][rows])
    assert same(b["rgb32f"], a["rgb32f"][rows])
    assert same(b["rgb8"], a["rgb8"][rows])


def _frame(r, rows=slice(None)):
    """A reference frame's rows as committed: arrays + the ray count."""
    return {"hit_id": r["hit_id"][rows], "rgb32f": r["rgb32f"][rows], "rgb8": r["rgb8"][rows], "rays": np.array([r["rays"]])}


def golden_rows(case):
    # the dragon without culling is 1e5 virtual calls per ray: 16 rows of it are enough here,
    # tests/golden/make_golden.py renders (and checks) all of them
    H = case["res"][1]
    return (H // 2 - 8, H // 2 + 8) if case["scene"] == "dragon" else (0, 0)


def live_golden(name):
    case = CASES[name]
    _, rs = _pair(case)
    y0, y1 = golden_rows(case)
    r = rs.render(case["accel"], case["spp"], case["seed"], y0=y0, y1=y1)
    return _frame(r, slice(y0, y1) if y1 else slice(None))


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_frames_are_reference_output(name):
    """Every committed golden frame == the reference's own rayTracing() on the reference's own
    objects, in float bits, rgb8, primary hit ids and Ray::nextId; and the oracle produces the same."""
    case = CASES[name]
    r = reference("golden/" + name, case["max_depth"], lambda: live_golden(name))
    fr = np.load(os.path.join(GOLDEN, "frames.npz"))
    gold = {k: fr[name + "/" + k] for k in ("rgb8", "rgb32f", "hit_id")}
    osc = O.Scene(scene_path(case["scene"]))
    osc.set_resolution(*case["res"])
    y0, y1 = golden_rows(case)
    rows = slice(y0, y1) if y1 else slice(None)
    if "rgb8" in r:
        _same_frame(gold, r, rows)
    o = osc.render(max_depth=case["max_depth"], accel=case["accel"], spp=case["spp"], seed=case["seed"], y0=y0, y1=y1)
    _same_frame(o, _frame(dict(gold, rays=0), rows), rows)
    assert o["counters"]["rays"] == int(r["rays"][0])
    if not y1:
        assert int(r["rays"][0]) == case["counters"]["rays"]


def random_scene(seed, path):
    """Generated scene `seed` written to `path`: (accel, compile-time depth)."""
    rng = np.random.default_rng(1000 + seed)
    accel = int(rng.integers(0, 3))
    depth = int(rng.integers(1, 7))
    write_scene(path, rng, n_sph=int(rng.integers(0, 7)), n_tri=int(rng.integers(0, 9)), n_box=int(rng.integers(0, 3)),
                n_pl=int(rng.integers(0, 2)), n_lights=int(rng.integers(0, 4)), accel=accel)
    return accel, depth


def live_random(seed, path):
    accel, depth = random_scene(seed, path)
    rs = R.RefScene.from_oracle_scene(O.Scene(path), path, depth=depth)
    out = {}
    for acc in (accel, (accel + 1) % 3):
        out.update({"a%d_%s" % (acc, k): v for k, v in _frame(rs.render(acc)).items()})
    return out


@pytest.mark.parametrize("seed", range(24))
def test_random_scenes_oracle_equals_reference(tmp_path, seed):
    """Generated scenes over all four primitive kinds (incl. planes in GRID mode), three
    material kinds, 0-3 lights, every accel mode, compile-time depths 1-6."""
    path = str(tmp_path / "scene.p3f")
    accel, depth = random_scene(seed, path)
    r = reference("random/%d" % seed, depth, lambda: live_random(seed, path))
    osc = O.Scene(path)
    for acc in (accel, (accel + 1) % 3):
        ra = {k: r["a%d_%s" % (acc, k)] for k in ("hit_id", "rgb32f", "rgb8", "rays")}
        o = osc.render(max_depth=depth, accel=acc)
        _same_frame(o, ra)
        assert o["counters"]["rays"] == int(ra["rays"][0])


DIST_CASES = [
    ("mount_low", (64, 36), 2, 0, True, False),     # 4x4 area-light grid, deterministic (RT/main.cpp:601-618)
    ("balls_low", (48, 48), 0, 0, True, False),
    ("balls_low", (48, 48), 2, 0, False, True),     # fuzzy reflection draws rand() inside the recursion (:651-660)
    ("balls_low", (40, 40), 2, 2, True, True),      # jittered light per sample (:620-624) + fuzzy + thin lens
    ("dof", (40, 40), 1, 3, True, False),
    ("balls_box", (48, 48), 1, 0, True, True),
]


def dist_key(scene, res, accel, spp, soft, fuzzy):
    return "dist/%s_%dx%d_a%d_s%d_%d%d" % (scene, res[0], res[1], accel, spp, soft, fuzzy)


def live_dist(scene, res, accel, spp, soft, fuzzy):
    _, rs = _pair(dict(scene=scene, res=list(res), max_depth=4))
    return _frame(rs.render(accel, spp, 4242, soft_shadow=soft, fuzzy_reflection=fuzzy))


@pytest.mark.parametrize("scene,res,accel,spp,soft,fuzzy", DIST_CASES)
def test_distribution_switches_oracle_equals_reference(scene, res, accel, spp, soft, fuzzy):
    """SOFT_SHADOW / FUZZY_REFLECTION (compile-time false in the reference, plain globals in the object
    code) and the spp>0 sample loop: the serial rand() stream makes them bit-comparable."""
    r = reference(dist_key(scene, res, accel, spp, soft, fuzzy), 4, lambda: live_dist(scene, res, accel, spp, soft, fuzzy))
    osc = O.Scene(scene_path(scene))
    osc.set_resolution(*res)
    o = osc.render(max_depth=4, accel=accel, spp=spp, seed=4242, soft_shadow=soft, fuzzy_reflection=fuzzy)
    _same_frame(o, r)
    assert o["counters"]["rays"] == int(r["rays"][0])


def live_baseline_strips(depth):
    if depth == 4:
        _, rs = _pair(dict(scene="mount_low", res=[1920, 1080], max_depth=4))
        out = {}
        for accel in (2, 1):
            out.update({"a%d_%s" % (accel, k): v for k, v in _frame(rs.render(accel, y0=500, y1=560), slice(500, 560)).items()})
        return out
    _, rs = _pair(dict(scene="mount_low", res=[512, 512], max_depth=6))
    return _frame(rs.render(2, 2, 12345, y0=240, y1=272), slice(240, 272))


def test_baseline_configs_at_reduced_height_oracle_equals_reference():
    """BASELINE config 2 geometry (1920 wide, depth 4, BVH) on a 1920x60 strip, config 4's
    (depth 6, 2x2 samples) on 512x32, and GRID mode incl. the pixel it is known to differ in."""
    r = reference("baseline/d4", 4, lambda: live_baseline_strips(4))
    osc = O.Scene(scene_path("mount_low"))
    osc.set_resolution(1920, 1080)
    for accel in (2, 1):
        ra = {k: r["a%d_%s" % (accel, k)] for k in ("hit_id", "rgb32f", "rgb8", "rays")}
        o = osc.render(max_depth=4, accel=accel, y0=500, y1=560)
        _same_frame(o, ra, slice(500, 560))
        assert o["counters"]["rays"] == int(ra["rays"][0])
    r = reference("baseline/d6", 6, lambda: live_baseline_strips(6))
    osc.set_resolution(512, 512)
    o = osc.render(max_depth=6, accel=2, spp=2, seed=12345, y0=240, y1=272)
    _same_frame(o, r, slice(240, 272))
    assert o["counters"]["rays"] == int(r["rays"][0])


def skybox_dirs():
    rng = np.random.default_rng(17)
    d = rng.standard_normal((20000, 3)).astype(np.float32)
    d[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    d[6:12] = np.array([[1, 1, 0], [-1, 1, 0], [1, 0, 1], [0, 1, 1], [0, -1, 1], [1, 1, 1]], np.float32)
    d[12:10000] /= np.linalg.norm(d[12:10000], axis=1, keepdims=True)
    return d


def test_skybox_lookup_bitexact_vs_reference_object_code():
    """Scene::GetSkyboxColor (RT/scene.cpp:383-461): nothing in the reference calls it, but its object code
    exists and the oracle's restatement must equal it bit for bit -- 20 000 directions incl. the six axes, the face
    diagonals (the `>` / `>=` tie rules of the face choice) and un-normalised ones, over a synthetic cube map whose six
    faces differ in size and pixel width."""
    faces = synthetic_cube_map()
    d = skybox_dirs()
    ref = reference("skybox", 4, lambda: {"colors": R.skybox_colors(faces, d)})["colors"]
    sc = O.Scene(scene_path("mount_low"))
    sc.set_skybox(faces)
    mine = np.stack([sc.skybox_color(v) for v in d])
    assert same(ref, mine)
    assert len(np.unique(mine, axis=0)) > 5000


def live_trace():
    path = scene_path("balls_box")
    osc = O.Scene(path)
    rs = R.RefScene.from_oracle_scene(osc, path)
    rays = scene_rays(osc, np.random.default_rng(5), 600)
    return {"colors": np.stack([np.stack([rs.trace(accel, o, d) for (o, d) in rays]) for accel in (0, 1, 2)])}


def test_single_raytracing_calls_bitexact():
    """rayTracing(ray, 1, 1.0) on arbitrary (also non-unit, also inside-geometry) rays."""
    ref = reference("trace", 4, live_trace)["colors"]
    osc = O.Scene(scene_path("balls_box"))
    rays = scene_rays(osc, np.random.default_rng(5), 600)
    for accel in (0, 1, 2):
        for j, (o, d) in enumerate(rays):
            b = osc.trace(accel, o, d)
            assert np.array_equal(ref[accel, j].view(np.uint32), b.view(np.uint32))


def live_vectors(tmp_dir):
    """(key, depth, live) of every reference vector the tests above read: what make_ref_vectors.py records."""
    yield "vector_ops", 4, live_vector_ops
    yield "aabb", 4, live_aabb
    yield "u8_rand", 4, live_u8_rand
    for name in CAMERA_SCENES:
        yield "camera/" + name, 4, (lambda name=name: live_camera(name))
    for name, nrays in ACCEL_CASES:
        yield "accel/" + name, 4, (lambda name=name, nrays=nrays: live_accel(name, nrays))
    yield "prim_bbox", 4, live_prim_bbox
    for name in sorted(CASES):
        yield "golden/" + name, CASES[name]["max_depth"], (lambda name=name: live_golden(name))
    for seed in range(24):
        path = os.path.join(tmp_dir, "scene_%d.p3f" % seed)
        yield "random/%d" % seed, random_scene(seed, path)[1], (lambda seed=seed, path=path: live_random(seed, path))
    for c in DIST_CASES:
        yield dist_key(*c), 4, (lambda c=c: live_dist(*c))
    yield "baseline/d4", 4, lambda: live_baseline_strips(4)
    yield "baseline/d6", 6, lambda: live_baseline_strips(6)
    yield "skybox", 4, lambda: {"colors": R.skybox_colors(synthetic_cube_map(), skybox_dirs())}
    yield "trace", 4, live_trace
