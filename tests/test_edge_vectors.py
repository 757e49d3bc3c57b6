"""The edge-case battery of tests/edge_cases.py on the CPU: the oracle against the reference's object code, and the battery
against itself.

What the reference answers comes from tests/golden/edge_vectors.npz (tests/golden/make_edge_vectors.py records it from the
functions below) and, where oracle/_ref is built, from live calls that are then also checked against the file -- the
`reference()` pattern of tests/test_oracle_vs_ref.py.  Every comparison is on bits, except that a NaN matches any NaN (sign
and payload of a NaN differ between x86 and the GPU).  The file holds results only: its inputs are a sha256 of what
edge_cases.py generates, so a drift of the battery is caught here.

tests/test_gpu_edge_rays.py imports the references computed here (once per process, read-only).
"""
import ctypes as C
import os
import tempfile

import numpy as np

from conftest import GOLDEN
from oracle import oracle_py as O
from oracle import ref_py as R
from oracle.ref_py import F, I
import edge_cases as E
import occlusion_refs as OR

EDGE_VECTORS = os.path.join(GOLDEN, "edge_vectors.npz")
DEPTHS = (1, 3)
ACCELS = (0, 1, 2)
_cache = {}


def same(a, b):
    """[n] bool: rows of a and b equal in every bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    eq = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return eq.reshape(len(a), -1).all(-1)


def assert_same(got, ref, what, names=None):
    ok = same(got, ref)
    if names is not None:
        for k, sl in names.items():
            if not ok[sl].all():
                print("%s: family %s differs in %d of %d" % (what, k, int((~ok[sl]).sum()), sl.stop - sl.start))
    i = int(np.argmin(ok))
    assert ok.all(), "%s: %d of %d differ, first %d: %s vs %s" % (what, int((~ok).sum()), len(ok), i, got[i], ref[i])


# ------------------------------------------------------------------ the scene and its grid
def scene_file():
    """edge_lattice.p3f, written once per process into a directory that lives as long as the process."""
    if "path" not in _cache:
        _cache["tmp"] = tempfile.TemporaryDirectory()
        _cache["path"] = E.write_edge_lattice(os.path.join(_cache["tmp"].name, "edge_lattice.p3f"))
    return _cache["path"]


def scene():
    if "osc" not in _cache:
        _cache["osc"] = O.Scene(scene_file())
    return _cache["osc"]


def grid_of(osc):
    """The box and dimensions of Grid::Build (RT/grid.cpp:38-65) from the oracle: the union of the primitives' boxes grown by
    EPSILON in float, and the oracle's cell counts."""
    ptype, prim, _ = osc.prims()
    boxes = [O.prim_bbox(int(ptype[j]), prim[j]) for j in range(len(ptype))]
    mn = np.min([b[0] for b in boxes], axis=0).astype(np.float32) - E.EPS
    mx = np.max([b[1] for b in boxes], axis=0).astype(np.float32) + E.EPS
    return {"mn": mn.astype(np.float32), "mx": mx.astype(np.float32), "dims": np.asarray(osc.refgrid_dims(), np.int32)}


def grid():
    if "grid" not in _cache:
        _cache["grid"] = grid_of(scene())
    return _cache["grid"]


def rays():
    """(origin, dir, {family: slice}) of the whole battery on edge_lattice."""
    if "rays" not in _cache:
        _cache["rays"] = E.battery(grid())
    return _cache["rays"]


def mask(accel):
    o, d, where = rays()
    return E.mode_mask(o, d, where, grid(), accel)


def inputs_digest():
    kind, prim, po, pd = E.pairs()
    o, d, _ = rays()
    text = np.frombuffer(open(scene_file(), "rb").read(), np.uint8)
    return E.digest(kind, prim, po, pd, o, d, text)


# ------------------------------------------------------------------ the oracle's side
_fp = C.POINTER(C.c_float)


def intersect_all(fn, kind, prim, o, d):
    """(hit [n] uint8, t [n], normal [n, 3]) of an intersect function with p3o_intersect's signature; t and normal are 0
    where it reports no hit."""
    n = len(kind)
    hit, t, nrm = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    prim, o, d = (np.ascontiguousarray(a, np.float32) for a in (prim, o, d))
    tt, nn = np.zeros(1, np.float32), np.zeros(3, np.float32)
    pt, pn = tt.ctypes.data_as(_fp), nn.ctypes.data_as(_fp)
    for i in range(n):
        nn[:] = 0
        if fn(int(kind[i]), prim[i].ctypes.data_as(_fp), o[i].ctypes.data_as(_fp), d[i].ctypes.data_as(_fp), pt, pn):
            hit[i], t[i], nrm[i] = 1, tt[0], nn
    return hit, t, nrm


def oracle_pairs():
    if "opairs" not in _cache:
        r = intersect_all(O.lib().p3o_intersect, *E.pairs())
        for a in r:
            a.setflags(write=False)
        _cache["opairs"] = r
    return _cache["opairs"]


def brute_force_closest(o, d):
    """rayTracing()'s own loop (RT/main.cpp:567-574) on rays o, d [n, 3]: O.intersect on every primitive of edge_lattice in
    scene order, `t < closest_t` from FLT_MAX, so the lowest index wins a tie and a NaN or infinite t is never taken.
    -> (hit_id [n] int32, -1 for none; t, +inf for none; normal, 0 for none; n_tied [n]: primitives whose t has the winner's
    bits; nan_hits [n]: primitives that report a hit with a NaN t)."""
    ptype, prim, _ = scene().prims()
    n, m = len(o), len(ptype)
    hid, t = np.full(n, -1, np.int32), np.full(n, np.inf, np.float32)
    nrm, tied = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    nan_hits = np.zeros(n, np.int32)
    for i in range(n):
        h, tt, nn = intersect_all(O.lib().p3o_intersect, ptype, prim, np.broadcast_to(o[i], (m, 3)), np.broadcast_to(d[i], (m, 3)))
        best = E.FLT_MAX
        for j in np.flatnonzero(h):
            if tt[j] < best:
                best, hid[i], t[i], nrm[i] = tt[j], j, tt[j], nn[j]
        if hid[i] >= 0:
            tied[i] = int(((h == 1) & (tt.view(np.uint32) == t[i:i + 1].view(np.uint32))).sum())
        nan_hits[i] = int(((h == 1) & np.isnan(tt)).sum())
    for a in (hid, t, nrm, tied, nan_hits):
        a.setflags(write=False)
    return hid, t, nrm, tied, nan_hits


def brute_closest():
    """brute_force_closest on the battery's rays, once per process."""
    if "closest" not in _cache:
        o, d, _ = rays()
        _cache["closest"] = brute_force_closest(o, d)
    return _cache["closest"]


def grid_closest():
    """GRID mode's closest hit is Grid::Traverse's, not the brute force (per-cell candidates, planes only inside their default
    box): the oracle's restatement of it, with t and normal from O.intersect on the primitive it names."""
    if "gclosest" not in _cache:
        osc = scene()
        o, d, _ = rays()
        ptype, prim, _ = osc.prims()
        keep = mask(1)
        n = len(o)
        hid, t, nrm = np.full(n, -1, np.int32), np.full(n, np.inf, np.float32), np.zeros((n, 3), np.float32)
        for i in np.flatnonzero(keep):
            ok, obj, _ = osc.refgrid_closest(o[i], d[i])
            if ok and obj >= 0:
                h, tt, nn = O.intersect(int(ptype[obj]), prim[obj], o[i], d[i])
                assert h
                hid[i], t[i], nrm[i] = obj, tt, nn
        for a in (hid, t, nrm):
            a.setflags(write=False)
        _cache["gclosest"] = (hid, t, nrm)
    return _cache["gclosest"]


def oracle_rays():
    """What the oracle answers where the fixture has the reference: {trace [3][2][n][3], bvh_shadow [n], grid_shadow [n]}.
    Rays a mode leaves out keep zeros."""
    if "orays" not in _cache:
        o, d, _ = rays()
        n = len(o)
        trace = np.zeros((3, len(DEPTHS), n, 3), np.float32)
        for k, depth in enumerate(DEPTHS):
            osc = O.Scene(scene_file())
            for accel in ACCELS:
                for i in np.flatnonzero(mask(accel)):
                    trace[accel, k, i] = osc.trace(accel, o[i], d[i], max_depth=depth)
        osc = O.Scene(scene_file())
        bvh, grd = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for i in range(n):
            bvh[i] = osc.refbvh_shadow(o[i], d[i])
        for i in np.flatnonzero(mask(1)):
            grd[i] = osc.refgrid_shadow(o[i], d[i])
        out = {"trace": trace, "bvh_shadow": bvh, "grid_shadow": grd}
        for a in out.values():
            a.setflags(write=False)
        _cache["orays"] = out
    return _cache["orays"]


def none_shadow():
    """NONE mode's shadow answer by the rule of tests/occlusion_refs.py: any intercepts() at all, direction as given."""
    if "none" not in _cache:
        o, d, _ = rays()
        ptype, prim, _ = scene().prims()
        with np.errstate(over="ignore"):                         # the scale family's lengths overflow, as in the reference
            r = OR.brute_force(ptype, prim, o, d, False)
        r.setflags(write=False)
        _cache["none"] = r
    return _cache["none"]


def bounded_any_hit():
    """Brute-force any-hit with BVH::Traverse(Ray&)'s acceptance (normalised direction, t < |dir|) over the primitives
    themselves, no tree in between; planes only where the ray meets their default [-1, 1]^3 box (AABB::intercepts), as the
    reference's tree and include/p3d_hip.h have it.  This is what p3d_occluded documents for BVH mode."""
    if "bounded" not in _cache:
        o, d, _ = rays()
        ptype, prim, _ = scene().prims()
        with np.errstate(over="ignore"):
            r = OR.brute_force(ptype[ptype != E.PLANE], prim[ptype != E.PLANE], o, d, True)
            lens = OR.length(d)
        one = np.ones(3, np.float32)
        for i in np.flatnonzero(r == 0):
            dn = O.normalize(d[i])
            if O.aabb_intercepts(-one, one, o[i], dn)[0]:
                for j in np.flatnonzero(ptype == E.PLANE):
                    h, t, _ = O.intersect(E.PLANE, prim[j], o[i], dn)
                    if h and np.float32(t) < lens[i]:
                        r[i] = 1
        r.setflags(write=False)
        _cache["bounded"] = r
    return _cache["bounded"]


# ------------------------------------------------------------------ the reference's side
def live_edge_vectors():
    """Everything the fixture holds, from the reference's object code in oracle/_ref."""
    kind, prim, po, pd = E.pairs()
    hit, t, nrm = intersect_all(R.lib(4).ref_intersect, kind, prim, po, pd)
    out = {"inputs_sha256": inputs_digest(), "pairs/hit": hit, "pairs/t": t, "pairs/normal": nrm}
    o, d, _ = rays()
    n = len(o)
    osc = scene()
    trace = np.zeros((3, len(DEPTHS), n, 3), np.float32)
    for k, depth in enumerate(DEPTHS):
        rs = R.RefScene.from_oracle_scene(osc, scene_file(), depth=depth)
        for accel in ACCELS:
            for i in np.flatnonzero(mask(accel)):
                trace[accel, k, i] = rs.trace(accel, o[i], d[i])
        rs.close()
    out["rays/trace"] = trace
    ref = R.lib(4)
    ptype, pdata, _ = osc.prims()
    ptype = np.ascontiguousarray(ptype, np.int32)
    acc = ref.ref_accel_new(len(ptype), I(ptype), F(pdata))
    ref.ref_bvh_build(acc)
    dims = np.zeros(3, np.int32)
    ref.ref_grid_build(acc, I(dims))
    assert np.array_equal(dims, grid()["dims"])
    bvh, grd = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        bvh[i] = bool(ref.ref_bvh_shadow(acc, F(np.ascontiguousarray(o[i])), F(np.ascontiguousarray(d[i]))))
    for i in np.flatnonzero(mask(1)):
        grd[i] = bool(ref.ref_grid_shadow(acc, F(np.ascontiguousarray(o[i])), F(np.ascontiguousarray(d[i]))))
    ref.ref_accel_free(acc)
    out["rays/bvh_shadow"], out["rays/grid_shadow"] = bvh, grd
    return out


def reference():
    """The reference's answers: the committed file, and where oracle/_ref is built the live ones checked against it."""
    if "ref" not in _cache:
        with np.load(EDGE_VECTORS) as z:
            stored = {k: z[k] for k in z.files}
        assert np.array_equal(stored["inputs_sha256"], inputs_digest()), \
            "tests/edge_cases.py no longer generates what %s was recorded for: run tests/golden/make_edge_vectors.py" % EDGE_VECTORS
        if all(R.available(dep) for dep in DEPTHS + (4,)):
            live = live_edge_vectors()
            assert sorted(live) == sorted(stored)
            for k, v in stored.items():
                if v.dtype == np.float32:
                    assert same(v.reshape(-1, 1), live[k].reshape(-1, 1)).all(), "%s: the live reference differs from the file" % k
                else:
                    assert np.array_equal(v, live[k]), "%s: the live reference differs from the file" % k
        for a in stored.values():
            a.setflags(write=False)
        _cache["ref"] = stored
    return _cache["ref"]


# ------------------------------------------------------------------ 1. the oracle against the reference
def test_oracle_intersectors_equal_the_reference_on_every_pair():
    ref = reference()
    hit, t, nrm = oracle_pairs()
    kind = E.pairs()[0]
    for k in range(4):
        m = kind == k
        print("%-8s %6d pairs, %5d hits, %5d with a non-finite t" % (E.TYPE_NAMES[k], int(m.sum()), int(hit[m].sum()),
                                                                      int((hit[m] == 1).sum() - np.isfinite(t[m][hit[m] == 1]).sum())))
    assert np.array_equal(hit, ref["pairs/hit"]), np.flatnonzero(hit != ref["pairs/hit"])[:5]
    assert_same(t, ref["pairs/t"], "t")
    assert_same(nrm, ref["pairs/normal"], "normal")


def test_oracle_rays_equal_the_reference_in_every_mode():
    ref, mine = reference(), oracle_rays()
    _, _, where = rays()
    for accel in ACCELS:
        for k, depth in enumerate(DEPTHS):
            assert_same(mine["trace"][accel, k], ref["rays/trace"][accel, k], "rayTracing() accel %d depth %d" % (accel, depth), where)
    for name in ("bvh_shadow", "grid_shadow"):
        bad = np.flatnonzero(mine[name] != ref["rays/" + name])
        assert len(bad) == 0, "%s: %d rays differ, first %s" % (name, len(bad), bad[:5])


def test_oracle_closest_hit_is_the_brute_force_in_scene_order(tmp_path):
    """The hit id the oracle's render path reports (its rayTracing() loop, accel NONE and BVH: SURVEY Q1) against the brute
    force over O.intersect, id for id, on the primary rays of edge_lattice seen straight down -z from (0, 0, 8) at 65 x 33.
    The centre column's rays have d.x == 0 and run down the plane x == 0, which is an edge shared by quads (and at y == 0,
    +-1 a vertex shared by up to eight triangles), so two or more primitives return the same t bits there: an oracle that
    took the farther primitive, or any but the lowest index on a tie, fails."""
    path = E.write_edge_lattice(str(tmp_path / "edge_lattice_down.p3f"), eye=(0.0, 0.0, 8.0), at=(0.0, 0.0, 0.0), res=(65, 33))
    sc = O.Scene(path)
    rays_ = [sc.primary_ray(np.float32(x + 0.5), np.float32(y + 0.5)) for y in range(33) for x in range(65)]
    o, d = np.stack([r[0] for r in rays_]), np.stack([r[1] for r in rays_])
    assert (d.reshape(33, 65, 3)[:, 32, 0] == 0).all(), "the centre column must run in the plane x == 0"
    hid, t, _, tied, _ = brute_force_closest(o, d)
    n_tied = int((tied >= 2).sum())
    print("%d primary rays: %d hit, %d with two or more primitives at the winning t" % (len(o), int((hid >= 0).sum()), n_tied))
    # the quads' shared edge x == 0 spans y in [-1, 1]: at 0.176 per pixel that is about 11 pixels of the centre column
    # (no misses: seen from above, the plane z == -0.75 is behind everything)
    assert n_tied >= 8 and len(np.unique(hid)) >= 30 and len(np.unique(scene().prims()[0][hid])) == 4
    for accel in (0, 2):
        got = sc.render(max_depth=1, accel=accel)["hit_id"].reshape(-1)
        bad = np.flatnonzero(got != hid)
        assert len(bad) == 0, "accel %d: %d primary hit ids differ from the brute force, first %s: %s vs %s" % (
            accel, len(bad), bad[:8], got[bad[:8]], hid[bad[:8]])
    # on the battery itself the oracle's trace path returns colours only: a miss of the brute force must give the background
    hid, _, _, _, _ = brute_closest()
    bg = sc.bg()
    trace = oracle_rays()["trace"]
    miss = hid < 0
    for accel in (0, 2):
        assert same(trace[accel, 0][miss], np.broadcast_to(bg, (int(miss.sum()), 3))).all(), "a miss must give the background"


# ------------------------------------------------------------------ 2. the battery's own properties
def test_pairs_keep_their_properties():
    kind, prim, o, d = E.pairs()
    hit, t, _ = oracle_pairs()
    n = len(kind)
    assert n >= 46080 and (kind <= 3).all()
    for k in range(4):
        m = kind == k
        h = hit[m] == 1
        n_nan, n_inf = int(np.isnan(t[m][h]).sum()), int(np.isinf(t[m][h]).sum())
        print("%-8s %6d pairs: %5d hits, %5d misses, %4d NaN t, %4d infinite t" % (E.TYPE_NAMES[k], int(m.sum()), int(h.sum()), int((~h).sum()), n_nan, n_inf))
        assert h.sum() >= 50 and (~h).sum() >= 50, E.TYPE_NAMES[k]
        # a triangle's and a box's t pass `> EPS` and a finite-input plane's t is a finite quotient: only a sphere reports a
        # hit with a NaN t (0 / 0 for a zero direction, inf - inf for a huge one); a box reports infinite ones
        if k == E.SPHERE:
            assert n_nan >= 100, "NaN-t hits of spheres are gone"
        if k in (E.SPHERE, E.BOX):
            assert n_inf >= 100, "hits with an infinite t of %s are gone" % E.TYPE_NAMES[k]
    # every wave of 64 mixes the kinds; some wave's triangle lanes mix frcp()'s plain path with the division
    full = n // 64 * 64
    waves = kind[:full].reshape(-1, 64)
    assert all(len(np.unique(w)) >= 3 for w in waves)
    e1, e2 = prim[:, 3:6] - prim[:, 0:3], prim[:, 6:9] - prim[:, 0:3]
    with np.errstate(all="ignore"):
        det = (e1 * np.cross(d, e2).astype(np.float32)).sum(1).astype(np.float32)
    plain = ((det.view(np.uint32) & 0x7f800000) - 0x00800000).astype(np.uint32) < 0x7e000000
    tri = (kind[:full] == E.TRIANGLE).reshape(-1, 64)
    mixed = sum(1 for w, p in zip(tri, plain[:full].reshape(-1, 64)) if w.any() and p[w].any() and (~p[w]).any())
    print("waves whose triangle lanes mix frcp()'s two paths: %d of %d" % (mixed, len(waves)))
    assert mixed >= 100
    # the determinant cases sit where they were put
    big = (kind == E.TRIANGLE) & (np.abs(det) >= np.float32(2.0 ** 126)) & (hit == 1)
    at_eps = (kind == E.TRIANGLE) & (np.abs(det) == E.EPS)
    assert big.sum() >= 4 and at_eps.sum() >= 4 and (hit[at_eps] == 1).any()


def test_ray_families_keep_their_properties():
    o, d, where = rays()
    g = grid()
    hid, t, _, tied, nan_hits = brute_closest()
    print("grid %s box %s .. %s" % (g["dims"], g["mn"], g["mx"]))
    for line in E.exclusion_report(o, d, where, g):
        print(line)
    assert 1500 <= len(o) <= 5500
    ties = E.dda_ties(o, d, g)
    entry = E.grid_entry(o, d, g)
    planes_x = np.array([E.cell_plane(g, 0, k) for k in range(int(g["dims"][0]) + 1)], np.float32)
    for k in E.FAMILIES:
        sl = where[k]
        n = sl.stop - sl.start
        hits, two, nan = int((hid[sl] >= 0).sum()), int((tied[sl] >= 2).sum()), int((nan_hits[sl] > 0).sum())
        on_plane = int(((d[sl][:, 0] == 0) & np.isin(o[sl][:, 0], planes_x)).sum())
        print("family %-10s %5d rays: %4d hit, %4d miss, %3d with two primitives at the winning t, %4d with a NaN-t intercept, "
              "%3d with d.x == 0 on a cell plane, %4d with a DDA tie" % (k, n, hits, n - hits, two, nan, on_plane, int((ties[sl] >= 2).sum())))
        assert 24 <= n <= 1200, k
        if k != "outside":
            assert hits >= 1, k
        assert n - hits >= 1, k
    assert (hid[where["outside"]] < 0).sum() >= 20 and not entry["enters"][where["outside"]].any(), "outside must miss the grid's box"
    # floors under what the families were built to hold, so that none of them degenerates quietly (the literal "every
    # property in every family" cannot hold: `outside` never enters the grid, only zero, overflowing or NaN inputs give a
    # NaN t, and `ties`, `on_surface` and `outside` place no origin on a cell plane)
    for k, floor in (("ties", 20), ("axis", 8), ("diagonal", 3), ("on_surface", 2), ("nonfinite", 3)):
        assert (tied[where[k]] >= 2).sum() >= floor, "equal t on two primitives in " + k
    assert (nan_hits[where["nonfinite"]] > 0).all(), "a NaN or an infinity in a ray makes some sphere's t NaN"
    assert (nan_hits[where["scale"]] > 0).sum() >= 200
    # NaN-t intercepts need a zero direction (on_surface, outside) or products that overflow (scale)
    for k in ("outside", "on_surface", "scale"):
        assert (nan_hits[where[k]] > 0).sum() >= 1, "NaN-t intercepts in " + k
    for k in ("axis", "diagonal", "scale"):
        sl = where[k]
        assert ((d[sl][:, 0] == 0) & np.isin(o[sl][:, 0], planes_x)).sum() >= 100, k
    # two zero components tie at FLT_MAX behind the live axis (grid_step's fall-through to z); a tie for the NEXT plane
    # needs a diagonal through a cell corner
    for k, floor in (("diagonal", 80), ("scale", 60), ("axis", 1), ("nonfinite", 1)):
        assert (ties[where[k]] >= 2).sum() >= floor, "DDA ties in " + k
    assert (ties[where["diagonal"]] == 3).sum() >= 1, "a three-way tie"
    fin = np.isfinite(o[where["nonfinite"]]).all(1) & np.isfinite(d[where["nonfinite"]]).all(1)
    assert not fin.any()


def test_shadow_columns_are_not_trivial_and_the_tree_keeps_the_headers_promise():
    """p3d_occluded's header promises BVH mode the answer of BVH::Traverse(Ray&).  Where that differs from an any-hit over the
    primitives themselves the reference's tree, not an intersector, decided: those rays stay in the battery and are counted."""
    ref = reference()
    o, d, where = rays()
    bvh, grd, none = ref["rays/bvh_shadow"], ref["rays/grid_shadow"], none_shadow()
    keep = mask(1)
    brute = bounded_any_hit()
    for k in E.FAMILIES:
        sl = where[k]
        print("family %-10s shadowed: NONE %4d, BVH %4d, GRID %4d of %4d run; BVH differs from the primitives' any-hit on %d" % (
            k, int(none[sl].sum()), int(bvh[sl].sum()), int(grd[sl][keep[sl]].sum()), int(keep[sl].sum()),
            int((bvh[sl] != brute[sl]).sum())))
    # the rays on which the tree and the primitives disagree: the reference answers "not in shadow", the primitives "in
    # shadow", and all of them start on a primitive's bounding box -- six on the lattice sphere of `on_surface`, leaving it
    # outwards or running along the box's face, and the `nonfinite` ray whose origin has a NaN z inside box A.  Anything else is a bug of bounded_any_hit or a
    # drift of the recorded column.
    differ = np.flatnonzero(bvh != brute)
    assert (bvh[differ] == 0).all() and (brute[differ] == 1).all()
    in_family = {k: int(((differ >= where[k].start) & (differ < where[k].stop)).sum()) for k in E.FAMILIES}
    assert in_family == dict({k: 0 for k in E.FAMILIES}, on_surface=6, nonfinite=1), in_family
    centre, r = np.float32([-1.5, -1.5, 0]), np.float32(E.LATTICE_R)
    for i in differ[differ < where["on_surface"].stop]:
        assert (np.abs(o[i] - centre).max() == r) and ((o[i] - centre) @ d[i] >= 0), "not on that sphere's box and heading off it: ray %d" % i
    assert 0.05 < bvh.mean() < 0.95 and 0.05 < none.mean() < 0.95
    assert grd[where["outside"]][keep[where["outside"]]].all(), "a segment that misses the grid's box is in shadow (RT/grid.cpp:327-328)"
    assert not grd[keep].all()
    sl = where["scale"]
    assert bvh[sl].sum() >= 10 and grd[sl][keep[sl]].sum() >= 10, "scale must hold occluded segments in BVH and GRID mode too"
