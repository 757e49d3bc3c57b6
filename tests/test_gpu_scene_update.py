"""p3d_scene_update on the GPU: a handle whose primitives (and lights) were moved in place renders, in every float bit and
on every pixel, what a handle freshly created from the moved scene renders, and what the oracle renders of it.

Every test writes scene A and scene B (same primitives, same order, moved geometry) as .p3f files, takes the arrays from
HostScene(...).arrays() and first asserts its own preconditions -- A's frame differs from B's in at least 5 % of the
pixels, and every moved bounded primitive's new bounding box is disjoint from its old one -- so that an update that does
nothing, or records written without a refit, cannot pass.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import RGB_TOL
from extra_scenes import scene_path
from oracle import oracle_py as O
import scene_motion as M
from scene_gen import write_scene
import test_oracle_vs_ref as OVR
import u_4a_2s_p3d_raytracer_template2_amd as P
from u_4a_2s_p3d_raytracer_template2_amd import api

pytestmark = pytest.mark.gpu

assert RGB_TOL == 0.0
ERR_ARG, ERR_STATE = -1, -5
RES = (96, 64)
SCHEDULES = (dict(wavefront=True), dict(tile=True), dict(tree=True))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, ref, what, rays=False):
    """rgb32f bits and hit ids of every pixel (and the ray count)."""
    bad = (bits(got["rgb32f"]) != bits(ref["rgb32f"])).any(-1)
    assert not bad.any(), "%s: %d pixels differ in rgb32f" % (what, int(bad.sum()))
    assert np.array_equal(got["hit_id"], ref["hit_id"]), "%s: hit ids differ" % what
    if rays:
        assert got["counters"]["rays"] == ref["counters"]["rays"], "%s: ray counts differ" % what


class Moving:
    """Scene files A and B, their flattened arrays, and a camera at the tests' resolution."""

    def __init__(self, path_a, path_b, res=RES):
        self.path = {"A": path_a, "B": path_b}
        self.res = res
        self.host = {k: P.HostScene(p) for k, p in self.path.items()}
        for h in self.host.values():
            h.set_resolution(*res)
        self.cam = self.host["A"].camera()
        self.arr = {k: h.arrays() for k, h in self.host.items()}
        self.ptype = self.arr["A"][0]
        assert np.array_equal(self.ptype, self.arr["B"][0]) and np.array_equal(self.arr["A"][2], self.arr["B"][2])
        self.data = {k: a[1] for k, a in self.arr.items()}
        self.lights = {k: a[4] for k, a in self.arr.items()}
        self.moved = np.flatnonzero((bits(self.data["A"]) != bits(self.data["B"])).any(-1))
        self._oracle = {}

    def fresh(self, which, **kw):
        return P.DeviceScene.from_host(self.host[which], **kw)

    def oracle(self, which, accel=2, depth=4, **kw):
        k = (which, accel, depth, tuple(sorted(kw.items())))
        if k not in self._oracle:
            sc = O.Scene(self.path[which])
            sc.set_resolution(*self.res)
            self._oracle[k] = sc.render(max_depth=depth, accel=accel, **kw)
            sc.close()
        return self._oracle[k]

    def preconditions(self, frame_a, frame_b, moved=None):
        M.assert_frames_differ(frame_a["rgb32f"], frame_b["rgb32f"])
        M.assert_boxes_disjoint(self.ptype, self.data["A"], self.data["B"], self.moved if moved is None else moved)


def mixed(tmp_path, seed=21):
    """About 6 spheres, 8 triangles, 2 boxes, 1 plane and 2 lights, served from LDS; in B everything has moved."""
    a, b = str(tmp_path / "mixed_a.p3f"), str(tmp_path / "mixed_b.p3f")
    write_scene(a, np.random.default_rng(seed), 6, 8, 2, 1, 2, 2)

    def move(kind, k, v):
        if kind == "l":
            return v + np.array([1.5, -2.0, 1.0, 0, 0, 0])
        if kind == "pl":
            return v + np.tile([0, 0, -0.35], 3)
        return M.shift_out_of_own_box(kind, v)
    M.rewrite_p3f(a, b, move)
    return Moving(a, b)


def lattice(tmp_path, seed=4):
    """600 triangles, 12 spheres and a floor plane read from HBM (direct triangle / sphere runs, several workgroups of leaves); in B every
    primitive sits where another one was."""
    a, b = str(tmp_path / "lattice_a.p3f"), str(tmp_path / "lattice_b.p3f")
    cells = M.write_lattice_scene(a, np.random.default_rng(seed), res=RES)
    target = np.roll(cells, len(cells) // 2 + 1)

    def move(kind, k, v):
        if kind in ("l", "pl"):
            return None
        (x0, y0), (x1, y1) = M.lattice_cell(int(cells[k])), M.lattice_cell(int(target[k]))
        step = np.array([x1 - x0, y1 - y0, 0.0])
        out = v.copy()
        if kind == "s":
            out[:3] += step
        else:
            out += np.tile(step, 3)
        return out
    M.rewrite_p3f(a, b, move)
    return Moving(a, b)


# ---- 1. small mixed scene served from LDS

def test_mixed_scene_from_lds_every_schedule_and_accel(tmp_path):
    m = mixed(tmp_path)
    assert len(m.moved) == len(m.ptype) and (m.ptype == 3).sum() == 1
    m.preconditions(m.oracle("A"), m.oracle("B"))
    ds, fresh = m.fresh("A"), m.fresh("B")
    assert_same(ds.render(m.cam, accel=2, counters=True), m.oracle("A"), "before the update", rays=True)
    ds.update(m.data["B"], lights6=m.lights["B"])
    for accel in (0, 2):
        ref = m.oracle("B", accel=accel)
        for sched in SCHEDULES:
            for no_lds in (False, True):
                what = "accel %d %s no_lds %d" % (accel, list(sched)[0], no_lds)
                got = ds.render(m.cam, accel=accel, counters=True, no_lds=no_lds, **sched)
                assert_same(got, fresh.render(m.cam, accel=accel, counters=True, no_lds=no_lds, **sched), what + " vs fresh", rays=True)
                assert_same(got, ref, what + " vs oracle", rays=True)
    # GRID mode after a host update: the grid is built from the new points
    assert_same(ds.render(m.cam, accel=1, counters=True), m.oracle("B", accel=1), "accel 1 vs oracle", rays=True)
    assert_same(ds.render(m.cam, accel=1, counters=True), fresh.render(m.cam, accel=1, counters=True), "accel 1 vs fresh", rays=True)
    ds.close(); fresh.close()


def test_grid_built_before_an_update_is_rebuilt(tmp_path):
    m = mixed(tmp_path)
    ds = m.fresh("A")
    assert_same(ds.render(m.cam, accel=1), m.oracle("A", accel=1), "GRID frame of A")
    m.preconditions(m.oracle("A", accel=1), m.oracle("B", accel=1))
    ds.update(m.data["B"], lights6=m.lights["B"])
    for sched in SCHEDULES:
        assert_same(ds.render(m.cam, accel=1, **sched), m.oracle("B", accel=1), "GRID frame of B")
    ds.close()


# ---- 2. several workgroups of leaves, direct triangle runs

def test_lattice_scene_from_hbm(tmp_path):
    m = lattice(tmp_path)
    ds, fresh = m.fresh("A"), m.fresh("B")
    fa = ds.render(m.cam, max_depth=2, tile=True)
    assert_same(fa, m.oracle("A", depth=2), "before the update")
    m.preconditions(fa, m.oracle("B", depth=2))
    before = ds.stats()
    assert 2 * before["n_nodes"] > 2 * 256, "the refit (one thread per child slot, 256 per workgroup) must span several workgroups"
    ds.update(m.data["B"])
    for sched in SCHEDULES:
        for private in (False, True):
            what = "%s private %d" % (list(sched)[0], private)
            got = ds.render(m.cam, max_depth=3, private_walk=private, **sched)
            assert_same(got, fresh.render(m.cam, max_depth=3, private_walk=private, **sched), what)
    assert_same(ds.render(m.cam, max_depth=2, tile=True), m.oracle("B", depth=2), "vs oracle")
    after = ds.stats()
    assert after["sah_cost"] == before["sah_cost"] and after["device_bytes"] > before["device_bytes"]
    ds.close(); fresh.close()


# ---- 3. the quantisation grid grows

def test_quantisation_grid_grows_and_shrinks_again(tmp_path):
    base = lattice(tmp_path)
    lo, hi, _ = M.bounds(base.ptype, base.data["A"])
    z0, z1 = lo[:, 2].min(), hi[:, 2].max()
    far = str(tmp_path / "lattice_far.p3f")
    tenth = set(range(0, len(base.ptype), 10))

    def move(kind, k, v):                     # every tenth primitive towards the camera: 3.2 x the old extent above the old box
        if kind in ("l", "pl") or k not in tenth:
            return None
        pts = v[:3].reshape(1, 3).copy() if kind == "s" else v.reshape(3, 3).copy()
        zmin = pts[:, 2].min() - (abs(v[3]) if kind == "s" else 0.0)
        pts[:, :2] -= 0.9 * pts[:, :2].mean(0)                  # gathered in front of the camera, sizes kept
        pts[:, 2] += 3.2 * (z1 - z0) + (z1 - zmin)
        return np.concatenate([pts.ravel(), v[3:]]) if kind == "s" else pts.ravel()
    M.rewrite_p3f(base.path["A"], far, move)
    m = Moving(base.path["A"], far)
    assert set(m.moved) == tenth
    lo_b, hi_b, _ = M.bounds(m.ptype, m.data["B"])
    assert lo_b[m.moved, 2].min() >= z1 + 3 * (z1 - z0), "the moved primitives must leave the old box by 3 x its extent"
    ds, fresh_a, fresh_b = m.fresh("A"), m.fresh("A"), m.fresh("B")
    fa = ds.render(m.cam, max_depth=2)
    m.preconditions(fa, m.oracle("B", depth=2))
    ds.update(m.data["B"])
    for sched in SCHEDULES:
        assert_same(ds.render(m.cam, max_depth=2, **sched), fresh_b.render(m.cam, max_depth=2, **sched), "grown %s" % list(sched)[0])
    assert_same(ds.render(m.cam, max_depth=2), m.oracle("B", depth=2), "grown vs oracle")
    ds.update(m.data["A"])
    for sched in SCHEDULES:
        assert_same(ds.render(m.cam, max_depth=2, **sched), fresh_a.render(m.cam, max_depth=2, **sched), "back %s" % list(sched)[0])
    ds.close(); fresh_a.close(); fresh_b.close()


# ---- 4. balls_high: direct sphere runs

def test_balls_high_every_second_sphere_shifted(tmp_path):
    a, b = scene_path("balls_high"), str(tmp_path / "balls_high_b.p3f")
    count = [0]

    def move(kind, k, v):
        if kind != "s":
            return None
        count[0] += 1
        if count[0] % 2:
            return None
        out = v.copy()
        out[count[0] // 2 % 3] += (2.2 * abs(v[3]) + 0.05) * (1 if count[0] % 4 else -1)
        return out
    M.rewrite_p3f(a, b, move)
    m = Moving(a, b, res=(128, 96))
    assert (m.ptype == 0).sum() == 7381 and len(m.moved) == 7381 // 2
    ds, fresh = m.fresh("A"), m.fresh("B")
    fa = ds.render(m.cam, max_depth=3, tile=True)
    m.preconditions(fa, fresh.render(m.cam, max_depth=3, tile=True))
    ds.update(m.data["B"])
    for sched in (dict(tile=True), dict(tree=True)):
        assert_same(ds.render(m.cam, max_depth=3, **sched), fresh.render(m.cam, max_depth=3, **sched), "balls_high %s" % list(sched)[0])
    ds.close(); fresh.close()


# ---- 5. partial update

def test_partial_update_in_scrambled_order(tmp_path):
    full = mixed(tmp_path)
    part = str(tmp_path / "mixed_part.p3f")
    lo, hi, bounded = M.bounds(full.ptype, full.data["A"])
    five = np.flatnonzero(bounded)[np.argsort(-(hi - lo).prod(-1)[bounded])[:5]]          # the five largest: they show
    keep = set(int(i) for i in five)
    M.rewrite_p3f(full.path["A"], part, lambda kind, k, v: M.shift_out_of_own_box(kind, v) if kind != "l" and k in keep else None)
    m = Moving(full.path["A"], part)
    assert set(int(i) for i in m.moved) == keep
    m.preconditions(m.oracle("A"), m.oracle("B"))
    ds, fresh = m.fresh("A"), m.fresh("B")
    fa = ds.render(m.cam)
    order = np.array(sorted(keep))[[3, 0, 4, 2, 1]]
    ds.update(m.data["B"][order], indices=order)
    for kw in (dict(), dict(no_lds=True, tile=True)):
        got = ds.render(m.cam, **kw)
        assert_same(got, fresh.render(m.cam, **kw), "partial update")
        assert (bits(got["rgb32f"]) != bits(fa["rgb32f"])).any()
    assert_same(ds.render(m.cam), m.oracle("B"), "partial update vs oracle")
    ds.close(); fresh.close()


# ---- 6. device-memory update

@pytest.mark.parametrize("make", [mixed, lattice])
def test_device_memory_update_equals_host_memory_update(tmp_path, make):
    m = make(tmp_path)
    dev, host = m.fresh("A"), m.fresh("A")
    fa = dev.render(m.cam, max_depth=2)
    m.preconditions(fa, m.oracle("B", depth=2))
    host.update(m.data["B"], lights6=m.lights["B"])
    dev.update(None, lights6=m.lights["B"])
    data = np.ascontiguousarray(m.data["B"][::-1], np.float32)
    index = np.arange(len(data), dtype=np.uint32)[::-1].copy()
    held = []

    def device_array(arr):
        ptr = C.c_void_p()
        assert P.lib().p3d_device_alloc(dev.h, arr.nbytes, C.byref(ptr)) == 0
        assert P.lib().p3d_upload(dev.h, ptr, arr.ctypes.data, arr.nbytes) == 0
        held.append(ptr)
        return ptr.value
    d_data, d_index = device_array(data), device_array(index)
    dev.update_device(len(data), d_data, d_index)
    for kw in (dict(), dict(accel=0, tree=True), dict(no_lds=True, tile=True)):
        assert_same(dev.render(m.cam, max_depth=2, **kw), host.render(m.cam, max_depth=2, **kw), "device vs host update")
    assert_same(dev.render(m.cam, max_depth=2), m.oracle("B", depth=2), "device update vs oracle")
    # the host does not have the points the grid is made of
    prm = dev._params(2, api.ACCEL_GRID, 0, None, 0, 1, 16, False)
    f32 = np.zeros((m.res[1], m.res[0], 3), np.float32)
    out = api.Outputs(None, f32.ctypes.data, None, 0)
    assert P.lib().p3d_render(dev.h, C.byref(m.cam), C.byref(prm), C.byref(out)) == ERR_STATE
    assert_same(dev.render(m.cam, max_depth=2), host.render(m.cam, max_depth=2), "after the refused GRID frame")
    dev.update(m.data["B"])
    assert_same(dev.render(m.cam, max_depth=2, accel=1), m.oracle("B", accel=1, depth=2), "GRID after the host update")
    # device memory without indices
    dev.update_device(len(data), device_array(np.ascontiguousarray(m.data["A"], np.float32)))
    host.update(m.data["A"])
    assert_same(dev.render(m.cam, max_depth=2), host.render(m.cam, max_depth=2), "device update without indices")
    # an index out of range: skipped on the device, reported, and the tree is consistent
    index[0] = len(data)
    u = api.PrimUpdate(len(data), device_array(index), d_data, 1, None)
    assert P.lib().p3d_scene_update(dev.h, C.byref(u)) == ERR_ARG
    skipped = m.data["B"].copy()
    skipped[len(data) - 1] = m.data["A"][len(data) - 1]
    host.update(skipped)
    assert_same(dev.render(m.cam, max_depth=2), host.render(m.cam, max_depth=2), "after a skipped index")
    for ptr in held:
        assert P.lib().p3d_device_free(dev.h, ptr) == 0
    dev.close(); host.close()


# ---- 7. lights only

def test_lights_only_with_soft_shadows(tmp_path):
    base = mixed(tmp_path)
    lit = str(tmp_path / "mixed_lit.p3f")
    M.rewrite_p3f(base.path["A"], lit, lambda kind, k, v: v + np.array([2.0, -1.5, 0.5, 0, 0, 0]) * (1 + k) if kind == "l" else None)
    m = Moving(base.path["A"], lit)
    assert len(m.moved) == 0 and (bits(m.lights["A"]) != bits(m.lights["B"])).any(-1).all() and len(m.lights["A"]) == 2
    M.assert_frames_differ(m.oracle("A", soft_shadow=True)["rgb32f"], m.oracle("B", soft_shadow=True)["rgb32f"])
    ds = m.fresh("A")
    assert_same(ds.render(m.cam, soft_shadow=True), m.oracle("A", soft_shadow=True), "soft shadows before")
    ds.update(None, lights6=m.lights["B"])
    assert_same(ds.render(m.cam, soft_shadow=True), m.oracle("B", soft_shadow=True), "soft shadows after")
    assert_same(ds.render(m.cam), m.oracle("B"), "point lights after")
    ds.close()


# ---- 8. degenerate trees

DEGENERATE = {
    # one sphere: one node pair with one absent child
    "one_sphere": (["f 0.8 0.4 0.3 0.7 1 1 1 0.3 40 0 1", "s -1.3 0.2 0.4 1.2"], lambda kind, k, v: v + np.array([2.6, 0, 0, 0])),
    # planes only: a root whose children are both absent
    "planes_only": (["f 0.4 0.7 0.5 0.8 1 1 1 0.2 30 0 1", "pl 10 10 -0.5 -10 10 -0.5 -10 -10 -0.5"],
                    lambda kind, k, v: np.array([10, 10, 0.4, -10, 10, 0.9, -10, -10, 0.1])),
}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_trees(tmp_path, name):
    a, b = str(tmp_path / "deg_a.p3f"), str(tmp_path / "deg_b.p3f")
    prims, moved_to = DEGENERATE[name]
    head = ["accel 2", "spp 0", "bclr 0.1 0.3 0.6", "v", "from 4.0 3.0 2.5", "at 0 0 0.3", "up 0 0 1", "angle 50", "hither 0.01",
            "resolution 96 64", "aperture 0", "focal 1", "l 2 5 6 0.9 0.9 0.8"]
    open(a, "w").write("\n".join(head + prims) + "\n")

    def move(kind, k, v):
        return None if kind == "l" else moved_to(kind, k, v)
    M.rewrite_p3f(a, b, move)
    m = Moving(a, b)
    M.assert_frames_differ(m.oracle("A")["rgb32f"], m.oracle("B")["rgb32f"])
    if name == "one_sphere":
        M.assert_boxes_disjoint(m.ptype, m.data["A"], m.data["B"], m.moved)
    ds = m.fresh("A")
    fa = ds.render(m.cam)
    ds.update(np.zeros((0, 12), np.float32))                       # n = 0 changes nothing
    assert_same(ds.render(m.cam), fa, "n = 0")
    ds.update(m.data["B"])
    for kw in (dict(), dict(no_lds=True), dict(accel=0, tree=True), dict(accel=1)):
        assert_same(ds.render(m.cam, **kw), m.oracle("B", accel=kw.get("accel", 2)), "degenerate %s" % (kw,))
    ds.close()


# ---- 9. other entries and state

def test_render_frames_and_trace_rays_after_an_update(tmp_path):
    m = lattice(tmp_path)
    ds, fresh = m.fresh("A"), m.fresh("B")
    fa = ds.render(m.cam, max_depth=2)
    m.preconditions(fa, fresh.render(m.cam, max_depth=2))
    ds.update(m.data["B"])
    cams = m.host["A"].orbit_cameras(3, 11.0)
    got, ref = ds.render_frames(cams, max_depth=3), fresh.render_frames(cams, max_depth=3)
    assert_same(got, ref, "p3d_render_frames")
    osc = O.Scene(m.path["B"])
    rays = OVR.scene_rays(osc, np.random.default_rng(9), 200)
    o, d = np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays])
    got, ref = ds.trace_rays(o, d), fresh.trace_rays(o, d)
    for k in api.RAY_PLANES:
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), "p3d_trace_rays: %s differs" % k
    assert (got["hit_id"] >= 0).sum() >= 20
    ds.close(); fresh.close()


def test_schedule_pick_survives_and_device_bytes_settle(tmp_path):
    m = lattice(tmp_path)
    ds = m.fresh("A")
    for _ in range(16):                              # the measuring frames of this configuration: three schedules x shared /
        fa = ds.render(m.cam, max_depth=3)           # private walks, two frames each (csrc/p3d_frame_config.h: SchedulePick)
    settled = {ds.render(m.cam, max_depth=3) is None or ds.last_schedule() for _ in range(3)}
    assert len(settled) == 1, "the choice must have settled before the update: %s" % (settled,)
    m.preconditions(fa, m.oracle("B", depth=3))
    picked = ds.last_schedule()
    ds.update(m.data["B"])
    assert ds.last_schedule() == picked
    seen = set()
    for _ in range(4):
        fb = ds.render(m.cam, max_depth=3)
        seen.add(ds.last_schedule())
    assert seen == {picked}, "a frame after an update must not measure again: %s after %s" % (seen, picked)
    assert_same(fb, m.oracle("B", depth=3), "after the update")
    first = ds.stats()["device_bytes"]
    for i in range(20):
        ds.update(m.data["A" if i % 2 == 0 else "B"])
        assert ds.stats()["device_bytes"] == first
    assert_same(ds.render(m.cam, max_depth=3), fb, "after 20 more updates")
    ds.close()


# ---- 10. refusals

def test_refusals(tmp_path):
    m = mixed(tmp_path)
    m.preconditions(m.oracle("A"), m.oracle("B"))
    ds = m.fresh("A")
    fa = ds.render(m.cam)
    n = len(m.ptype)
    data = np.ascontiguousarray(m.data["B"], np.float32)
    index = np.arange(n, dtype=np.uint32)
    index[n // 2] = n                                               # one index past the end: nothing may change
    u = api.PrimUpdate(n, index.ctypes.data, data.ctypes.data, 0, None)
    assert P.lib().p3d_scene_update(ds.h, C.byref(u)) == ERR_ARG
    assert_same(ds.render(m.cam), fa, "after a refused update")
    u = api.PrimUpdate(n, None, data.ctypes.data, 2, None)
    assert P.lib().p3d_scene_update(ds.h, C.byref(u)) == ERR_ARG
    u = api.PrimUpdate(n, None, None, 0, None)
    assert P.lib().p3d_scene_update(ds.h, C.byref(u)) == ERR_ARG
    assert_same(ds.render(m.cam), fa, "after refused updates")
    culled = m.fresh("A", cull_never_hit=True)
    u = api.PrimUpdate(n, None, data.ctypes.data, 0, None)
    assert P.lib().p3d_scene_update(culled.h, C.byref(u)) == ERR_STATE
    assert P.lib().p3d_last_error().decode() != ""
    ds.update(data, lights6=m.lights["B"])
    assert_same(ds.render(m.cam), m.oracle("B"), "the handle still updates")
    ds.close(); culled.close()


# ---- a device-built tree, and a deep one

def test_refit_of_a_device_built_chain(tmp_path):
    """The geometric-series scene (tests/lbvh_scenes.py): built on the device (builder=1) its tree is a chain some 38 levels
    deep.  Every second sphere moves out of its own box; the refitted handle renders what a handle freshly built on the
    device from the moved scene renders (a different tree), and what the oracle renders.  Both trees are first checked
    against the reference of test_gpu_lbvh.py, max_depth exactly: the launches below size their stacks from it."""
    import lbvh_scenes as LS
    import test_gpu_lbvh as LB
    assert LB._PROBE["failed"] == 0, "a probe test of this run failed: nothing is rendered through such a tree"
    a, b = LS.write_lbvh_scene(str(tmp_path / "chain_a.p3f"), "geometric"), str(tmp_path / "chain_b.p3f")
    M.rewrite_p3f(a, b, lambda kind, k, v: M.shift_out_of_own_box(kind, v) if kind == "s" and k % 2 == 1 else None)
    m = Moving(a, b)
    assert len(m.moved) == LS.N_SPHERES // 2
    m.preconditions(m.oracle("A", depth=3), m.oracle("B", depth=3))
    depth = {k: LB.check_case(*api.host_build_prims(m.host[k].desc())) for k in "AB"}
    assert depth["A"] >= 30
    ds, fresh = m.fresh("A", builder=1), m.fresh("B", builder=1)
    for h, k in ((ds, "A"), (fresh, "B")):                           # the device builder's trees
        assert h.stats()["max_depth"] == depth[k] and h.stats()["n_nodes"] == LS.N_SPHERES // 2 - 1
    assert_same(ds.render(m.cam, max_depth=3, accel=2, counters=True), m.oracle("A", depth=3), "before the update", rays=True)
    ds.update(m.data["B"])
    ref = m.oracle("B", depth=3)
    for sched in SCHEDULES:
        for no_lds in (False, True):
            what = "%s no_lds %d" % (list(sched)[0], no_lds)
            got = ds.render(m.cam, max_depth=3, accel=2, counters=True, no_lds=no_lds, **sched)
            assert_same(got, fresh.render(m.cam, max_depth=3, accel=2, counters=True, no_lds=no_lds, **sched), what + " vs fresh", rays=True)
            assert_same(got, ref, what + " vs oracle", rays=True)
    ds.close(); fresh.close()
