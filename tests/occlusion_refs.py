"""References for the p3d_occluded tests (not a test module): the segments the reference's object code already answered
-- tests/golden/ref_vectors.npz `accel/<scene>/hits` for test_oracle_vs_ref.scene_rays(sc, default_rng(7), n): column 2 is
BVH::Traverse(Ray&), column 3 Grid::Traverse(Ray&) -- and brute forces over the oracle's intersectors, computed once per
process and never modified afterwards."""
import ctypes as C
import os

import numpy as np

from conftest import GOLDEN
from extra_scenes import scene_path
from oracle import oracle_py as O
import test_oracle_vs_ref as OVR

N_RAYS = dict(OVR.ACCEL_CASES)
_cache = {}


def segments(name, n=None, seed=7):
    """(oracle scene, origins [n, 3], dirs [n, 3]) of scene_rays(sc, default_rng(seed), n); n = the fixture's count."""
    n = N_RAYS[name] if n is None else n
    k = ("seg", name, n, seed)
    if k not in _cache:
        osc = O.Scene(scene_path(name))
        rays = OVR.scene_rays(osc, np.random.default_rng(seed), n)
        o, d = np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays])
        o.setflags(write=False); d.setflags(write=False)
        _cache[k] = (osc, o, d)
    return _cache[k]


def ref_columns(name):
    """(BVH::Traverse(Ray&), Grid::Traverse(Ray&)) of the reference's object code on segments(name): uint8 [n] each."""
    k = ("ref", name)
    if k not in _cache:
        hits = np.load(os.path.join(GOLDEN, "ref_vectors.npz"))["accel/%s/hits" % name]
        assert hits.shape == (N_RAYS[name], 6)
        cols = hits[:, 2].astype(np.uint8), hits[:, 3].astype(np.uint8)
        for c in cols:
            c.setflags(write=False)
        _cache[k] = cols
    return _cache[k]


def length(d):
    """|L| as Vector::length() forms it: float products summed left to right, float square root."""
    d = np.ascontiguousarray(d, np.float32)
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], dtype=np.float32)


def brute_force(ptype, prim12, o, d, bounded):
    """Any-hit over every primitive through the oracle's intersectors (oracle_py.intersect's function, called with
    prepared pointers).  bounded: direction O.normalize(d), accepted with t < |d| (BVH::Traverse(Ray&)); else the direction
    as given and no bound (processLight()'s loop of accel NONE)."""
    fp = C.POINTER(C.c_float)
    fn = O.lib().p3o_intersect
    prim = np.zeros((len(ptype), 12), np.float32)
    prim[:, :prim12.shape[1]] = prim12
    pp = [prim[j].ctypes.data_as(fp) for j in range(len(ptype))]
    kinds = [int(t) for t in ptype]
    t, nrm = np.zeros(1, np.float32), np.zeros(3, np.float32)
    pt, pn = t.ctypes.data_as(fp), nrm.ctypes.data_as(fp)
    lens = length(d)
    out = np.zeros(len(o), np.uint8)
    for i in range(len(o)):
        oi = np.ascontiguousarray(o[i], np.float32)
        di = O.normalize(d[i]) if bounded else np.ascontiguousarray(d[i], np.float32)
        po, pd = oi.ctypes.data_as(fp), di.ctypes.data_as(fp)
        for j in range(len(kinds)):
            if fn(kinds[j], pp[j], po, pd, pt, pn) and (not bounded or t[0] < lens[i]):
                out[i] = 1
                break
    return out


def brute_scene(name, bounded, n=None):
    """brute_force on segments(name, n), cached."""
    k = ("brute", name, bounded, n)
    if k not in _cache:
        osc, o, d = segments(name, n)
        ptype, prim, _ = osc.prims()
        r = brute_force(ptype, prim, o, d, bounded)
        r.setflags(write=False)
        _cache[k] = r
    return _cache[k]
