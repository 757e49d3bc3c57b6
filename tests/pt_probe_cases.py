"""Inputs of the path tracer's device probes (p3d_pt_debug_hit_world / _scatter / _direct_lighting), shared by
tests/test_pt_probe_inputs.py (CPU: the cases are not trivial) and tests/test_gpu_pathtracer_probes.py (GPU: the kernel's
hit_world, scatter and direct_lighting against oracle/pt_oracle.cpp).  Seeded numpy only; every ray is one a frame can
produce: directions normalised in float32 or `unit + rough * v` (|v| <= 1, rough one of the scene's own fuzzy metals),
origins within 40 units of the scene.  Case i runs in lane i % 64 of workgroup i / 64, so every group is padded to whole
waves and the mixed-wave groups lay their lanes out on purpose."""
import functools

import numpy as np

from oracle import oracle_py as O

F = np.float32
LIGHTS = np.array([[-10.0, 15.0, 0.0], [8.0, 15.0, 3.0], [1.0, 15.0, -9.0]], F)
BIG = np.array([[-4.0, 1.0, 0.0], [4.0, 1.0, 0.0], [0.0, 1.0, 0.0]], F)          # diffuse, metal, glass (+ its -0.5 bubble)
MT_DIFFUSE, MT_METAL, MT_GLASS = 0, 1, 2
BRANCHES = ["diffuse", "metal", "reflect", "refract", "tir"]
MARGIN_CAP = 1e-5          # a scatter / lighting case this close to a branch decision is left out of the comparison ...
LEFT_OUT_CAP = 0.01        # ... and at most this share of any material's cases may be


def unit(v):
    v = np.asarray(v, F)
    return (v / np.sqrt((v * v).sum(axis=-1, keepdims=True, dtype=F), dtype=F)).astype(F)


def _sphere_dirs(rng, n):
    v = rng.normal(size=(n, 3)).astype(F)
    return unit(v)


def _in_ball(rng, n):
    return (_sphere_dirs(rng, n) * (rng.random((n, 1)) ** (1.0 / 3.0)).astype(F)).astype(F)


class Cases:
    def __init__(self):
        self.o, self.d, self.time, self.tmin, self.tmax, self.seed, self.active, self.group = [], [], [], [], [], [], [], []
        self.names = []

    def add(self, rng, name, o, d, time=None, tmin=0.001, tmax=10000.0, active=None, pad=True):
        o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
        n = len(o)
        time = rng.random(n).astype(F) if time is None else np.broadcast_to(np.asarray(time, F), (n,)).copy()
        seed = (rng.random(n) * 5.0).astype(F)                 # gSeed = pixel hash in [0, 1] + iTime
        tmin = np.broadcast_to(np.asarray(tmin, F), (n,)).copy()
        tmax = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
        active = np.ones(n, np.int32) if active is None else np.asarray(active, np.int32)
        cols = [o, d, time, tmin, tmax, seed, active]
        if pad and n % 64:                                      # whole waves: the tail repeats the group's first cases
            idx = np.arange(n + 64 - n % 64) % n
            cols = [c[idx] for c in cols]
        gid = len(self.names)
        self.names.append(name)
        for lst, c in zip((self.o, self.d, self.time, self.tmin, self.tmax, self.seed, self.active), cols):
            lst.append(c)
        self.group.append(np.full(len(cols[0]), gid, np.int32))
        return gid

    def done(self):
        out = {k: np.concatenate(getattr(self, k)) for k in ("o", "d", "time", "tmin", "tmax", "seed", "active", "group")}
        out["names"] = list(self.names)
        assert len(out["seed"]) % 64 == 0
        return out


def _primary(W=64, H=36, eye=(-10.0, 0.0, 8.0)):
    """getRay() of a W x H frame at pixel centres (pinhole), as mainImage() sets the camera up."""
    eye, at, up = np.array(eye, F), np.array([0, 0, -1], F), np.array([0, 1, 0], F)
    w = eye - at
    plane = np.sqrt((w * w).sum(dtype=F), dtype=F)
    height = F(2.0) * plane * F(np.tan(F(60.0) * F(3.14159265358979) / F(180.0) * F(0.5)))
    width = F(W / H) * height
    n = unit(w)
    u = unit(np.cross(up, n).astype(F))
    v = np.cross(n, u).astype(F)
    ys, xs = np.mgrid[0:H, 0:W]
    px = (width * ((xs.ravel().astype(F) + F(0.5)) / F(W) - F(0.5))).astype(F)
    py = (height * ((ys.ravel().astype(F) + F(0.5)) / F(H) - F(0.5))).astype(F)
    d = unit(px[:, None] * u + py[:, None] * v + n * (-plane))
    return np.broadcast_to(eye, d.shape).copy(), d


def _perp(rng, a):
    """unit vectors perpendicular to the rows of a"""
    r = rng.normal(size=a.shape)
    a64 = a.astype(np.float64)
    a64 /= np.linalg.norm(a64, axis=1, keepdims=True)
    r -= (r * a64).sum(axis=1, keepdims=True) * a64
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def _outside(rng, n, lo=12.0, hi=38.0):
    ang = rng.random(n) * 2 * np.pi
    rad = lo + rng.random(n) * (hi - lo)
    return np.stack([rad * np.cos(ang), 0.3 + rng.random(n) * 8.0, rad * np.sin(ang)], axis=1).astype(F)


def _inside_field(rng, n):
    return np.stack([rng.random(n) * 10 - 5, 0.45 + rng.random(n) * 0.5, rng.random(n) * 10 - 5], axis=1).astype(F)


def _fuzzy(rng, u, roughs):
    """unit + rough * v, |v| <= 1: what scatter() hands on from a fuzzy metal (not re-normalised)"""
    r = rng.choice(roughs, len(u)).astype(F)
    return (u + r[:, None] * _in_ball(rng, len(u))).astype(F)


@functools.lru_cache(maxsize=None)
def hit_world_cases(seed=20240611):
    rng = np.random.default_rng(seed)
    centre, cls, rough = O.pt_small_spheres()
    present = np.flatnonzero(cls >= 0)
    roughs = rough[cls == 3]
    C = Cases()

    o, d = _primary()
    C.add(rng, "primary", o, d)
    o2, d2 = _primary(eye=(6.0, 3.0, 8.0))                       # iMouse somewhere else: another eye
    C.add(rng, "primary_mouse", o2[::3], d2[::3])

    # aimed at every small sphere: its centre, and tangent at radius * (1 +- 2^-k), from outside and from inside the field
    for where in ("outside", "inside"):
        oo, dd, tt = [], [], []
        for i in present:
            c = centre[i].astype(np.float64)
            ks = np.arange(8, 21)
            offs = np.concatenate([[0.0], 0.2 * (1 + 2.0 ** -ks), 0.2 * (1 - 2.0 ** -ks)])
            org = (_outside(rng, 1) if where == "outside" else _inside_field(rng, 1))[0].astype(np.float64)
            org = np.broadcast_to(org, (len(offs), 3)).copy()
            # static centre for time 0; moving spheres are met at their lifted centre at any other time, so use both
            axis = c - org
            p = _perp(rng, axis)
            target = c + p * offs[:, None]
            oo.append(org)
            dd.append(unit(target - org))
            tt.append(np.where(np.arange(len(offs)) % 2 == 0, 0.0, rng.random(len(offs))))
        C.add(rng, "tangent_" + where, np.concatenate(oo), np.concatenate(dd), time=np.concatenate(tt))

    # d.y == 0 exactly at the slab edges and the sphere tops; d.x == 0, d.z == 0
    for y in (-0.05, 0.0, 0.39, 0.41, 0.95, 1.0):
        n = 128
        org = np.stack([rng.random(n) * 24 - 12, np.full(n, y), rng.random(n) * 24 - 12], axis=1)
        tgt = np.stack([rng.random(n) * 10 - 5, np.full(n, y), rng.random(n) * 10 - 5], axis=1)
        dd = unit(tgt - org)
        dd[:, 1] = 0.0
        dd = unit(dd)
        assert (dd[:, 1] == 0).all()
        C.add(rng, "dy0_y%g" % y, org, dd)
    for ax in (0, 2):
        n = 256
        org = _outside(rng, n, 6.0, 20.0)
        org[:, ax] = (rng.random(n) * 10 - 5).astype(F)
        tgt = np.stack([rng.random(n) * 10 - 5, rng.random(n) * 0.5, rng.random(n) * 10 - 5], axis=1).astype(F)
        v = tgt - org
        v[:, ax] = 0.0
        C.add(rng, "d%s0" % "xyz"[ax], org, unit(v))

    # rays that start inside spheres: the big glass one, its bubble, small ones
    n = 384
    C.add(rng, "inside_glass", BIG[2] + _sphere_dirs(rng, n) * (0.52 + 0.46 * rng.random((n, 1))).astype(F), _sphere_dirs(rng, n))
    C.add(rng, "inside_bubble", BIG[2] + _in_ball(rng, n) * F(0.49), _sphere_dirs(rng, n))
    C.add(rng, "inside_big_other", BIG[rng.integers(0, 2, n)] + _in_ball(rng, n) * F(0.98), _sphere_dirs(rng, n))
    idx = np.repeat(present, 6)
    C.add(rng, "inside_small", centre[idx] + _in_ball(rng, len(idx)) * F(0.19), _sphere_dirs(rng, len(idx)), time=0.0)

    # long grazing rays across the floor from 30 units out
    n = 1024
    ang = rng.random(n) * 2 * np.pi
    org = np.stack([30 * np.cos(ang), 0.01 + rng.random(n) * 0.6, 30 * np.sin(ang)], axis=1).astype(F)
    tgt = np.stack([rng.random(n) * 12 - 6, rng.random(n) * 0.5 - 0.01, rng.random(n) * 12 - 6], axis=1).astype(F)
    C.add(rng, "grazing_floor", org, unit(tgt - org))

    # along cell boundaries and through the corners x, z in {-5, 4, 4.9}
    oo, dd = [], []
    for k in range(-5, 6):
        for ax in (0, 2):
            for y in (0.1, 0.2, 0.45):
                for eps in (0.0, 1e-6, -1e-6):
                    org = np.array([0.0, y, 0.0])
                    org[ax] = k + eps
                    org[2 - ax] = -9.0
                    v = np.zeros(3)
                    v[2 - ax] = 1.0
                    oo.append(org)
                    dd.append(v)
    corners = [(x, z) for x in (-5.0, 4.0, 4.9) for z in (-5.0, 4.0, 4.9)]
    for (x, z) in corners:
        org = _outside(rng, 40, 6.0, 30.0)
        tgt = np.array([x, 0.2, z], F) + (rng.random((40, 3)) * 0.02 - 0.01).astype(F)
        oo.extend(org)
        dd.extend(unit(tgt - org))
    C.add(rng, "cell_edges_corners", np.array(oo, F), unit(np.array(dd, F)))

    # the near set's two 64-bit words: gx = 1 (cells 60..69) sits across bit 63/64
    n = 1024
    tgt = np.stack([1.0 + rng.random(n) * 0.999, rng.random(n) * 0.4, rng.random(n) * 10 - 5], axis=1).astype(F)
    org = (tgt + np.stack([rng.normal(size=n) * 0.15, 1.5 + rng.random(n) * 6, rng.normal(size=n) * 0.15], axis=1)).astype(F)
    C.add(rng, "straddle_bit63", org, unit(tgt - org))
    cells6 = np.flatnonzero((cls >= 0) & (np.arange(100) >= 60) & (np.arange(100) < 70))
    idx = np.repeat(cells6, 24)
    org = _outside(rng, len(idx), 6.0, 20.0)
    C.add(rng, "aim_gx1", org, unit(centre[idx] + _in_ball(rng, len(idx)) * F(0.15) - org), time=0.0)

    # fuzzy-metal rays (not unit length): from the fuzzy spheres' own surfaces and from further away
    fz = np.flatnonzero(cls == 3)
    idx = np.repeat(fz, 40)
    nrm = _sphere_dirs(rng, len(idx))
    nrm[:, 1] = np.abs(nrm[:, 1])
    org = (centre[idx] + nrm * F(0.201)).astype(F)
    u = unit(nrm + _sphere_dirs(rng, len(idx)) * F(0.9))
    C.add(rng, "fuzzy_from_spheres", org, (u + rough[idx][:, None] * _in_ball(rng, len(idx))).astype(F))
    n = 1024
    org = _outside(rng, n, 6.0, 38.0)
    tgt = centre[rng.choice(present, n)] + _in_ball(rng, n) * F(0.6)
    C.add(rng, "fuzzy_far", org, _fuzzy(rng, unit(tgt - org), roughs))
    # ... and the ones whose |d.d - 1| is small although they are not unit length: from far away past a sphere at a
    # perpendicular distance a unit-length test would call a miss (hit_sphere's t assumes |d| = 1: the sphere it sees
    # has radius^2 + (d.d - 1) q^2 at range q)
    n = 512
    i = rng.choice(present, n)
    org = _outside(rng, n, 8.0, 38.0)
    org[:, 1] = (0.2 + rng.random(n) * 1.4).astype(F)
    c = centre[i].astype(np.float64)
    c[:, 1] += np.where(cls[i] == 0, rng.random(n) * 0.5, 0.0)
    q = np.linalg.norm(c - org, axis=1)
    e = 10.0 ** -(3.0 + rng.random(n) * 2.5) * 0.999                                   # d.d - 1 in (3e-6, 1e-3)
    pmax = np.sqrt(0.04 + e * q * q)
    p = _perp(rng, c - org)
    p[:, 1] = np.abs(p[:, 1])
    u = unit(c + p * (pmax * (0.3 + 0.69 * rng.random(n)))[:, None] - org).astype(np.float64)
    r = rng.choice(roughs[roughs < 0.2], n).astype(np.float64)
    # v along u with u.v = e / (2 r) to first order: |v| <= 1 since e <= 1e-3 << 2 r
    v = u * ((np.sqrt(1.0 + e) - 1.0) / r)[:, None]
    assert (np.linalg.norm(v, axis=1) <= 1.0).all()
    # each alone in its wave (lane w % 64 of wave w, the other lanes inactive): the culling works on the union of a wave's
    # rays, and neighbours that look at the whole field would hide a bound that is too tight for this one
    lone = np.arange(n) * 64 + np.arange(n) % 64
    act = np.zeros(n * 64, np.int32)
    act[lone] = 1
    C.add(rng, "fuzzy_nearly_unit", np.repeat(org, 64, axis=0), np.repeat((u + r[:, None] * v).astype(F), 64, axis=0),
          time=np.repeat(rng.random(n), 64), active=act)

    # ---- mixed waves (lane layout matters: no padding needed, every block is 64 lanes)
    def field_rays(n):
        org = _outside(rng, n, 6.0, 25.0)
        tgt = centre[rng.choice(present, n)] + _in_ball(rng, n) * F(0.3)
        return org, unit(tgt - org)

    def sky_rays(n):
        org = np.stack([rng.random(n) * 10 - 5, 2.0 + rng.random(n) * 3, rng.random(n) * 10 - 5], axis=1).astype(F)
        dd = _sphere_dirs(rng, n)
        dd[:, 1] = np.abs(dd[:, 1]) + F(0.05)
        return org, unit(dd)

    oo, dd = [], []
    for w in range(16):                      # one lane at cell (-5,-5), one at (4,4), the rest miss the slab
        org, dr = sky_rays(64)
        a, b = rng.choice(64, 2, replace=False)
        for lane, (x, z) in ((a, (-5, -5)), (b, (4, 4))):
            tgt = np.array([x + 0.45, 0.2, z + 0.45], F) + (rng.random(3) * 0.3 - 0.15).astype(F)
            org[lane] = tgt + np.array([rng.normal() * 0.05, 1.0 + rng.random() * 4, rng.normal() * 0.05], F)
            dr[lane] = unit(tgt - org[lane])
        oo.append(org)
        dd.append(dr)
    C.add(rng, "wave_two_corners", np.concatenate(oo), np.concatenate(dd))

    masks = {"lane0": [0], "lane63": [63], "lanes31_32": [31, 32], "every_third": list(range(0, 64, 3))}
    for name, lanes in masks.items():
        org, dr = field_rays(64 * 4)
        act = np.zeros(64 * 4, np.int32)
        for w in range(4):
            act[64 * w + np.array(lanes)] = 1
        C.add(rng, "wave_active_" + name, org, dr, active=act)

    # one fuzzy-metal ray (keeps the whole field) alone in its wave, and inside a wave whose other rays see one cell
    org, dr = field_rays(64 * 8)
    act = np.zeros(64 * 8, np.int32)
    for w in range(8):
        lane = 64 * w + int(rng.integers(0, 64))
        act[lane] = 1
        dr[lane] = _fuzzy(rng, dr[lane:lane + 1], roughs[roughs > 0.1])[0]
    C.add(rng, "wave_lone_fuzzy", org, dr, active=act)
    oo, dd = [], []
    for w in range(8):
        i = rng.choice(present)
        tgt = centre[i] + _in_ball(rng, 64) * F(0.15)
        org = (tgt + np.stack([rng.normal(size=64) * 0.05, 1.0 + rng.random(64) * 3, rng.normal(size=64) * 0.05], axis=1)).astype(F)
        dr = unit(tgt - org)
        lane = int(rng.integers(0, 64))
        dr[lane] = _fuzzy(rng, dr[lane:lane + 1], roughs[roughs > 0.1])[0]
        oo.append(org)
        dd.append(dr)
    C.add(rng, "wave_fuzzy_in_narrow_union", np.concatenate(oo), np.concatenate(dd), time=0.0)

    # the same ray in 64 waves, in lane w of wave w, among different neighbours: 64 identical results
    org, dr = field_rays(64 * 64)
    so, sd = _outside(rng, 1, 10.0, 11.0)[0], None
    sd = unit(centre[present[len(present) // 2]] + np.array([0.05, 0.02, -0.03], F) - so)
    gid = C.add(rng, "same_ray_64_waves", org, dr)
    same = np.arange(64) * 64 + np.arange(64)
    C.o[-1][same], C.d[-1][same] = so, sd
    for k in ("time", "tmin", "tmax", "seed"):
        getattr(C, k)[-1][same] = getattr(C, k)[-1][same[0]]
    out = C.done()
    out["same_ray"] = np.flatnonzero(out["group"] == gid)[same]

    # shadow feelers (tmin 0, tmax 1, time 0) from points on every kind of primitive towards the three lights
    ref = O.pt_hit_world(out["o"], out["d"], out["time"], out["tmin"], out["tmax"], out["seed"])
    picks = []
    for prim_sel in [ref["prim"] == k for k in range(6)] + [(ref["prim"] >= 6) & (cls[np.clip(ref["prim"] - 6, 0, 99)] == k) for k in range(5)]:
        picks.append(np.flatnonzero(prim_sel & (ref["hit"] == 1))[:64])
    picks = np.concatenate(picks)
    fo = np.repeat((ref["pos"][picks] + F(0.001) * ref["normal"][picks]).astype(F), 3, axis=0)
    fd = unit(np.tile(LIGHTS, (len(picks), 1)) - np.repeat(ref["pos"][picks], 3, axis=0))
    S = Cases()
    S.add(rng, "shadow_feelers", fo, fd, time=0.0, tmin=0.0, tmax=1.0)
    extra = S.done()
    base = len(out["names"])
    for k in ("o", "d", "time", "tmin", "tmax", "seed", "active"):
        out[k] = np.concatenate([out[k], extra[k]])
    out["group"] = np.concatenate([out["group"], extra["group"] + base])
    out["names"] += extra["names"]
    for k in ("o", "d", "time", "tmin", "tmax", "seed", "active", "group", "same_ray"):
        out[k].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hit_world_reference():
    """oracle hit_world() on every case (the inactive ones too), computed once"""
    c = hit_world_cases()
    ref = O.pt_hit_world(c["o"], c["d"], c["time"], c["tmin"], c["tmax"], c["seed"])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _mat_row(albedo=(0, 0, 0), spec=(0, 0, 0), rough=0.0, ref_idx=0.0, refract=(0, 0, 0)):
    return np.array(list(albedo) + list(spec) + [rough, ref_idx] + list(refract), F)


@functools.lru_cache(maxsize=None)
def record_cases(seed=77):
    """Records for scatter() / direct_lighting(): what the oracle's hit_world() returns on the rays above (the scene's own
    positions, normals and materials, the ray that found them and the RNG state it left) plus hand-made ones per material.
    Returns (ray, rec, seed, light_pos, label) with label = the material kind a cap is counted over."""
    rng = np.random.default_rng(seed)
    c, ref = hit_world_cases(), hit_world_reference()
    _, cls, rough = O.pt_small_spheres()
    sel = np.flatnonzero((ref["hit"] == 1) & (c["tmax"] > 1.0) & (c["active"] == 1))
    ray = {"o": [c["o"][sel]], "d": [c["d"][sel]], "t": [c["time"][sel]]}
    rec = {k: [ref[k][sel]] for k in ("pos", "normal", "t", "mat_type", "mat")}
    sd = [ref["seed_out"][sel]]

    def hand(n, mat_type, mat, cos_kind, flip=False):
        nrm = _sphere_dirs(rng, n)
        tang = _perp(rng, nrm).astype(F)
        if cos_kind == "normal":
            cs = 1.0 - 10.0 ** -(1 + 5 * rng.random(n))
        elif cos_kind == "grazing":
            cs = 10.0 ** -(1 + 2.5 * rng.random(n))
        else:
            cs = rng.random(n)
        sgn = 1.0 if flip else -1.0                      # -1: the ray arrives against the normal (enters)
        dirs = unit((sgn * cs)[:, None] * nrm + np.sqrt(1 - cs * cs)[:, None] * tang)
        pos = np.stack([rng.random(n) * 10 - 5, rng.random(n) * 2, rng.random(n) * 10 - 5], axis=1).astype(F)
        t = (0.5 + rng.random(n) * 20).astype(F)
        ray["o"].append((pos - dirs * t[:, None]).astype(F))
        ray["d"].append(dirs)
        ray["t"].append(rng.random(n).astype(F))
        rec["pos"].append(pos)
        rec["normal"].append(nrm)
        rec["t"].append(t)
        rec["mat_type"].append(np.full(n, mat_type, np.int32))
        rec["mat"].append(np.broadcast_to(mat, (n, 11)).copy() if mat.ndim == 1 else mat)
        sd.append((rng.random(n) * 5).astype(F))

    n = 128
    fuzzy_rows = np.stack([_mat_row(spec=(0.7, 0.8, 0.6), rough=r) for r in rng.choice(rough[cls == 3], n)])
    for kind in ("normal", "grazing", "any"):
        hand(n, MT_DIFFUSE, _mat_row(albedo=(0.4, 0.2, 0.1), rough=1.0, ref_idx=1.0), kind)
        hand(n, MT_METAL, _mat_row(spec=(0.7, 0.6, 0.5)), kind)
        hand(n, MT_METAL, fuzzy_rows, kind)
        for flip in (False, True):                        # glass entered and left (left at a grazing angle: total reflection)
            hand(n, MT_GLASS, _mat_row(albedo=(1, 1, 1), spec=(0.04,) * 3, ref_idx=1.333), kind, flip)
            hand(n, MT_GLASS, _mat_row(albedo=(1, 1, 1), spec=(0.04,) * 3, ref_idx=1.2, refract=(0.3, 0.6, 0.1)), kind, flip)
            hand(n, MT_GLASS, _mat_row(albedo=(1, 1, 1), spec=(0.04,) * 3, rough=0.3, ref_idx=1.333, refract=(0.2, 0.1, 0.4)), kind, flip)
    ray = {k: np.concatenate(v).astype(F) for k, v in ray.items()}
    rec = {k: np.concatenate(v) for k, v in rec.items()}
    sd = np.concatenate(sd).astype(F)
    light = LIGHTS[np.arange(len(sd)) % 3]
    for d_ in (ray, rec):
        for v in d_.values():
            v.setflags(write=False)
    sd.setflags(write=False)
    return ray, rec, sd, light


@functools.lru_cache(maxsize=None)
def scatter_reference():
    ray, rec, sd, _ = record_cases()
    return O.pt_scatter(ray, rec, sd)


@functools.lru_cache(maxsize=None)
def lighting_reference():
    ray, rec, sd, light = record_cases()
    return O.pt_direct_lighting(light, ray, rec, sd)
