"""p3d_indirect_paths without a GPU: the host restatement of steps 3 and 4 (p3dh_path_add, p3dh_path_next) against the NumPy
restatement (tests/path_reference.py), bit for bit, on synthetic records; the whole path composed on the CPU through the
oracle's answers, whose one-bounce planes are p3d_indirect_diffuse's reference; the conditions under which the GPU tests
mean something, on the reference side alone; the interface."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ao_reference as AO                                  # noqa: E402
import indirect_reference as R                             # noqa: E402
import path_reference as PR                                # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P            # noqa: E402
from extra_scenes import scene_path                        # noqa: E402
from oracle import oracle_py as O                          # noqa: E402
from test_ao_host import oracle_planes                     # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api        # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
BIAS, SEED = 0.001, 77


def same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = got.view(np.uint32) != ref.view(np.uint32) if got.dtype == np.float32 else got != ref
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def records(m=4096):
    """m synthetic (ray, answer, key, sample, throughput) records over a scene of 5 primitives and 3 materials: misses,
    back-facing normals, zero and NaN normals, s = 0 and 63, T carried from a previous bounce."""
    rng = np.random.default_rng(11)
    o = (rng.random((m, 3), dtype=F) * F(4.0) - F(2.0)).astype(F)
    d = AO.normalized((rng.random((m, 3), dtype=F) * F(2.0) - F(1.0)).astype(F))
    t = (rng.random(m, dtype=F) * F(6.0)).astype(F)
    n = AO.normalized((rng.random((m, 3), dtype=F) * F(2.0) - F(1.0)).astype(F))
    n[5::16] = F(0.0)                                           # zero normals
    n[7::16, 1] = F(np.nan)                                     # NaN normals
    n[9::16] *= F(3.0)                                          # not unit length
    hit_id = rng.integers(0, 5, m).astype(np.int32)
    hit_id[3::8] = -1                                           # misses
    t[3::8] = F(np.inf)
    prim_material = np.array([2, 0, 1, 1, 0], np.uint32)
    materials12 = rng.random((3, 12), dtype=F)
    materials12[1, 0:3] = [F(0.0), F(1.5), F(2.0 ** -130)]      # an albedo with a zero, a value above 1 and a denormal
    pk0 = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(U)
    s = rng.integers(0, 64, m).astype(U)
    s[0::4] = 0
    s[1::4] = 63
    T = (rng.random((m, 3), dtype=F) * F(1.2)).astype(F)
    r = (rng.random((m, 3), dtype=F)).astype(F)
    total = (rng.random((m, 3), dtype=F) * F(3.0)).astype(F)
    return o, d, t, n, hit_id, prim_material, materials12, pk0, s, T, r, total


def test_next_and_add_equal_the_numpy_restatement():
    o, d, t, n, hit_id, pm, mats, pk0, s, T, r, total = records()
    away = ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]) > 0
    hit = hit_id >= 0
    assert (hit & away).sum() > 500 and (hit & ~away).sum() > 500, "back-facing and front-facing normals"
    assert (~hit).sum() > 400 and (hit & ~n.any(axis=1)).sum() > 100 and (hit & np.isnan(n).any(axis=1)).sum() > 100
    assert (hit & (s == 0)).sum() > 500 and (hit & (s == 63)).sum() > 500
    outs = {}
    for b in range(0, 7):                                       # the ray just traced is b; the next vertex is b + 1 = 1 .. 7
        got = api.host_path_next(b, BIAS, o, d, t, n, hit_id, pm, mats, pk0, s, T)
        ref = PR.path_next(b, BIAS, o, d, t, n, hit_id, pm, mats, pk0, s, T)
        for g, e, what in zip(got, ref, ("origin", "direction", "throughput", "alive")):
            same_bits(g, e, "b = %d: %s" % (b, what))
        o2, d2, T2, alive = got
        assert np.array_equal(alive.astype(bool), hit)
        assert not o2[~hit].any() and not d2[~hit].any()
        same_bits(np.ascontiguousarray(T2[~hit]), np.ascontiguousarray(T[~hit]), "a path that ended keeps its throughput")
        a = mats[pm[np.where(hit, hit_id, 0)], 0:3]
        if b == 0:
            same_bits(np.ascontiguousarray(T2[hit]), np.ascontiguousarray(a[hit]), "T_1 is the albedo")
        else:
            same_bits(np.ascontiguousarray(T2[hit]), np.ascontiguousarray((T * a).astype(F)[hit]), "T carried from the bounce before")
        ok = hit & np.isfinite(n).all(axis=1) & n.any(axis=1)
        ln = np.sqrt((d2[ok].astype(np.float64) ** 2).sum(-1))
        assert np.abs(ln - 1.0).max() < 1e-6, "the next rays are unit length"
        outs[b] = d2
    assert (outs[0].view(np.uint32) != outs[1].view(np.uint32)).any(axis=1)[ok].mean() > 0.99, "the bounce keys the direction"
    # D_3 from its key alone: rng_mix(rng_mix(pk_0, 0x80000000 + 3), s)
    fin = hit & np.isfinite(n).all(axis=1)
    again = PR.cosine_direction(np.where(away[:, None], -n, n).astype(F), AO.rng_mix(pk0, U(0x80000003)), s)
    same_bits(np.ascontiguousarray(again[fin]), np.ascontiguousarray(outs[2][fin]), "D_3 from its key")
    alive = (np.arange(len(o)) % 5 != 0).astype(np.uint8)
    for b in (0, 1, 4):
        got, ref = api.host_path_add(b, T, r, alive, total), PR.path_add(b, T, r, alive, total)
        same_bits(got, ref, "add b = %d" % b)
        q = alive.astype(bool)
        same_bits(np.ascontiguousarray(got[~q]), np.ascontiguousarray(total[~q]), "an ended path keeps its sum")
        if b == 0:
            same_bits(np.ascontiguousarray(got[q]), np.ascontiguousarray(r[q]), "R = r_0")
        else:
            fused = (total.astype(np.float64) + T.astype(np.float64) * r.astype(np.float64)).astype(F)
            assert (got[q].view(np.uint32) != fused[q].view(np.uint32)).any(), "the inputs tell a product and a sum from a fused multiply-add"


def _oracle_paths(name, res, S, B, accel, use_host=False):
    cam, depth, normal = oracle_planes(name, res)
    osc = O.Scene(scene_path(name))
    _, _, pm = osc.prims()
    kw = dict(next_fn=api.host_path_next, add_fn=api.host_path_add) if use_host else {}
    return cam, depth, normal, osc, PR.paths(PR.oracle_answer(osc, O.lib(), accel), [cam], dict(depth=depth[None], normal=normal[None]), S, B, BIAS,
                                             SEED, (pm.astype(np.uint32), osc.materials()), **kw)


def test_the_whole_path_on_the_cpu():
    """balls_box at 12 x 8, S = 4, B = 3 through the oracle answer, once with the NumPy steps and once with the host layer's;
    the planes of B = 1 are indirect_reference's for the same rays."""
    cam, depth, normal, osc, ref = _oracle_paths("balls_box", (12, 8), 4, 3, 2)
    _, _, _, _, host = _oracle_paths("balls_box", (12, 8), 4, 3, 2, use_host=True)
    for k in ("indirect", "rgb32f", "R"):
        same_bits(host[k], ref[k], "host layer against NumPy: " + k)
    assert np.isfinite(ref["indirect"]).all() and ref["valid"].any() and ref["traced"][2] > 0
    _, _, _, _, one = _oracle_paths("balls_box", (12, 8), 4, 1, 2)
    o, d, v = R.rays(cam, depth, normal, 4, BIAS, SEED)
    rad = R.radiance_from(R.oracle_radiance(osc, 2), [(o, d, v)], 4)
    single = R.resolve(rad, v[None])
    same_bits(one["indirect"], single["indirect"], "B = 1 is p3d_indirect_diffuse: indirect")
    same_bits(one["rgb32f"], single["rgb32f"], "B = 1 is p3d_indirect_diffuse: rgb32f")
    q = v.astype(bool)
    assert (ref["R"][0][q] >= one["R"][0][q]).all(), "further bounces only add light"


def test_balls_box_is_not_trivial():
    """The conditions of the issue on the reference side alone: balls_box at 24 x 16, S = 8, B = 3, accel 2, bias 0.001,
    seed 77, the scene's own camera, the oracle's answers."""
    _, _, _, _, three = _oracle_paths("balls_box", (24, 16), 8, 3, 2)
    _, _, _, _, one = _oracle_paths("balls_box", (24, 16), 8, 1, 2)
    q = three["valid"].astype(bool)
    n = int(q.sum()) * 8
    traced, missed, nonzero = three["traced"], three["missed"], three["nonzero"]
    print("balls_box 24x16 S=8 B=3: %d valid pixels, %d paths; traced per bounce %s (%.1f%% / %.1f%% / %.1f%%), missed per bounce %s, "
          "non-zero terms per bounce %s" % (int(q.sum()), n, traced.tolist(), 100.0 * traced[0] / n, 100.0 * traced[1] / n, 100.0 * traced[2] / n,
                                            missed.tolist(), nonzero.tolist()))
    differ = (three["indirect"].view(np.uint32) != one["indirect"].view(np.uint32)).any(axis=-1)
    print("indirect at B = 3 differs from B = 1 on %d of %d valid pixels" % (int(differ[q].sum()), int(q.sum())))
    assert traced[0] == n and q.any() and (~q).any()
    assert traced[2] >= 0.05 * n, "at least 5 % of the samples of valid pixels trace a ray at bounce 2"
    assert missed[0] + missed[1] >= 0.05 * n, "at least 5 % end on a miss at bounce 0 or 1"
    assert nonzero[1] + nonzero[2] > 0, "some T_b * r_b with b >= 1 is not zero"
    assert differ[q].sum() >= 0.25 * q.sum(), "indirect at B = 3 differs from B = 1 on at least a quarter of the valid pixels"
    assert not differ[~q].any()


def test_the_symbols_are_exported_declared_and_listed():
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    for name in ("p3d_indirect_paths", "p3dh_path_next", "p3dh_path_add"):
        assert re.search(r"\bT %s$" % name, dyn, re.M), "libp3d_hip.so does not export " + name
        assert hasattr(P.lib(), name)
    header = open(os.path.join(REPO, "include", "p3d_hip.h")).read()
    assert re.search(r"\bint p3d_indirect_paths\(p3d_scene\* scene, const p3d_camera\* cams, int32_t n, const p3d_render_params\* params,\s*"
                     r"const p3d_path_params\* paths, const p3d_indirect_inputs\* in, const p3d_indirect_outputs\* out\);", header)
    assert "} p3d_path_params;" in header
    assert "p3d_indirect_paths" in api.C_ABI_SYMBOLS
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4\b", header) and P.lib().p3d_abi_version() == 4
    assert C.sizeof(api.PathParams) == 16 and api.PathParams.bounces.offset == 4 and api.PathParams.seed.offset == 12
    for name in ("indirect_paths", "indirect_paths_device"):
        assert hasattr(P.DeviceScene, name)
    for name in ("host_path_next", "host_path_add"):
        assert hasattr(P, name) and hasattr(api, name)


def test_a_null_scene_is_refused():
    L = P.lib()
    cam, depth, normal = oracle_planes("balls_box", (24, 16))
    out = np.zeros(depth.shape + (3,), F)
    prm = api.RenderParams()
    prm.accel = 2
    g = api.PathParams(8, 3, BIAS, 0)
    i = api.IndirectInputs(depth.ctypes.data, normal.ctypes.data, None, None, 0)
    o = api.IndirectOutputs(out.ctypes.data, None, 0)
    assert L.p3d_indirect_paths(None, C.byref(cam), 1, C.byref(prm), C.byref(g), C.byref(i), C.byref(o)) == -1
    assert L.p3d_last_error() and not out.any()
