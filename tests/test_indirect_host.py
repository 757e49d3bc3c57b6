"""p3d_indirect_diffuse without a GPU: the host restatement of steps 8 and 9 (p3dh_indirect_resolve) against the NumPy
restatement (tests/indirect_reference.py), bit for bit, on radiances built to tell a balanced tree from a serial sum; every
combination of optional planes; pixels without a query; the interface; and the whole definition composed on the CPU --
p3dh_ao_segments at radius 1, the oracle's rayTracing() at MAX_DEPTH 1, the resolve -- on a view that is not trivial."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ao_reference as AO                                  # noqa: E402
import indirect_reference as R                             # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P            # noqa: E402
from extra_scenes import scene_path                        # noqa: E402
from oracle import oracle_py as O                          # noqa: E402
from test_ao_host import oracle_planes                     # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api        # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BIAS, SEED = 0.001, 77


def same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def radiances(samples, n=96):
    """(n, samples, 3) radiances: colours in [0, 1] like the clamped direct lighting, then rows of denormals, of +0 and -0,
    of terms of mixed magnitude whose rounding depends on the order of the sum, and of values above 1."""
    rng = np.random.default_rng(samples)
    r = rng.random((n, samples, 3), dtype=F)
    r[1] = (rng.integers(1, 1 << 20, (samples, 3)).astype(np.uint32)).view(F)                 # denormals
    r[2] = F(0.0)
    r[3] = F(-0.0)
    r[4] = np.where(rng.random((samples, 3)) < 0.5, F(0.0), F(-0.0))
    r[5] = F(1.0); r[5, 1:] = F(2.0 ** -24)                                                     # 1 + many half-ulps
    r[6] = (rng.random((samples, 3), dtype=F) * F(2.0) ** rng.integers(-30, 4, (samples, 3)).astype(F)).astype(F)
    r[7] = rng.random((samples, 3), dtype=F) * F(1.0e30)
    r[8, :, 0] = F(2.0 ** -149)
    return r


@pytest.mark.parametrize("colour", [False, True], ids=["no_colour", "colour"])
@pytest.mark.parametrize("albedo", [False, True], ids=["no_albedo", "albedo"])
@pytest.mark.parametrize("samples", [1, 2, 4, 8, 16, 32, 64])
def test_resolve_equals_the_numpy_restatement(samples, albedo, colour):
    r = radiances(samples)
    n = r.shape[0]
    rng = np.random.default_rng(1000 + samples)
    valid = np.ones(n, np.uint8)
    valid[10::7] = 0                                            # pixels without a query, their radiances left in place
    a = (rng.random((n, 3), dtype=F) * F(1.5)) if albedo else None
    c = (rng.random((n, 3), dtype=F) * F(2.0) - F(0.5)) if colour else None
    if colour:
        c[10] = F(-0.0)                                         # an invalid pixel returns c itself, the sign of a zero included
    if samples >= 4:                                            # the inputs must tell the tree from a left-to-right sum
        differs = (R.tree_sum(r).view(np.uint32) != R.serial_sum(r).view(np.uint32)).any(axis=-1)
        assert differs[valid.astype(bool)].sum() >= 5, "no radiance row separates the balanced tree from a serial sum"
        assert (r[1].view(np.uint32) < 0x00800000).all() and np.signbit(r[3]).all()
    got, ref = api.host_indirect_resolve(r, valid, a, c), R.resolve(r, valid, a, c)
    same_bits(got["indirect"], ref["indirect"], "indirect")
    same_bits(got["rgb32f"], ref["rgb32f"], "rgb32f")
    q = valid.astype(bool)
    assert not got["indirect"][~q].any() and not np.signbit(got["indirect"][~q]).any(), "no query: indirect = +0"
    if colour:
        same_bits(got["rgb32f"][~q], c[~q], "no query: rgb32f = c")
    else:
        assert not got["rgb32f"][~q].any()
    if not albedo and not colour:
        same_bits(got["rgb32f"], got["indirect"], "without albedo and colour rgb32f is the indirect light")
    if samples == 1:
        same_bits(got["indirect"][q], r[q, 0], "one sample is its own mean")


def test_the_mean_of_equal_samples_is_the_sample():
    r = np.broadcast_to(np.random.default_rng(3).random((50, 1, 3), dtype=F), (50, 64, 3)).copy()
    got = api.host_indirect_resolve(r, np.ones(50, np.uint8))
    same_bits(got["indirect"], np.ascontiguousarray(r[:, 0]), "64 equal terms: every partial sum is exact")


def test_leading_dimensions_are_kept():
    r = radiances(8, 24).reshape(2, 3, 4, 8, 3)
    valid = np.ones((2, 3, 4), np.uint8)
    valid[1, 2, 3] = 0
    got, ref = api.host_indirect_resolve(r, valid), R.resolve(r, valid)
    assert got["indirect"].shape == (2, 3, 4, 3)
    same_bits(got["indirect"], ref["indirect"], "indirect")
    same_bits(got["rgb32f"], ref["rgb32f"], "rgb32f")


# ---- the interface
def test_the_symbols_are_exported_declared_and_listed():
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    for name in ("p3d_indirect_diffuse", "p3dh_indirect_resolve", "p3dh_ao_segments"):
        assert re.search(r"\bT %s$" % name, dyn, re.M), "libp3d_hip.so does not export " + name
        assert hasattr(P.lib(), name)
    header = open(os.path.join(REPO, "include", "p3d_hip.h")).read()
    assert re.search(r"\bint p3d_indirect_diffuse\(p3d_scene\* scene, const p3d_camera\* cams, int32_t n, const p3d_render_params\* params,\s*"
                     r"const p3d_indirect_params\* indirect, const p3d_indirect_inputs\* in, const p3d_indirect_outputs\* out\);", header)
    for name in ("p3d_indirect_params", "p3d_indirect_inputs", "p3d_indirect_outputs"):
        assert "} %s;" % name in header
    assert "p3d_indirect_diffuse" in api.C_ABI_SYMBOLS
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4\b", header) and P.lib().p3d_abi_version() == 4
    assert C.sizeof(api.IndirectParams) == 12 and api.IndirectParams.seed.offset == 8
    assert C.sizeof(api.IndirectInputs) == 40 and api.IndirectInputs.memory.offset == 32
    assert C.sizeof(api.IndirectOutputs) == 24 and api.IndirectOutputs.memory.offset == 16
    for name in ("indirect_diffuse", "indirect_diffuse_device"):
        assert hasattr(P.DeviceScene, name)
    assert hasattr(P, "host_indirect_resolve") and hasattr(api, "host_indirect_resolve")
    assert api.INDIRECT_SAMPLES == 8 and api.INDIRECT_BIAS == 0.001


def test_a_null_scene_is_refused():
    L = P.lib()
    cam, depth, normal = oracle_planes("balls_box", (24, 16))
    out = np.zeros(depth.shape + (3,), F)
    prm = api.RenderParams()
    prm.accel = 2
    g = api.IndirectParams(8, BIAS, 0)
    i = api.IndirectInputs(depth.ctypes.data, normal.ctypes.data, None, None, 0)
    o = api.IndirectOutputs(out.ctypes.data, None, 0)
    assert L.p3d_indirect_diffuse(None, C.byref(cam), 1, C.byref(prm), C.byref(g), C.byref(i), C.byref(o)) == -1
    assert L.p3d_last_error() and not out.any()


# ---- the definition composed on the CPU
def test_the_cpu_composition_is_finite_and_not_trivial():
    """balls_box at 16 x 12, S = 8, the scene's own camera: host rays at radius 1, the oracle's rayTracing() at MAX_DEPTH 1
    (accel 2), the host resolve.  The non-triviality conditions of the GPU test, on the reference's answers alone."""
    S = 8
    cam, depth, normal = oracle_planes("balls_box", (16, 12))
    o, d, v = api.host_ao_segments(cam, depth, normal, samples=S, radius=1.0, bias=BIAS, seed=SEED)
    ro, rd, rv = R.rays(cam, depth, normal, S, BIAS, SEED)
    same_bits(o, ro, "origin"); same_bits(d, rd, "direction")
    assert np.array_equal(v, rv)
    q = v.astype(bool)
    ln = np.sqrt((d[q].astype(np.float64) ** 2).sum(-1))
    assert np.abs(ln - 1.0).max() < 1e-6, "the rays are unit length"
    osc = O.Scene(scene_path("balls_box"))
    rad = R.radiance_from(R.oracle_radiance(osc, 2), [(o, d, v)], S)[0]
    rng = np.random.default_rng(5)
    albedo, colour = rng.random((12, 16, 3), dtype=F), rng.random((12, 16, 3), dtype=F)
    got, ref = api.host_indirect_resolve(rad, v, albedo, colour), R.resolve(rad, v, albedo, colour)
    same_bits(got["indirect"], ref["indirect"], "indirect"); same_bits(got["rgb32f"], ref["rgb32f"], "rgb32f")
    assert np.isfinite(got["indirect"]).all() and np.isfinite(got["rgb32f"]).all()
    assert (got["indirect"] >= 0).all() and (got["indirect"] <= 1).all(), "a mean of clamped colours"
    hit, shadowed = R.census(osc, O.lib(), o[q].reshape(-1, 3), d[q].reshape(-1, 3))
    print("balls_box 16x12 S=8: %d pixels with a query, %.1f%% of their samples hit, %d shadowed" % (int(q.sum()), 100.0 * hit.mean(), int(shadowed.sum())))
    assert q.any() and (~q).any()
    assert hit.mean() >= 0.1 and (~hit).mean() >= 0.1, "at least 10 % of the samples hit and at least 10 % miss"
    assert shadowed.any(), "a shadow query of a hit sample must answer occluded"
    bg = osc.bg()
    flat = rad[q].reshape(-1, 3)
    same_bits(np.ascontiguousarray(flat[~hit]), np.broadcast_to(bg, flat[~hit].shape).copy(), "a miss returns the background")
    assert len(np.unique(got["indirect"][q].view(np.uint32), axis=0)) > 1, "indirect is not constant over the frame"
