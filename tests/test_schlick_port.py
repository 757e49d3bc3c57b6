"""P3D_FEATURE_SCHLICK on the CPU: the device's pow restatement (csrc/p3d_pow.h) compiled FOR THE HOST against the host's
libm, the shading's KR expression against the reference's own line compiled with g++, and the Schlick fixture against
the reference's object code.

The header is plain C++ apart from the wave-level branch, so g++ -mfma -ffp-contract=off runs exactly the expressions the
GPU runs.  Bit-equal to pow() here means the tables, the fused multiply-adds and the special cases are those of this
image's glibc (2.35, __pow_fma); tests/test_gpu_schlick.py then shows the GPU evaluates them to the same bits.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO, scene_path

CS = os.path.join(REPO, "u_4a_2s_p3d_raytracer_template2_amd", "csrc")
SCHLICK_NPZ = os.path.join(GOLDEN, "schlick_frames.npz")
IORS = (1.0, 1.35, 1.6)            # the refraction indices of the glass materials of the seven scene files

SRC = r"""
#define P3D_POW_HOST_CHECK
#include "p3d_pow.h"
#include <cmath>
#include <string.h>

static bool same(double a, double b) { uint64_t x, y; memcpy(&x, &a, 8); memcpy(&y, &b, 8); return x == y || (a != a && b != b); }
static bool samef(float a, float b) { uint32_t x, y; memcpy(&x, &a, 4); memcpy(&y, &b, 4); return x == y || (a != a && b != b); }

// RT/main.cpp:700-701 as written there (float operands, std::pow on doubles)
static float reference_kr(float ior_1, float newIor, float cos_theta_i) {
    float rI = std::pow((ior_1 - newIor) / (ior_1 + newIor), 2);
    float KR = rI + (1 - rI) * std::pow(1 - cos_theta_i, 5);
    return KR;
}

// every base 1 - c that a float c in [0, 2] can give: k 2^-24 (k <= 2^24) and -k 2^-23 (k <= 2^23); i < n_domain()
static long n_domain() { return (1l << 24) + 1 + (1l << 23); }
static double domain_x(long i) { return i <= (1l << 24) ? std::ldexp((double)i, -24) : -std::ldexp((double)(i - (1l << 24)), -23); }

extern "C" {
void pow_both(const double* x, const double* y, long n, double* port, double* libm) {
    for (long i = 0; i < n; ++i) { port[i] = p3d::p3d_pow(x[i], y[i]); libm[i] = std::pow(x[i], y[i]); }
}
// the base domain with y = 5: how many differ, and the first that does
long pow_domain(double* first_bad) {
    long bad = 0;
    for (long i = 0; i < n_domain(); ++i) {
        const double x = domain_x(i);
        if (!same(p3d::p3d_pow(x, 5.0), std::pow(x, 5.0)) && bad++ == 0) *first_bad = x;
    }
    return bad;
}
// the port's KR against the reference's line for c = 1 - x over the base domain (c is exact: 1 - c gives x back)
long kr_domain(float ior_1, float newIor, float* first_bad) {
    long bad = 0;
    for (long i = 0; i < n_domain(); ++i) {
        const float c = (float)(1.0 - domain_x(i));
        if (!samef(p3d::p3d_schlick_kr(ior_1, newIor, c, p3d::PowTab()), reference_kr(ior_1, newIor, c)) && bad++ == 0) *first_bad = c;
    }
    return bad;
}
void kr_reference(const float* a, const float* b, const float* c, long n, float* out) {
    for (long i = 0; i < n; ++i) out[i] = reference_kr(a[i], b[i], c[i]);
}
void kr_cos_domain(float* out) { for (long i = 0; i < n_domain(); ++i) out[i] = (float)(1.0 - domain_x(i)); }
long kr_domain_size() { return n_domain(); }
}
"""


def pow_cases(rng, n):
    """(tag, x, y) argument sets beyond the shading domain: random doubles with y = 5, then every special case."""
    bits = lambda k: rng.integers(0, 2 ** 63, k, dtype=np.uint64).view(np.float64) * np.where(rng.random(k) < .5, 1.0, -1.0)
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, 0.5, -0.5,
                   2.0, -2.0, 3.0, -3.0, 5.0, -5.0, 2.5, -2.5, 1e300, -1e300, 1.7976931348623157e308, 0.9999999999999999,
                   1.0000000000000002, 2.0 ** 63, -(2.0 ** 63), 2.0 ** 53 + 2, 2.0 ** 53 + 1, 1e-20, -1e-20, 1e20, 0.1, 7.0, -7.0], np.float64)
    X, Y = np.meshgrid(sp, sp)
    snan = np.array([0x7ff0000000000001, 0xfff0000000000001, 0x7ff4000000000000], np.uint64).view(np.float64)
    one = np.ones(3)
    return [
        ("random bit patterns, y = 5", bits(n // 2), np.full(n // 2, 5.0)),
        ("random x in [-1.5, 1.5], y = 5", rng.random(n // 2) * 3 - 1.5, np.full(n // 2, 5.0)),
        ("random bit patterns, random y", bits(n // 10), bits(n // 10)),
        ("negative x, integer and half-integer y", -rng.random(n // 10) * 4, rng.integers(-60, 60, n // 10) * np.where(rng.random(n // 10) < .5, 1.0, 0.5)),
        ("special values, all pairs", X.ravel(), Y.ravel()),
        ("signalling NaNs", np.concatenate([snan, one]), np.concatenate([np.zeros(3), snan])),
        ("2^y across the overflow and subnormal thresholds", np.full(n // 10, 2.0), rng.random(n // 10) * 80 - 40 + np.where(rng.random(n // 10) < .5, 1024, -1074)),
        ("x near 1 with huge y", 1 + (rng.random(n // 20) - 0.5) * 1e-12, rng.random(n // 20) * 1e15),
        ("tiny and huge |y|", rng.random(n // 20) * 4, (2.0 ** rng.integers(-80, 80, n // 20)) * np.where(rng.random(n // 20) < .5, 1.0, -1.0)),
        ("subnormal x", rng.random(n // 20) * 1e-308, rng.random(n // 20) * 4),
    ]


def differing(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))     # NaN payloads are not compared


@pytest.fixture(scope="module")
def pow_host(tmp_path_factory):
    if "fma" not in open("/proc/cpuinfo").read():
        pytest.skip("host without FMA: glibc selects a different pow variant")
    d = tmp_path_factory.mktemp("pow")
    src = d / "h.cpp"
    src.write_text(SRC)
    so = d / "h.so"
    import subprocess
    subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CS, str(src), "-o", str(so), "-lm"])
    L = C.CDLL(str(so))
    L.pow_both.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    L.pow_domain.restype = C.c_long
    L.pow_domain.argtypes = [C.POINTER(C.c_double)]
    L.kr_domain.restype = C.c_long
    L.kr_domain.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float)]
    L.kr_reference.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    L.kr_cos_domain.argtypes = [C.c_void_p]
    L.kr_domain_size.restype = C.c_long
    return L


def cos_domain(L):
    """c = 1 - x for every base x of the shading's pow(1 - cos_theta_i, 5) (2^24 + 2^23 + 1 floats in [0, 2])."""
    c = np.zeros(L.kr_domain_size(), np.float32)
    L.kr_cos_domain(c.ctypes.data)
    return c


def test_pow_restatement_is_libm_on_every_base_the_shading_can_pass(pow_host):
    first = C.c_double(0.0)
    bad = pow_host.pow_domain(C.byref(first))
    assert bad == 0, "%d bases differ from libm's pow(x, 5), first x = %r" % (bad, first.value)


def test_pow_restatement_is_libm_bit_for_bit_on_random_and_special_arguments(pow_host):
    rng = np.random.default_rng(2026)
    total = 0
    for tag, x, y in pow_cases(rng, 10_000_000):
        x = np.ascontiguousarray(x, np.float64); y = np.ascontiguousarray(y, np.float64)
        port = np.zeros_like(x); libm = np.zeros_like(x)
        pow_host.pow_both(x.ctypes.data, y.ctypes.data, len(x), port.ctypes.data, libm.ctypes.data)
        bad = differing(port, libm)
        assert not bad.any(), "%s: %d differ, first: x=%r y=%r port=%r libm=%r" % (
            tag, int(bad.sum()), x[bad][0], y[bad][0], port[bad][0], libm[bad][0])
        total += len(x)
    assert total > 12_000_000


@pytest.mark.parametrize("ior_1", IORS)
@pytest.mark.parametrize("new_ior", IORS)
def test_schlick_kr_is_the_reference_expression(pow_host, ior_1, new_ior):
    first = C.c_float(0.0)
    bad = pow_host.kr_domain(ior_1, new_ior, C.byref(first))
    assert bad == 0, "ior %g -> %g: %d values of cos_theta_i give another KR, first %r" % (ior_1, new_ior, bad, first.value)


def _fixture():
    if not os.path.exists(SCHLICK_NPZ):
        pytest.fail("tests/golden/schlick_frames.npz missing")
    z = np.load(SCHLICK_NPZ)
    names = sorted({k.split("/")[0] for k in z.files})
    return z, {n: json.loads(str(z[n + "/meta"])) for n in names}


def test_schlick_fixture_shows_the_reflections_the_default_hides():
    """SCHLICK_APPROX changes what the glass of mount_low shows: at least 1 000 rgb8 pixels differ from the default frame
    of the same case (rendered here by the oracle restatement, which has no Schlick branch), and the ray count does not
    change (the reference traces the reflection ray of a glass hit whatever KR is)."""
    from oracle import oracle_py as O
    z, cases = _fixture()
    name = "ml_320x180_d4_bvh"
    m = cases[name]
    sc = O.Scene(scene_path(m["scene"]))
    sc.set_resolution(*m["res"])
    off = sc.render(max_depth=m["max_depth"], accel=m["accel"])
    n8 = int((off["rgb8"] != z[name + "/rgb8"]).any(axis=-1).sum())
    assert n8 >= 1000, n8
    assert np.array_equal(off["hit_id"], z[name + "/hit_id"])
    assert off["counters"]["rays"] == int(z[name + "/rays"])


def test_schlick_fixture_is_the_reference_object_code():
    """Where oracle/_ref exists: one strip of every fixture case re-rendered by the reference with its SCHLICK_APPROX
    global set, equal in every bit; the global reads false again afterwards."""
    from oracle import ref_py as R
    if not R.available():
        pytest.skip("oracle/_ref not built (needs the reference tree at build time)")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_schlick_golden", os.path.join(GOLDEN, "make_schlick_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    z, cases = _fixture()
    assert set(cases) == set(G.CASES)
    for name, m in sorted(cases.items()):
        H = m["res"][1]
        y0, y1 = (0, 8) if m["spp"] else (H // 2, H // 2 + 8)     # sampled frames draw a serial stream: from row 0
        r = G.render_ref(m, y0, y1)
        for k in ("rgb8", "rgb32f", "hit_id"):
            a, b = r[k][y0:y1], z[name + "/" + k][y0:y1]
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s: %s differs in rows %d-%d" % (name, k, y0, y1)
        assert not C.c_bool.in_dll(R.lib(m["max_depth"]), "SCHLICK_APPROX").value
