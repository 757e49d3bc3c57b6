"""p3d_upsample without a GPU: the host restatement (p3dh_upsample) against the NumPy restatement of the definition
(tests/upsample_reference.py), bit for bit, and the properties a guided upsampler must have."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upsample_reference as R                             # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P            # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api        # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.5                                                # the 4 % depth noise of random_planes() gives fractional weights
SHAPES = [(1, 1), (3, 2), (9, 5), (17, 12)]                # the LOW (res_x, res_y)
F = np.float32


def same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = got.view(np.uint32) != ref.view(np.uint32) if got.dtype == np.float32 else got != ref
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


@pytest.mark.parametrize("npow", [0, 5])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_equals_the_numpy_restatement(shape, s, channels, n, npow):
    planes = R.random_planes(*shape, s=s, n=n, channels=channels, seed=10 * s + channels)
    ref = R.upsample(*planes, sigma_depth=SIGMA, normal_power_log2=npow, info=True)
    if shape[0] * shape[1] > 6:                            # the planes alone, under the reference alone: every class of pixel
        z = planes[3]
        assert np.isinf(z).any() and np.isnan(z).any() and (z == 0).any()
        assert np.isnan(planes[1]).any() and (planes[1] == 0).any()
        assert ref["fractional"].any(), "no pixel with a fractional weight"
        assert (~R.valid(z) & (ref["fallback"] == 0)).any(), "no miss centre made of sky"
        assert (ref["fallback"] == 1).any(), "no fallback pixel"
        assert ref["fallback"].mean() <= 0.25, "fallback pixels are more than a quarter of the frame"
    got = api.host_upsample(*planes, sigma_depth=SIGMA, normal_power_log2=npow)
    assert got["plane"].shape == (n, shape[1] * s, shape[0] * s) + ((3,) if channels == 3 else ())
    same_bits(got["plane"], ref["plane"], "plane")
    same_bits(got["fallback"], ref["fallback"], "fallback")


def three_surfaces(lw, lh, s):
    """Depth 1 left of a vertical edge, depth 5 right of it, a sky band above: the edges at 3.3 and lh - 1.6 low pixels, off the
    low grid.  Colours whose channels are powers of two or zero.  -> the planes and the full-resolution ground truth."""
    colours = np.array([(0.5, 0.0, 2.0), (4.0, 0.25, 0.0), (0.0, 1.0, 0.125)], F)         # near, far, sky

    def region(X, Y):
        X, Y = np.broadcast_arrays(X, Y)
        return np.where(Y > (lh - 1.6) * s, 2, np.where(X < 3.3 * s, 0, 1))

    def planes(reg):
        z = np.array([1.0, 5.0, np.inf], F)[reg]
        nrm = np.zeros(reg.shape + (3,), F)
        nrm[..., 2] = np.where(reg == 2, 0.0, 1.0)
        return z[None], nrm[None], colours[reg][None]

    lz, ln, lo = planes(region(s * (np.arange(lw) + 0.5)[None, :], s * (np.arange(lh) + 0.5)[:, None]))
    z, nr, truth = planes(region((np.arange(lw * s) + 0.5)[None, :], (np.arange(lh * s) + 0.5)[:, None]))
    return (lo, lz, ln, z, nr), truth


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_three_surfaces_come_back_exactly_and_plain_bilinear_mixes_them(s):
    """Every pixel has a tap with b > 0 on its own surface (the tap on its side of each edge), the other surfaces' taps weigh
    nothing (|dZ| / (sigma Z) >= 1.6), and a weighted mean of one colour whose channels are powers of two is that colour:
    scaling by a power of two commutes with rounding, so sum = C * sw exactly."""
    planes, truth = three_surfaces(9, 7, s)
    assert len(np.unique(planes[3])) == 3 and (np.isinf(planes[3]).sum(1) >= s).any()
    for channels in (3, 1):
        p = planes if channels == 3 else (np.ascontiguousarray(planes[0][..., 0]),) + planes[1:]
        t = truth if channels == 3 else np.ascontiguousarray(truth[..., 0])
        for npow in (0, 5):
            got = api.host_upsample(*p, sigma_depth=SIGMA, normal_power_log2=npow)
            same_bits(got["plane"], t, "s=%d c=%d" % (s, channels))
            assert not got["fallback"].any()
    flat = (planes[0], np.ones_like(planes[1]), np.zeros_like(planes[2]) + F((0, 0, 1)), np.ones_like(planes[3]),
            np.zeros_like(planes[4]) + F((0, 0, 1)))
    bilinear = api.host_upsample(*flat, sigma_depth=SIGMA, normal_power_log2=0)
    assert not bilinear["fallback"].any()
    assert np.array_equal(bilinear["plane"], truth) == (s == 1), "plain bilinear mixes across the edges for s >= 2"


@pytest.mark.parametrize("s", [2, 3, 4])
def test_a_column_no_low_centre_samples_falls_back_to_bilinear(s):
    lw, lh = 9, 5
    rng = np.random.default_rng(s)
    low = rng.random((1, lh, lw, 3)).astype(F)
    lz, z = np.ones((1, lh, lw), F), np.ones((1, lh * s, lw * s), F)
    ln, nr = np.zeros((1, lh, lw, 3), F), np.zeros((1, lh * s, lw * s, 3), F)
    ln[..., 2] = nr[..., 2] = 1.0
    xf = 4 * s + s - 1
    z[..., xf] = 0.2                                       # |dZ| / (sigma Z) = 8: no low sample explains the column
    got = api.host_upsample(low, lz, ln, z, nr, sigma_depth=SIGMA, normal_power_log2=5)
    expect = np.zeros((1, lh * s, lw * s), np.uint8)
    expect[..., xf] = 1
    same_bits(got["fallback"], expect, "fallback")
    bilinear = api.host_upsample(low, lz, ln, np.ones_like(z), nr, sigma_depth=SIGMA, normal_power_log2=5)
    assert not bilinear["fallback"].any()
    same_bits(got["plane"], bilinear["plane"], "the column takes the bilinear value (and the rest is bilinear anyway)")


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_a_plane_of_ones_comes_back_as_ones(s):
    _, lz, ln, z, nr = R.random_planes(17, 12, s=s, n=2, channels=1, seed=s)
    got = api.host_upsample(np.ones_like(lz), lz, ln, z, nr, sigma_depth=SIGMA, normal_power_log2=5)
    ok = got["fallback"] == 0
    assert ok.any() and (~ok).any()
    same_bits(got["plane"][ok], np.ones(int(ok.sum()), F), "ones")


def test_frames_of_a_batch_are_independent():
    planes = R.random_planes(9, 5, s=3, n=3, channels=3, seed=8)
    batch = api.host_upsample(*planes, sigma_depth=SIGMA, normal_power_log2=5)
    for f in range(3):
        one = api.host_upsample(*[a[f:f + 1] for a in planes], sigma_depth=SIGMA, normal_power_log2=5)
        same_bits(one["plane"][0], batch["plane"][f], "plane of frame %d" % f)
        same_bits(one["fallback"][0], batch["fallback"][f], "fallback of frame %d" % f)


def test_the_symbols_are_exported_declared_and_listed():
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    for name in ("p3d_upsample", "p3d_debug_upsample", "p3dh_upsample"):
        assert re.search(r"\bT %s$" % name, dyn, re.M), "libp3d_hip.so does not export " + name
        assert hasattr(P.lib(), name)
    header = open(os.path.join(REPO, "include", "p3d_hip.h")).read()
    assert re.search(r"\bint p3d_upsample\(p3d_scene\* scene, const p3d_upsample_params\* params, const p3d_upsample_inputs\* in, "
                     r"const p3d_upsample_outputs\* out\);", header)
    assert re.search(r"\bint p3d_debug_upsample\(int device, const p3d_upsample_params\* params, const p3d_upsample_inputs\* in, "
                     r"const p3d_upsample_outputs\* out\);", header)
    assert "typedef struct p3d_upsample_params {" in header and "} p3d_upsample_inputs;" in header and "} p3d_upsample_outputs;" in header
    assert "p3d_upsample" in api.C_ABI_SYMBOLS and "p3d_debug_upsample" in api.C_ABI_SYMBOLS
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4\b", header) and P.lib().p3d_abi_version() == 4
    # the constants of the definition, in the header's text
    for text in ("t = 2 x + 1 - s", "i0 = floor(t / (2 s))", "r = t - 2 s i0", "fx = (float)r / (float)(2 s)", "bx0 = 1 - fx", "bx1 = fx",
                 "inv_z = 1 / (sigma_depth * Z_p)", "tz = max(0, 1 - |Z_q - Z_p| * inv_z)", "w  = (b * wz) * wn", "fallback = 1",
                 "dy = 0, 1 (outer)"):
        assert text in header, text
    assert C.sizeof(api.UpsampleParams) == 28 and api.UpsampleParams.factor.offset == 8 and api.UpsampleParams.channels.offset == 16
    assert api.UpsampleParams.sigma_depth.offset == 20 and api.UpsampleParams.normal_power_log2.offset == 24
    assert C.sizeof(api.UpsampleInputs) == 48 and api.UpsampleInputs.memory.offset == 40
    assert C.sizeof(api.UpsampleOutputs) == 24 and api.UpsampleOutputs.fallback.offset == 8 and api.UpsampleOutputs.memory.offset == 16
    for name in ("upsample", "upsample_device"):
        assert hasattr(P.DeviceScene, name)
    assert api.UPSAMPLE_SIGMA_DEPTH == api.DENOISE_SIGMA_DEPTH and api.UPSAMPLE_NORMAL_POWER_LOG2 == api.DENOISE_NORMAL_POWER_LOG2


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    """Every refusal of upsample_check_request, through the probe (which checks before it looks for a device); the outputs
    are untouched."""
    L = P.lib()
    lo, lz, ln, z, nr = R.random_planes(3, 2, s=2, n=1, channels=1, seed=7)
    plane = np.full(z.shape, 7.0, F)
    fb = np.full(z.shape, 0xA5, np.uint8)
    good = (3, 2, 2, 1, 1, 0.5, 5)

    def call(params=good, planes=(lo, lz, ln, z, nr), in_memory=0, o="both", out_memory=0, null=None):
        p = api.UpsampleParams(*params) if params is not None else None
        i = api.UpsampleInputs(*[x.ctypes.data if x is not None else None for x in planes], in_memory) if planes is not None else None
        o = {"both": (plane.ctypes.data, fb.ctypes.data), "none": (None, None)}.get(o, o)
        o = api.UpsampleOutputs(o[0], o[1], out_memory)
        return L.p3d_debug_upsample(0, C.byref(p) if p else None, C.byref(i) if i else None, C.byref(o) if null != "out" else None)

    ERR_ARG, ERR_LIMIT = -1, -4
    assert L.p3d_upsample(None, C.byref(api.UpsampleParams(*good)), None, None) == ERR_ARG and b"scene" in L.p3d_last_error()
    assert call(params=None) == ERR_ARG and call(planes=None) == ERR_ARG and call(null="out") == ERR_ARG
    for k in range(5):
        assert call(planes=tuple(None if j == k else x for j, x in enumerate((lo, lz, ln, z, nr)))) == ERR_ARG
    assert call(o="none") == ERR_ARG and b"both NULL" in L.p3d_last_error()
    for factor in (0, 5, -1):
        assert call(params=good[:2] + (factor,) + good[3:]) == ERR_ARG and b"factor" in L.p3d_last_error()
    for channels in (0, 2, 4):
        assert call(params=good[:4] + (channels,) + good[5:]) == ERR_ARG and b"channels" in L.p3d_last_error()
    for bad in ((0, 2), (3, 0), (-3, 2)):
        assert call(params=bad + good[2:]) == ERR_ARG
    assert call(params=good[:3] + (0,) + good[4:]) == ERR_ARG
    for sigma in (0.0, -1.0, np.inf, np.nan):
        assert call(params=good[:5] + (sigma,) + good[6:]) == ERR_ARG and b"sigma_depth" in L.p3d_last_error()
    for npow in (-1, 9):
        assert call(params=good[:6] + (npow,)) == ERR_ARG and b"normal_power_log2" in L.p3d_last_error()
    assert call(in_memory=2) == ERR_ARG and call(in_memory=-1) == ERR_ARG and call(out_memory=2) == ERR_ARG
    assert call(in_memory=1) == ERR_ARG and call(out_memory=1) == ERR_ARG, "the probe takes host planes"
    for k, x in enumerate((lo, lz, ln, z, nr)):               # an output plane that is an input plane
        assert call(o=(x.ctypes.data, fb.ctypes.data)) == ERR_ARG and b"input plane" in L.p3d_last_error(), k
        assert call(o=(plane.ctypes.data, x.ctypes.data)) == ERR_ARG, k
    # 4 * 11586^2 * 4 = 2^31 + ...: W * H alone does not fit; then the frames, then the channels
    assert call(params=(11586, 11586, 4, 1, 1, 0.5, 5)) == ERR_LIMIT and b"31 bits" in L.p3d_last_error()
    assert call(params=(2, 2, 1, 1 << 29, 1, 0.5, 5)) == ERR_LIMIT
    assert call(params=(16384, 16384, 1, 3, 3, 0.5, 5)) == ERR_LIMIT
    assert call(params=(1 << 30, 1, 4, 1, 1, 0.5, 5)) == ERR_LIMIT
    assert (plane == 7.0).all() and (fb == 0xA5).all(), "a refused call wrote an output"
