"""GPU tests of the path tracer below the frame level: the frame kernel's own hit_world(), scatter() and
direct_lighting() (p3d_pt_debug_*) against oracle/pt_oracle.cpp on the cases of tests/pt_probe_cases.py, the chunked
linear sums of p3d_pt_render (the form bench.py times) against the sum of single frames, and the rgba recurrence.

hit_world is + - * / sqrt, integer hashing and int-to-float conversion on both sides, compiled without contraction and
with correctly rounded divide and sqrt: it is compared BIT FOR BIT.  Only scatter() and direct_lighting() call libm; their
libm-touched outputs are held to 4 x e_ref, e_ref being the float oracle's own distance from its double evaluation."""
import numpy as np
import pytest

from oracle import oracle_py as O
import u_4a_2s_p3d_raytracer_template2_amd as P
import pt_probe_cases as K

pytestmark = pytest.mark.gpu

U = np.uint32


def bits_equal(a, b):
    return np.ascontiguousarray(a).view(U) == np.ascontiguousarray(b).view(U)


def same_bits_or_nan(a, b):
    return bits_equal(a, b) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def device_hit_world():
    c = K.hit_world_cases()
    n = len(c["seed"])
    rng = np.random.default_rng(3)
    fill = {"hit": np.full(n, -7, np.int32), "t": rng.random(n).astype(np.float32) + 100, "pos": rng.random((n, 3)).astype(np.float32),
            "normal": rng.random((n, 3)).astype(np.float32), "mat_type": np.full(n, 9, np.int32),
            "mat": rng.random((n, 11)).astype(np.float32), "seed_out": rng.random(n).astype(np.float32) - 50}
    got = P.pt_debug_hit_world(c["o"], c["d"], c["time"], c["tmin"], c["tmax"], c["seed"], active=c["active"], fill=fill)
    return fill, got


def _report(c, bad, what):
    g = c["group"][bad]
    return "%s differs on %d cases: %s" % (what, int(bad.sum()), {c["names"][k]: int((g == k).sum()) for k in np.unique(g)})


def test_hit_world_is_bit_equal_to_the_oracle(device_hit_world):
    c, ref = K.hit_world_cases(), K.hit_world_reference()
    _, got = device_hit_world
    act = c["active"] == 1
    for k in ("hit", "t", "seed_out"):
        bad = act & ~bits_equal(got[k], ref[k])
        assert not bad.any(), _report(c, bad, k)
    hit = act & (ref["hit"] == 1)
    for k in ("pos", "normal", "mat"):
        bad = hit & ~bits_equal(got[k], ref[k]).all(axis=1)
        assert not bad.any(), _report(c, bad, k)
    bad = hit & (got["mat_type"] != ref["mat_type"])
    assert not bad.any(), _report(c, bad, "mat_type")
    miss = act & (ref["hit"] == 0)
    assert bits_equal(got["t"][miss], c["tmax"][miss]).all()


def test_hit_world_nearly_unit_fuzzy_rays_keep_every_sphere(device_hit_world):
    """A fuzzy-metal ray is not unit length, and hit_sphere() (which assumes it is) then sees a sphere of
    radius^2 + (d.d - 1) q^2 at range q.  With the culling's geometric path open to |d.d - 1| < 1e-3 that sphere outgrows
    the slab's 0.05 margin from q = 4.7 on; the bound is 4e-6 (pt_kernels.hip), under which it stays inside the margin
    out to q = 75.  Each of these rays is alone in its wave: neighbours that keep the whole field would hide the loss."""
    c, ref = K.hit_world_cases(), K.hit_world_reference()
    _, got = device_hit_world
    m = (c["group"] == c["names"].index("fuzzy_nearly_unit")) & (c["active"] == 1)
    dd = (c["d"][m].astype(np.float64) ** 2).sum(axis=1)
    assert ((np.abs(dd - 1) < 1e-3) & (np.abs(dd - 1) > 4e-6)).sum() >= 400
    assert (ref["hit"][m] == 1).sum() >= 200
    for k in ("hit", "t", "seed_out"):
        bad = ~bits_equal(got[k][m], ref[k][m])
        assert not bad.any(), "%s differs on %d of %d rays" % (k, int(bad.sum()), int(m.sum()))


def test_hit_world_inactive_lanes_keep_their_sentinel(device_hit_world):
    c = K.hit_world_cases()
    fill, got = device_hit_world
    off = c["active"] == 0
    assert off.sum() >= 64
    for k in fill:
        assert bits_equal(got[k][off], fill[k][off]).all(), k


def test_hit_world_same_ray_in_64_waves_gives_64_identical_results(device_hit_world):
    c = K.hit_world_cases()
    _, got = device_hit_world
    s = c["same_ray"]
    assert got["hit"][s[0]] == 1
    for k in got:
        assert bits_equal(got[k][s], np.broadcast_to(got[k][s[0]], got[k][s].shape)).all(), k


def _held(name, out, dev, flt, hp, sel):
    """device within 4 x e_ref of the double evaluation, e_ref = the float oracle's own distance from it"""
    if not sel.any():
        return
    e_ref = float(np.abs(flt[sel].astype(np.float64) - hp[sel]).max())
    e_dev = float(np.abs(dev[sel].astype(np.float64) - hp[sel]).max())
    print("%-10s %-6s cases %5d  e_ref %.3e  device %.3e" % (name, out, int(sel.sum()), e_ref, e_dev))
    assert e_dev <= 4.0 * e_ref, (name, out, e_ref, e_dev)


def test_scatter_against_the_oracle():
    """seed_out, out.o, out.t, a metal's attenuation and everything at rough == 0 bit for bit; the rest within 4 x e_ref.
    Measured on an MI355X (e_ref = float oracle against its double variant, device = kernel against the double variant,
    largest component over the cases; attenuations not listed have e_ref = device = 0):
    branch / material   output  e_ref      device
    diffuse             atten   9.761e-07  9.761e-07
    diffuse             d       9.973e-06  9.973e-06
    metal (fuzzy)       d       2.307e-07  2.307e-07
    reflect             d       1.886e-07  1.886e-07
    refract             atten   4.481e-08  4.608e-08
    refract             d       5.868e-07  5.868e-07
    total reflection    d       1.362e-07  1.362e-07
    """
    ray, rec, sd, _ = K.record_cases()
    ref = K.scatter_reference()
    got = P.pt_debug_scatter(ray, rec, sd)
    ok = ref["margin"] >= K.MARGIN_CAP
    assert bits_equal(got["seed_out"][ok], ref["seed_out"][ok]).all()
    # no libm call reaches these: the scattered ray's origin and time; a metal's attenuation; everything when rough == 0
    assert bits_equal(got["o"][ok], ref["o"][ok]).all()
    assert bits_equal(got["t"][ok], ref["t"][ok]).all()
    br, rough = ref["branch"], rec["mat"][:, 6]
    metal = ok & (br == 1)
    assert bits_equal(got["atten"][metal], ref["atten"][metal]).all()
    smooth = ok & (rough == 0) & ((br == 1) | (br == 2) | (br == 4))
    assert smooth.sum() >= 100
    for k in ("atten", "d"):
        assert bits_equal(got[k][smooth], ref[k][smooth]).all(), k
    for b, name in enumerate(K.BRANCHES):
        sel = ok & (br == b)
        _held(name, "atten", got["atten"], ref["atten"], ref["hp_atten"], sel)
        _held(name, "d", got["d"], ref["d"], ref["hp_d"], sel)


def test_direct_lighting_against_the_oracle():
    """seed_out bit for bit, unlit results exactly zero, lit colours within 4 x e_ref.  Measured on an MI355X (e_ref, device):
    diffuse 1.460e-06, 1.460e-06; metal 0, 0 (a metal's albedo is black: its highlight is zero); glass 3.009e-08, 3.009e-08."""
    ray, rec, sd, light = K.record_cases()
    ref = K.lighting_reference()
    got = P.pt_debug_direct_lighting(light, ray, rec, sd)
    ok = ref["margin"] >= K.MARGIN_CAP
    assert bits_equal(got["seed_out"][ok], ref["seed_out"][ok]).all()
    dark = ok & (ref["lit"] < 2)
    assert bits_equal(got["rgb"][dark], np.zeros_like(got["rgb"][dark])).all()
    for mt, name in ((K.MT_DIFFUSE, "diffuse"), (K.MT_METAL, "metal"), (K.MT_GLASS, "glass")):
        _held(name, "rgb", got["rgb"], ref["rgb"], ref["hp_rgb"], ok & (ref["lit"] == 2) & (rec["mat_type"] == mt))


# ---- chunked linear sums (p3d_pt_render with rgba == NULL: pt_capi.cpp)
def chunk_rule(n_frames):
    """pt_capi.cpp: a linear-only request of >= 32 frames is cut into min(32, n / 8) runs of ceil(n / runs) frames"""
    if n_frames < 32:
        return 1, n_frames
    chunks = max(1, min(32, n_frames // 8))
    return chunks, (n_frames + chunks - 1) // chunks


def expected_sum(frames, chunked):
    """float32 sum of the per-frame colours in the kernel's order: left to right within a run (from +0), then the runs left
    to right; an empty run contributes +0."""
    n = len(frames)
    chunks, cf = chunk_rule(n) if chunked else (1, n)
    parts = []
    for c in range(chunks):
        s = np.zeros_like(frames[0])
        for k in range(c * cf, min(c * cf + cf, n)):
            s = s + frames[k]
        parts.append(s)
    if chunks == 1:
        return parts[0]
    total = parts[0]
    for s in parts[1:]:
        total = total + s
    return total


class FrameBank:
    def __init__(self, pt):
        self.pt, self.bank = pt, {}

    def frames(self, W, H, n, first=0, stride=1):
        out = []
        for j in range(n):
            k = first + j * stride
            if (W, H, k) not in self.bank:
                self.bank[(W, H, k)] = self.pt.render(W, H, 1, first_frame=k)[1]
            out.append(self.bank[(W, H, k)])
        return out


def test_chunked_linear_sums_equal_the_sum_of_single_frames():
    import torch
    assert chunk_rule(40) == (5, 8) and chunk_rule(37) == (4, 10) and chunk_rule(97) == (12, 9) and chunk_rule(32) == (4, 8)
    assert 11 * 9 > 97          # the twelfth run of 97 frames starts at frame 99: empty
    pt = P.PathTracer()
    bank = FrameBank(pt)

    def check(W, H, n, first=0, stride=1, device_form=True):
        frames = bank.frames(W, H, n, first, stride)
        assert all(f.dtype == np.float32 for f in frames)
        _, lin = pt.render(W, H, n, first_frame=first, frame_stride=stride, want_rgba=False)
        exp = expected_sum(frames, chunked=True)
        assert same_bits_or_nan(lin, exp).all(), ("linear-only", W, H, n, first, stride, int((~same_bits_or_nan(lin, exp)).sum()))
        rgba, lin2 = pt.render(W, H, n, first_frame=first, frame_stride=stride)
        exp2 = expected_sum(frames, chunked=False)
        assert same_bits_or_nan(lin2, exp2).all(), ("with rgba", W, H, n, first, stride)
        if device_form:
            buf = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            pt.render_device(0, buf.data_ptr(), W, H, n, first_frame=first, frame_stride=stride)
            pt.sync()
            dev = buf.cpu().numpy().reshape(H, W, 3)
            assert same_bits_or_nan(dev, lin).all(), ("device memory", W, H, n)
        return chunk_rule(n)[0] > 1 and not same_bits_or_nan(exp, exp2).all()

    W, H = 50, 18
    order_matters = [check(W, H, n) for n in (40, 37, 97, 32)]
    order_matters.append(check(W, H, 40, first=2, stride=3))
    assert any(order_matters)                   # the run order is visible in the bits: the comparison can tell
    check(160, 90, 32, device_form=False)       # d_partial grows ...
    check(W, H, 40)                             # ... and is reused at the smaller size
    check(W, H, 31)                             # not chunked: the plain sum
    pt.close()


def _recurrence(frames, dtype):
    prev = np.zeros(frames[0].shape, dtype)
    w = dtype(0)
    for c in frames:
        prev_lin = np.power(prev, dtype(2.2))
        w = w + dtype(1)
        t = dtype(1) / w
        col = prev_lin * (dtype(1) - t) + c.astype(dtype) * t
        prev = np.power(col, dtype(1) / dtype(2.2))
    return prev


def test_rgba_follows_the_shader_recurrence():
    """toLinear / mix / toGamma over the device's own per-frame colours, N = 24 at 50x18, within 4 x the distance of
    the same recurrence in numpy float32 from float64.  Measured on an MI355X: e_ref 5.130e-07, device 2.878e-07."""
    W, H, N = 50, 18, 24
    pt = P.PathTracer()
    frames = FrameBank(pt).frames(W, H, N)
    rgba, _ = pt.render(W, H, N)
    pt.close()
    ok = np.all([np.isfinite(f).all(axis=2) & (f >= 0).all(axis=2) for f in frames], axis=0)
    assert ok.mean() > 0.99
    assert np.array_equal(rgba[..., 3], np.full((H, W), N, np.float32))
    with np.errstate(invalid="ignore"):
        r64, r32 = _recurrence(frames, np.float64), _recurrence(frames, np.float32)
    e_ref = float(np.abs(r32[ok].astype(np.float64) - r64[ok]).max())
    e_dev = float(np.abs(rgba[..., :3][ok].astype(np.float64) - r64[ok]).max())
    print("rgba recurrence: e_ref %.3e  device %.3e" % (e_ref, e_dev))
    assert e_dev <= 4.0 * e_ref
