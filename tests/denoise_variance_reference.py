"""The filter of p3d_denoise_variance in NumPy, written from its definition (include/p3d_hip.h, DESIGN "Variance-guided
denoising") and from nothing else: float32 throughout, one operation per expression node, the taps in the defined order.
The host restatement (p3dh_denoise_variance) is compared with it bit for bit, and the device with the host restatement."""
import numpy as np

from denoise_reference import F, K1, _lum, _max0, _tap, clamp01, u8fromfloat, valid_depth

K2 = (F(0.5), F(0.25))
EPS = F(2.0 ** -20)


def prefiltered_variance(v, z):
    """g of the definition over one frame: the 3 x 3 Gaussian of v over the valid in-frame neighbours, at stride 1."""
    valid = valid_depth(z)
    sg = np.zeros_like(v)
    sk = np.zeros_like(v)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                use = valid_depth(_tap(z, dx, dy, F(0)))
                k = K2[abs(dx)] * K2[abs(dy)]
                sg = np.where(use, sg + k * _tap(v, dx, dy, F(0)), sg)
                sk = np.where(use, sk + k, sk)
        g = sg / np.where(valid, sk, F(1))
    assert g.dtype == F
    return np.where(g > 0, g, F(0)).astype(F)


def denoise_variance_pass(c, v, z, n, a, i, sigma_depth, sigma_albedo, sigma_color, normal_power_log2):
    """Pass i over one frame: c, n, a (H, W, 3), v, z (H, W) float32 -> the colour and the variance after the pass."""
    s = 1 << i
    valid = valid_depth(z)
    with np.errstate(all="ignore"):
        inv_a = F(1) / F(sigma_albedo)
        g = prefiltered_variance(v, z)
        inv_c = F(1) / (F(sigma_color) * np.sqrt(g) + EPS)
        inv_z = F(1) / (F(sigma_depth) * z)
        lp = _lum(c)
        acc = np.zeros_like(c)
        sw = np.zeros_like(z)
        sv = np.zeros_like(z)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                zq = _tap(z, dx * s, dy * s, F(0))
                nq, aq, cq = _tap(n, dx * s, dy * s, F(0)), _tap(a, dx * s, dy * s, F(0)), _tap(c, dx * s, dy * s, F(0))
                vq = _tap(v, dx * s, dy * s, F(0))
                use = valid & valid_depth(zq)
                h = K1[abs(dx)] * K1[abs(dy)]
                tz = _max0(F(1) - np.abs(zq - z) * inv_z)
                wz = tz * tz
                dn = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                wn = _max0(dn)
                for _ in range(normal_power_log2):
                    wn = wn * wn
                da = (np.abs(aq[..., 0] - a[..., 0]) + np.abs(aq[..., 1] - a[..., 1])) + np.abs(aq[..., 2] - a[..., 2])
                ta = _max0(F(1) - da * inv_a)
                wa = ta * ta
                w = ((h * wz) * wn) * wa
                tc = _max0(F(1) - np.abs(_lum(cq) - lp) * inv_c)
                w = w * (tc * tc)
                assert w.dtype == F and inv_c.dtype == F
                acc = np.where(use[..., None], acc + w[..., None] * cq, acc)
                sw = np.where(use, sw + w, sw)
                sv = np.where(use, sv + (w * w) * vq, sv)
        took = valid & (sw > 0)
        out = np.where(took[..., None], acc / sw[..., None], c)
        vout = np.where(took, sv / (sw * sw), v)
    assert out.dtype == F and vout.dtype == F
    return out, vout


def denoise_variance(rgb32f, depth, normal, albedo, variance, iterations, sigma_depth, sigma_albedo, sigma_color, normal_power_log2):
    """n frames (n, H, W[, 3]) -> {"rgb32f", "rgb8", "variance"}; every frame on its own."""
    c = np.array(rgb32f, F)
    v = np.array(variance, F)
    for f in range(c.shape[0]):
        for i in range(iterations):
            c[f], v[f] = denoise_variance_pass(c[f], v[f], depth[f], normal[f], albedo[f], i, sigma_depth, sigma_albedo, sigma_color,
                                               normal_power_log2)
    return {"rgb32f": c, "rgb8": u8fromfloat(clamp01(c)), "variance": v}


def random_variance(z, seed=1):
    """A seeded non-negative variance plane in the shape of z: mostly the size of a noisy luminance's variance (up to 0.05),
    a tenth of the pixels converged (0) and a tenth very noisy (up to 4)."""
    rng = np.random.default_rng(seed * 104729 + z.size)
    v = (rng.random(z.shape, dtype=F) * F(0.05)).astype(F)
    pick = rng.random(z.shape)
    v[pick < 0.1] = 0
    v[pick > 0.9] = (rng.random(z.shape, dtype=F) * F(4))[pick > 0.9]
    return v
