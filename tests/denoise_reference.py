"""The filter of p3d_denoise in NumPy, written from its definition (include/p3d_hip.h, DESIGN "Denoising") and from nothing
else: float32 throughout, one operation per expression node, the taps in the defined order.  The host restatement
(p3dh_denoise) is compared with it bit for bit, and the device with the host restatement."""
import numpy as np

F = np.float32
K1 = (F(0.375), F(0.25), F(0.0625))


def _max0(v):
    return np.where(v > 0, v, F(0)).astype(F)


def _lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _tap(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside the frame."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, ye = max(0, -dy), min(h, h - dy)
    xs, xe = max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        b[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return b


def valid_depth(z):
    return np.isfinite(z) & (z > 0)


def clamp01(v):
    return np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)


def u8fromfloat(x):
    s = (x * F(255.99)).astype(F)
    return np.where(s >= F(255), 255, np.nan_to_num(s, nan=0.0).astype(np.int32) & 255).astype(np.uint8)


def denoise_pass(c, z, n, a, i, sigma_depth, sigma_albedo, sigma_color, normal_power_log2):
    """Pass i over one frame: c, n, a (H, W, 3), z (H, W) float32 -> the colour after the pass."""
    s = 1 << i
    color = sigma_color > 0
    valid = valid_depth(z)
    with np.errstate(all="ignore"):
        inv_a = F(1) / F(sigma_albedo)
        inv_c = F(1) / (F(sigma_color) * F(2.0 ** -i)) if color else F(0)
        inv_z = F(1) / (F(sigma_depth) * z)
        lp = _lum(c)
        acc = np.zeros_like(c)
        sw = np.zeros_like(z)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                zq = _tap(z, dx * s, dy * s, F(0))
                nq, aq, cq = _tap(n, dx * s, dy * s, F(0)), _tap(a, dx * s, dy * s, F(0)), _tap(c, dx * s, dy * s, F(0))
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
                if color:
                    tc = _max0(F(1) - np.abs(_lum(cq) - lp) * inv_c)
                    w = w * (tc * tc)
                assert w.dtype == F
                acc = np.where(use[..., None], acc + w[..., None] * cq, acc)
                sw = np.where(use, sw + w, sw)
        out = np.where((valid & (sw > 0))[..., None], acc / sw[..., None], c)
    assert out.dtype == F
    return out


def denoise(rgb32f, depth, normal, albedo, iterations, sigma_depth, sigma_albedo, sigma_color, normal_power_log2):
    """n frames (n, H, W[, 3]) -> {"rgb32f", "rgb8"}; every frame on its own."""
    c = np.array(rgb32f, F)
    for f in range(c.shape[0]):
        for i in range(iterations):
            c[f] = denoise_pass(c[f], depth[f], normal[f], albedo[f], i, sigma_depth, sigma_albedo, sigma_color, normal_power_log2)
    return {"rgb32f": c, "rgb8": u8fromfloat(clamp01(c))}


def random_planes(w, h, n=3, seed=1):
    """Seeded planes of n frames with the special pixels of the definition: misses (+inf), a zero depth, a NaN depth and a
    zero normal; frames of fewer than 12 pixels get them frame by frame instead (frame 1: all misses)."""
    rng = np.random.default_rng(seed * 7919 + w * 131 + h)
    c = rng.random((n, h, w, 3), dtype=F)
    z = (F(1) + rng.random((n, h, w), dtype=F)).astype(F)
    nr = rng.normal(size=(n, h, w, 3)).astype(F) * F(0.4) + np.array([0, 0, 1], F)
    nr = (nr / np.sqrt((nr * nr).sum(-1, keepdims=True))).astype(F)
    a = (rng.integers(0, 3, (n, h, w, 1)) * F(0.25) + rng.random((n, h, w, 3), dtype=F) * F(0.1)).astype(F)
    if w * h >= 12:
        for f in range(n):
            at = rng.choice(w * h, 8, replace=False)
            zf, nf = z[f].reshape(-1), nr[f].reshape(-1, 3)
            zf[at[:4]] = np.inf
            zf[at[4]] = 0.0
            zf[at[5]] = np.nan
            nf[at[6]] = 0.0
            zf[at[7]] = -1.0
    else:
        z[1 % n] = np.inf
        nr[2 % n] = 0.0
    miss = ~valid_depth(z)
    a[miss & np.isinf(z)] = 0
    return c, z, nr, a
