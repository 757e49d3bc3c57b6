"""p3d_upsample restated in NumPy from the definition in include/p3d_hip.h and nothing else: float32 IEEE operations in the
header's order, whole planes at a time.  Also the planes the upsampler's tests run on."""
import numpy as np

F = np.float32


def valid(z):
    """A depth is valid when it is finite and > 0."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0)


def max0(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, v, F(0)).astype(F)


def axis_taps(size_high, s):
    """Per full-resolution coordinate: the first tap i0 and the weights (b0, b1) of taps i0 and i0 + 1."""
    x = np.arange(size_high, dtype=np.int64)
    t = 2 * x + 1 - s
    i0 = t // (2 * s)                                     # floor division
    r = t - 2 * s * i0
    assert ((r >= 0) & (r < 2 * s)).all()
    fx = r.astype(F) / F(2 * s)
    return i0, (F(1) - fx, fx)


def upsample(low, low_depth, low_normal, depth, normal, sigma_depth, normal_power_log2, info=False):
    """Planes as api.host_upsample takes them, with a leading frame axis: low (n, h, w) or (n, h, w, 3), low_depth (n, h, w),
    low_normal (n, h, w, 3), depth (n, H, W), normal (n, H, W, 3).  Returns {"plane", "fallback"}; with info also "fractional":
    pixels one of whose contributing taps has a weight strictly between 0 and its bilinear weight."""
    lz, z = np.asarray(low_depth, F), np.asarray(depth, F)
    n, h, w = lz.shape
    H, W = z.shape[1:]
    s = W // w
    assert (W, H) == (w * s, h * s) and 1 <= s <= 4
    lo = np.asarray(low, F).reshape(n, h, w, -1)
    c = lo.shape[-1]
    ln, nr = np.asarray(low_normal, F), np.asarray(normal, F)
    i0, bx = axis_taps(W, s)
    j0, by = axis_taps(H, s)
    centre = valid(z)
    sigma = F(sigma_depth)
    with np.errstate(all="ignore"):
        inv_z = (F(1) / (sigma * z)).astype(F)
        sums = np.zeros((n, H, W, c), F)
        sw = np.zeros((n, H, W), F)
        bsums = np.zeros((n, H, W, c), F)
        bsw = np.zeros((n, H, W), F)
        fractional = np.zeros((n, H, W), bool)
        for dy in (0, 1):
            for dx in (0, 1):
                i, j = i0 + dx, j0 + dy
                inside = ((j >= 0) & (j < h))[:, None] & ((i >= 0) & (i < w))[None, :]
                ic, jc = np.clip(i, 0, w - 1), np.clip(j, 0, h - 1)
                b = (bx[dx][None, :] * by[dy][:, None]).astype(F)[None]
                zq = lz[:, jc][:, :, ic]
                nq = ln[:, jc][:, :, ic]
                cq = lo[:, jc][:, :, ic]
                tz = max0(F(1) - np.abs(zq - z) * inv_z)
                wz = tz * tz
                wn = max0((nr[..., 0] * nq[..., 0] + nr[..., 1] * nq[..., 1]) + nr[..., 2] * nq[..., 2])
                for _ in range(normal_power_log2):
                    wn = wn * wn
                guided = ((b * wz) * wn).astype(F)
                on_surface = inside[None] & centre & valid(zq)
                in_sky = inside[None] & ~centre & ~valid(zq)
                m = on_surface | in_sky
                wt = np.where(on_surface, guided, np.broadcast_to(b, guided.shape)).astype(F)
                sums = np.where(m[..., None], sums + wt[..., None] * cq, sums).astype(F)
                sw = np.where(m, sw + wt, sw).astype(F)
                fractional |= on_surface & (guided > 0) & (guided < b)
                mb = np.broadcast_to(inside[None], m.shape)
                bsums = np.where(mb[..., None], bsums + b[..., None] * cq, bsums).astype(F)
                bsw = np.where(mb, bsw + b, bsw).astype(F)
        explained = sw > 0
        assert (bsw > 0).all(), "at least one tap inside the frame has b > 0"
        plane = np.where(explained[..., None], sums / sw[..., None], bsums / bsw[..., None]).astype(F)
    out = {"plane": plane.reshape(np.asarray(depth).shape + ((3,) if np.asarray(low).ndim == 4 else ())),
           "fallback": (~explained).astype(np.uint8)}
    if info:
        out["fractional"] = fractional
    return out


def random_planes(lw, lh, s, n, channels, seed):
    """Matching low and full-resolution planes of n frames -> (low, low_depth, low_normal, depth, normal).  Three piecewise
    surfaces (two slanted planes and a sky band of misses) and a strip thinner than a full-resolution pixel, all sampled
    analytically at the low and at the full-resolution pixel centres; depths and normals perturbed per sample, so that weights
    are fractional; a few NaN and 0 depths in either resolution."""
    rng = np.random.default_rng(seed)
    W, H = lw * s, lh * s

    def sample(X, Y, f):
        """The scene at the points (X, Y) in full-resolution pixels."""
        X, Y = np.broadcast_arrays(X, Y)
        u, v = X / (lw * s), Y / (lh * s)
        far = u > 0.55 + 0.2 * (v - 0.5) + 0.03 * f
        sky = v > 0.72 + 0.1 * u
        z = np.where(far, 5.0 + 0.5 * u + 0.2 * v, 2.0 + 0.3 * u - 0.2 * v)
        nrm = np.where(far[..., None], (0.6, 0.0, 0.8), (0.1, 0.2, 0.97))
        sig = np.where(far[..., None], (0.2, 0.7, 0.4), (0.9, 0.3, 0.6)) + 0.2 * np.sin(7 * u + 5 * v)[..., None]
        # the strip: a column 0.2 pixels wide through the centre of full-resolution column xf; low centres s (i + 0.5) miss it
        # for every s >= 2 (s = 3: centres lie in columns 1 mod 3, xf is 2 mod 3)
        xf = s * max(1, lw // 3) + (s - 1)
        strip = (np.abs(X - (xf + 0.5)) < 0.1) & ~sky
        z = np.where(strip, 0.5, z)
        nrm = np.where(strip[..., None], (-0.7, 0.1, 0.7), nrm)
        sig = np.where(strip[..., None], (0.05, 0.05, 0.9), sig)
        z = z * (1 + 0.04 * (rng.random(z.shape) - 0.5))
        nrm = nrm + 0.15 * (rng.random(nrm.shape) - 0.5)
        nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
        z = np.where(sky, np.inf, z)
        nrm = np.where(sky[..., None], 0.0, nrm)
        sig = np.where(sky[..., None], (0.3, 0.5, 1.0), sig)
        z = z.astype(F)
        k = max(1, z.size // 40)
        at = rng.choice(z.size, min(2 * k, z.size), replace=False)
        z.reshape(-1)[at[:k]] = np.nan
        z.reshape(-1)[at[k:]] = 0.0
        return z, nrm.astype(F), sig.astype(F)

    lows, highs = [], []
    for f in range(n):
        lows.append(sample(s * (np.arange(lw) + 0.5)[None, :], s * (np.arange(lh) + 0.5)[:, None], f))
        highs.append(sample((np.arange(W) + 0.5)[None, :], (np.arange(H) + 0.5)[:, None], f))
    lz, ln, lo = (np.stack(a) for a in zip(*lows))
    z, nr, _ = (np.stack(a) for a in zip(*highs))
    low = np.ascontiguousarray(lo if channels == 3 else lo[..., 0])
    return low, lz, ln, z, nr
