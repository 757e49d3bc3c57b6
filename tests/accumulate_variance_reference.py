"""p3d_accumulate_variance in NumPy, written from its definition (include/p3d_hip.h) and from nothing else: float32
throughout, one operation per expression node, the taps in the defined order.  The host restatement
(p3dh_accumulate_variance) is compared with it bit for bit, and the device with the host restatement.  The colour, length
and prev_xy it returns are restated here too, so that their equality with p3d_accumulate[_moving] is a finding of the
tests and not an assumption of this file."""
import numpy as np

import accumulate_moving_reference as AM
import accumulate_reference as R
from denoise_reference import _lum, _max0, _tap

F = np.float32


def _dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def moments_of(c):
    """m = (l, l * l) of a colour plane (..., 3) -> (..., 2)."""
    l = _lum(c)
    return np.stack([l, l * l], -1).astype(F)


def temporal_frame(cam, c, z, n, i, prev, moved, depth_tolerance, normal_min, max_history, probe=None):
    """Steps 0 to 4 for one frame with the moments in them.  prev: None, or the dict of the frame looked back at -- rgb32f,
    depth, normal, length, moments, hit_id (or None), cam.  moved: None (a static world), or (prim_type, a_rec, b_rec) of
    p3d_accumulate_moving.  -> (colour, length, moments, temporal variance, prev_xy)."""
    h, w = z.shape
    nan = np.array([0x7FC00000], np.uint32).view(F)[0]
    xy = np.full((h, w, 2), nan, F)
    m = moments_of(c)
    length = np.ones((h, w), F)
    out, om = c.copy(), m.copy()
    if prev is not None:
        pc = prev["cam"]
        v3 = lambda a: [F(a[0]), F(a[1]), F(a[2])]
        rx, ry = F(w), F(h)
        with np.errstate(all="ignore"):
            # 1. Camera::PrimaryRay((x + 0.5, y + 0.5)) and the hit point
            fx = ((np.arange(w, dtype=F) + F(0.5)) / rx - F(0.5))[None, :]
            fy = ((np.arange(h, dtype=F) + F(0.5)) / ry - F(0.5))[:, None]
            eye, cu, cv, cn = v3(cam.eye), v3(cam.u), v3(cam.v), v3(cam.n)
            cw, ch, cpd = F(cam.w), F(cam.h), F(cam.plane_dist)
            D = [((cu[k] * cw) * fx + (cv[k] * ch) * fy) + cn[k] * -cpd for k in range(3)]
            ln = F(1) / np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
            d = [D[k] * ln for k in range(3)]
            P = [eye[k] + d[k] * z for k in range(3)]
            no_point = np.zeros((h, w), bool)
            Q = P
            if moved is not None:
                Q, no_point = AM.previous_point(P, i, *moved)
            # 2. the projection into the previous camera
            peye, pu, pv, pn = v3(pc.eye), v3(pc.u), v3(pc.v), v3(pc.n)
            pw, ph, ppd = F(pc.w), F(pc.h), F(pc.plane_dist)
            q = [Q[k] - peye[k] for k in range(3)]
            a, b, cc = _dot(q, pu), _dot(q, pv), -_dot(q, pn)
            ok = R.valid_depth(z) & ~no_point & (cc > 0)
            s = cc / ppd
            gx, gy = a / (pw * s), b / (ph * s)
            px, py = (gx + F(0.5)) * rx - F(0.5), (gy + F(0.5)) * ry - F(0.5)
            ok &= (px > -1) & (px < rx) & (py > -1) & (py < ry)
            xy = np.where(ok[..., None], np.stack([px, py], -1), xy)
            x0f, y0f = np.floor(px), np.floor(py)
            tx, ty = px - x0f, py - y0f
            x0 = np.where(ok, x0f, 0).astype(np.int64)
            y0 = np.where(ok, y0f, 0).astype(np.int64)
            dist = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
            lim = F(depth_tolerance) * dist
            # 3. the taps: colour, length, then the two moments, then the weight
            ux, uy = F(1) - tx, F(1) - ty
            ids = i is not None and prev.get("hit_id") is not None
            acc = np.zeros_like(c)
            sl = np.zeros((h, w), F)
            sm = np.zeros((h, w, 2), F)
            sw = np.zeros((h, w), F)
            for ox, oy, wgt in ((0, 0, ux * uy), (1, 0, tx * uy), (0, 1, ux * ty), (1, 1, tx * ty)):
                qx, qy = x0 + ox, y0 + oy
                use = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                zq = prev["depth"][qyc, qxc]
                nq = prev["normal"][qyc, qxc]
                use &= R.valid_depth(zq) & (np.abs(zq - dist) <= lim)
                use &= ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]) >= F(normal_min)
                if ids:
                    use &= prev["hit_id"][qyc, qxc] == i
                assert wgt.dtype == F
                acc = np.where(use[..., None], acc + wgt[..., None] * prev["rgb32f"][qyc, qxc], acc)
                sl = np.where(use, sl + wgt * prev["length"][qyc, qxc], sl)
                sm = np.where(use[..., None], sm + wgt[..., None] * prev["moments"][qyc, qxc], sm)
                sw = np.where(use, sw + wgt, sw)
            # 4. the blend, the moments with the colour's alpha
            took = ok & (sw > 0)
            H = acc / sw[..., None]
            ln = sl / sw + F(1)
            ln = np.where(ln > F(max_history), F(max_history), ln)
            alpha = F(1) / ln
            out = np.where(took[..., None], H + (c - H) * alpha[..., None], c)
            length = np.where(took, ln, F(1))
            Hm = sm / sw[..., None]
            om = np.where(took[..., None], Hm + (m - Hm) * alpha[..., None], m)
            if probe is not None:
                probe.update(took=took, ok=ok)
    with np.errstate(all="ignore"):
        vt = om[..., 1] - om[..., 0] * om[..., 0]
    vt = np.where(R.valid_depth(z), np.where(vt > 0, vt, F(0)), F(0)).astype(F)
    assert out.dtype == F and length.dtype == F and om.dtype == F and xy.dtype == F
    return out, length, om, vt, xy


def spatial_frame(c, z, n, length, vt, min_temporal, radius, sigma_depth, normal_power_log2, probe=None):
    """The variance of one frame: vt, replaced by the spatial estimate over the frame's INPUT colour where Z is valid, the
    output length is below min_temporal and the taps carry weight."""
    valid = R.valid_depth(z)
    lq_all = _lum(c)
    with np.errstate(all="ignore"):
        inv_z = F(1) / (F(sigma_depth) * z)
        s1 = np.zeros_like(z)
        s2 = np.zeros_like(z)
        sw = np.zeros_like(z)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                zq, nq, lq = _tap(z, dx, dy, F(0)), _tap(n, dx, dy, F(0)), _tap(lq_all, dx, dy, F(0))
                use = valid & R.valid_depth(zq)
                tz = _max0(F(1) - np.abs(zq - z) * inv_z)
                wz = tz * tz
                wn = _max0((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                for _ in range(normal_power_log2):
                    wn = wn * wn
                wgt = wz * wn
                assert wgt.dtype == F
                s1 = np.where(use, s1 + wgt * lq, s1)
                s2 = np.where(use, s2 + wgt * (lq * lq), s2)
                sw = np.where(use, sw + wgt, sw)
        a, b = s1 / sw, s2 / sw
        est = _max0(b - a * a)
    spatial = valid & (length < F(min_temporal)) & (sw > 0)
    if probe is not None:
        probe.update(spatial=spatial)
    out = np.where(spatial, est, vt)
    assert out.dtype == F
    return out


def accumulate_variance(rgb32f, depth, normal, cams, hit_id, history, motion, depth_tolerance, normal_min, max_history, min_temporal, radius,
                        sigma_depth, normal_power_log2, probes=None):
    """n frames -> {"rgb32f", "length", "moments", "variance"[, "prev_xy"]}.  history: None, or accumulate_reference's dict
    with "moments" (and "prim_data" with a motion).  motion: None or dict(prim_type, prim_data (n, n_prims, 12)).  probes: a
    list that receives one dict per frame with `took` (a history was blended in) and `spatial` (the estimate was taken)."""
    nf = rgb32f.shape[0]
    out = {"rgb32f": np.zeros_like(rgb32f), "length": np.zeros(depth.shape, F), "moments": np.zeros(depth.shape + (2,), F),
           "variance": np.zeros(depth.shape, F)}
    if motion is not None:
        out["prev_xy"] = np.zeros(depth.shape + (2,), F)
        prim_data = np.asarray(motion["prim_data"], F).reshape(nf, len(motion["prim_type"]), 12)
    prev = history
    for f in range(nf):
        moved = None
        if motion is not None:
            b_rec = prim_data[f - 1] if f > 0 else (history["prim_data"] if history is not None else prim_data[0])
            moved = (motion["prim_type"], prim_data[f], b_rec)
        i = None if hit_id is None else hit_id[f]
        probe = {}
        c, l, m, vt, xy = temporal_frame(cams[f], rgb32f[f], depth[f], normal[f], i, prev, moved, depth_tolerance, normal_min, max_history, probe)
        out["rgb32f"][f], out["length"][f], out["moments"][f] = c, l, m
        out["variance"][f] = spatial_frame(rgb32f[f], depth[f], normal[f], l, vt, min_temporal, radius, sigma_depth, normal_power_log2, probe)
        if motion is not None:
            out["prev_xy"][f] = xy
        if probes is not None:
            probe.setdefault("took", np.zeros(depth[f].shape, bool))
            probes.append(probe)
        prev = dict(rgb32f=c, depth=depth[f], normal=normal[f], length=l, moments=m, hit_id=i, cam=cams[f])
    return out


def with_moments(history, seed=1):
    """accumulate_reference.make_sequence's history with a "moments" plane such a history could have accumulated: the
    moments of its colour, the second one raised by a seeded non-negative variance."""
    if history is None:
        return None
    rng = np.random.default_rng(seed * 613 + history["depth"].size)
    m = moments_of(history["rgb32f"])
    m[..., 1] = (m[..., 1] + rng.random(m.shape[:-1], dtype=F) * F(0.02)).astype(F)
    return dict(history, moments=m)
