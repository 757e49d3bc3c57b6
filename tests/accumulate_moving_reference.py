"""p3d_accumulate_moving in NumPy, written from its definition (include/p3d_hip.h) and from nothing else: one operation per
expression node, in the stated order, in float32 -- or, with dtype=np.float64, the same formulas evaluated in double, which is
what the float32 chain's rounding is measured against.  The host restatement (p3dh_accumulate_moving) is compared with the
float32 form bit for bit, and the device with the host restatement.  Also the generator of the test sequences: a small
analytic world whose sphere, triangle and box move between frames, traced in float64."""
import numpy as np

import accumulate_reference as R

F = np.float32
SPHERE, TRIANGLE, BOX, PLANE = 0, 1, 2, 3
MEANINGFUL = {SPHERE: 4, TRIANGLE: 9, BOX: 6, PLANE: 4}


def _dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def previous_point(P, i, prim_type, a_rec, b_rec, T=F):
    """P: three (H, W) arrays of dtype T; i (H, W) int32; prim_type (n,); a_rec, b_rec (n, 12) float32: the records of the frame
    and of the frame it looks back at.  -> (P_prev as three arrays, no_point (H, W): a changed plane)."""
    n = len(prim_type)
    inside = (i >= 0) & (i < n)
    ic = np.where(inside, i, 0)
    kind = np.asarray(prim_type)[ic]
    a32, b32 = np.ascontiguousarray(a_rec, F)[ic], np.ascontiguousarray(b_rec, F)[ic]           # (H, W, 12)
    aw, bw = a32.view(np.uint32), b32.view(np.uint32)
    same = np.zeros(i.shape, bool)
    for k in np.unique(kind):
        m = MEANINGFUL.get(int(k), 4)
        same |= (kind == k) & (aw[..., :m] == bw[..., :m]).all(-1)
    static = ~inside | same
    a, b = a32.astype(T), b32.astype(T)
    A = lambda j: a[..., j]
    B = lambda j: b[..., j]
    with np.errstate(all="ignore"):
        # sphere
        s = B(3) / A(3)
        sph = [B(k) + (P[k] - A(k)) * s for k in range(3)]
        # triangle
        e1 = [A(3 + k) - A(k) for k in range(3)]
        e2 = [A(6 + k) - A(k) for k in range(3)]
        w = [P[k] - A(k) for k in range(3)]
        d11, d12, d22, w1, w2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(w, e1), _dot(w, e2)
        den = d11 * d22 - d12 * d12
        beta = (d22 * w1 - d12 * w2) / den
        gamma = (d11 * w2 - d12 * w1) / den
        tri = [(B(k) + (B(3 + k) - B(k)) * beta) + (B(6 + k) - B(k)) * gamma for k in range(3)]
        # box
        box = []
        for k in range(3):
            e = A(3 + k) - A(k)
            t = np.where(e != 0, (P[k] - A(k)) / np.where(e != 0, e, T(1)), T(0))
            box.append(B(k) + (B(3 + k) - B(k)) * t)
    out = []
    for k in range(3):
        q = np.where(kind == SPHERE, sph[k], np.where(kind == TRIANGLE, tri[k], np.where(kind == BOX, box[k], P[k])))
        q = np.where(static, P[k], q)
        assert q.dtype == T
        out.append(q)
    return out, ~static & (kind >= PLANE)


def accumulate_frame(cam, c, z, n, i, prev, prim_type, a_rec, b_rec, depth_tolerance, normal_min, max_history, T=F, probe=None):
    """One frame of p3d_accumulate_moving: the planes as accumulate_reference.accumulate_frame takes them (i is needed), prev
    None or the dict of the frame looked back at; a_rec / b_rec (n_prims, 12) the records of this frame and of that one.
    -> (colour, length, prev_xy (H, W, 2)), dtype T (the planes are converted; with T = float64 nothing rounds to float32)."""
    h, w = z.shape
    nan = np.array([0x7FC00000], np.uint32).view(F)[0].astype(T)
    length = np.ones((h, w), T)
    xy = np.full((h, w, 2), nan, T)
    c, z, n = c.astype(T), z.astype(T), n.astype(T)
    if prev is None:
        return c.copy(), length, xy
    pc = prev["cam"]
    pcol, pz, pn_, plen = (prev[k].astype(T) for k in ("rgb32f", "depth", "normal", "length"))
    v3 = lambda a: [T(a[0]), T(a[1]), T(a[2])]
    rx, ry = T(w), T(h)
    with np.errstate(all="ignore"):
        # 1. Camera::PrimaryRay((x + 0.5, y + 0.5)) and the hit point
        fx = ((np.arange(w).astype(T) + T(0.5)) / rx - T(0.5))[None, :]
        fy = ((np.arange(h).astype(T) + T(0.5)) / ry - T(0.5))[:, None]
        eye, cu, cv, cn = v3(cam.eye), v3(cam.u), v3(cam.v), v3(cam.n)
        cw, ch, cpd = T(cam.w), T(cam.h), T(cam.plane_dist)
        D = [((cu[k] * cw) * fx + (cv[k] * ch) * fy) + cn[k] * -cpd for k in range(3)]
        ln = T(1) / np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
        d = [D[k] * ln for k in range(3)]
        P = [eye[k] + d[k] * z for k in range(3)]
        # where that surface point was one frame ago
        Q, no_point = previous_point(P, i, prim_type, a_rec, b_rec, T)
        # 2. the projection into the previous camera
        peye, pu, pv, pn = v3(pc.eye), v3(pc.u), v3(pc.v), v3(pc.n)
        pw, ph, ppd = T(pc.w), T(pc.h), T(pc.plane_dist)
        q = [Q[k] - peye[k] for k in range(3)]
        a, b, cc = _dot(q, pu), _dot(q, pv), -_dot(q, pn)
        ok = R.valid_depth(z) & ~no_point & (cc > 0)
        s = cc / ppd
        gx, gy = a / (pw * s), b / (ph * s)
        px, py = (gx + T(0.5)) * rx - T(0.5), (gy + T(0.5)) * ry - T(0.5)
        ok &= (px > -1) & (px < rx) & (py > -1) & (py < ry)
        xy = np.where(ok[..., None], np.stack([px, py], -1), xy)
        x0f, y0f = np.floor(px), np.floor(py)
        tx, ty = px - x0f, py - y0f
        x0 = np.where(ok, x0f, 0).astype(np.int64)
        y0 = np.where(ok, y0f, 0).astype(np.int64)
        dist = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        lim = T(depth_tolerance) * dist
        # 3. the taps
        ux, uy = T(1) - tx, T(1) - ty
        ids = prev.get("hit_id") is not None
        acc = np.zeros_like(c)
        sl = np.zeros((h, w), T)
        sw = np.zeros((h, w), T)
        for ox, oy, wgt in ((0, 0, ux * uy), (1, 0, tx * uy), (0, 1, ux * ty), (1, 1, tx * ty)):
            qx, qy = x0 + ox, y0 + oy
            use = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            zq = pz[qyc, qxc]
            nq = pn_[qyc, qxc]
            use &= R.valid_depth(zq) & (np.abs(zq - dist) <= lim)
            use &= ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]) >= T(normal_min)
            if ids:
                use &= prev["hit_id"][qyc, qxc] == i
            acc = np.where(use[..., None], acc + wgt[..., None] * pcol[qyc, qxc], acc)
            sl = np.where(use, sl + wgt * plen[qyc, qxc], sl)
            sw = np.where(use, sw + wgt, sw)
        # 4. the blend
        took = ok & (sw > 0)
        H = acc / sw[..., None]
        ln = sl / sw + T(1)
        ln = np.where(ln > T(max_history), T(max_history), ln)
        alpha = T(1) / ln
        out = np.where(took[..., None], H + (c - H) * alpha[..., None], c)
        length = np.where(took, ln, T(1))
        if probe is not None:
            probe.update(c=cc, px=px, py=py, ok=ok, took=took, no_point=no_point, Q=Q, P=P)
    assert out.dtype == T and length.dtype == T and xy.dtype == T
    return out, length, xy


def accumulate(rgb32f, depth, normal, cams, hit_id, prim_type, prim_data, history, depth_tolerance, normal_min, max_history):
    """n frames -> {"rgb32f", "length", "prev_xy"}; prim_data (n, n_prims, 12); a history carries "prim_data" (n_prims, 12)."""
    out = np.zeros_like(rgb32f)
    length = np.zeros(depth.shape, F)
    xy = np.zeros(depth.shape + (2,), F)
    prim_data = np.asarray(prim_data, F).reshape(rgb32f.shape[0], len(prim_type), 12)
    prev = history
    for f in range(rgb32f.shape[0]):
        b_rec = prim_data[f - 1] if f > 0 else (history["prim_data"] if history is not None else prim_data[0])
        out[f], length[f], xy[f] = accumulate_frame(cams[f], rgb32f[f], depth[f], normal[f], hit_id[f], prev, prim_type, prim_data[f], b_rec,
                                                    depth_tolerance, normal_min, max_history)
        prev = dict(rgb32f=out[f], depth=depth[f], normal=normal[f], length=length[f], hit_id=hit_id[f], cam=cams[f])
    return {"rgb32f": out, "length": length, "prev_xy": xy}


# ---------------------------------------------------------------- the moving world
PRIM_TYPE = np.array([PLANE, SPHERE, TRIANGLE, BOX], np.uint32)
PALETTE = np.array([[0.55, 0.5, 0.45], [0.8, 0.3, 0.2], [0.2, 0.7, 0.3], [0.25, 0.35, 0.8]], F)
SKY = np.array([0.4, 0.6, 0.9], F)


def world(g):
    """The four records (4, 12) float32 at time g (frame f is time f, the history's frame time -1): the ground plane y = 0
    stands still; the sphere translates AND grows; the triangle's three vertices move independently; the box translates and
    stretches.  Every step is a fraction of the primitive's size."""
    rec = np.zeros((4, 12), F)
    rec[0, :4] = (0.0, 1.0, 0.0, 0.0)
    rec[1, :4] = (-1.3 + 0.10 * g, 0.9 + 0.04 * g, 0.3 - 0.08 * g, 0.7 + 0.03 * g)
    rec[2, :9] = (-0.4 + 0.05 * g, 0.15, 1.2, 1.3, 0.25 + 0.04 * g, 0.9 - 0.05 * g, 0.5 - 0.03 * g, 1.7 + 0.02 * g, 1.0)
    rec[3, :6] = (1.5 + 0.06 * g, 0.0, -1.6, 2.3 + 0.10 * g, 0.9 + 0.05 * g, -0.7)
    return rec


def trace(cam, rec):
    """The records through the pixel centres of cam, float64: depth (+inf on sky), normal, hit_id (-1 on sky), float32 / int32,
    planes bottom row first."""
    w, h = cam.res_x, cam.res_y
    rec = np.asarray(rec, np.float64)
    eye, u, v, n = (np.array(list(a), np.float64) for a in (cam.eye, cam.u, cam.v, cam.n))
    fx = ((np.arange(w) + 0.5) / w - 0.5)[None, :, None]
    fy = ((np.arange(h) + 0.5) / h - 0.5)[:, None, None]
    d = u * cam.w * fx + v * cam.h * fy - n * cam.plane_dist
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    ts, ns = [], []
    with np.errstate(all="ignore"):
        # the plane: PN . X = D
        pn, pd = rec[0, :3], rec[0, 3]
        den = d @ pn
        t = np.where(den < -1e-9, (pd - eye @ pn) / den, np.inf)
        ts.append(np.where(t > 0, t, np.inf)); ns.append(np.broadcast_to(pn, d.shape))
        # the sphere
        c, r = rec[1, :3], rec[1, 3]
        L = eye - c
        bq = d @ L
        disc = bq * bq - (L @ L - r * r)
        t = np.where(disc > 0, -bq - np.sqrt(np.abs(disc)), np.inf)
        t = np.where(t > 0, t, np.inf)
        ts.append(t); ns.append((eye + d * np.where(np.isinf(t), 0.0, t)[..., None] - c) / r)
        # the triangle (Moeller-Trumbore)
        p0, p1, p2 = rec[2, 0:3], rec[2, 3:6], rec[2, 6:9]
        e1, e2 = p1 - p0, p2 - p0
        pv = np.cross(d, e2)
        det = pv @ e1
        tv = eye - p0
        bu = (pv @ tv) / det
        qv = np.cross(tv, e1)
        bv = (d * qv).sum(-1) / det
        t = (qv @ e2) / det
        t = np.where((np.abs(det) > 1e-12) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0), t, np.inf)
        tn = np.cross(e1, e2)
        tn = tn / np.linalg.norm(tn)
        ts.append(t); ns.append(np.where(((d @ tn) > 0)[..., None], -tn, tn))
        # the box (slabs)
        mn, mx = rec[3, 0:3], rec[3, 3:6]
        t0, t1 = (mn - eye) / d, (mx - eye) / d
        near, far = np.minimum(t0, t1), np.maximum(t0, t1)
        tn_, tf = near.max(-1), far.min(-1)
        t = np.where((tn_ <= tf) & (tn_ > 0), tn_, np.inf)
        axis = near.argmax(-1)
        bn = -np.sign(np.take_along_axis(d, axis[..., None], -1)) * np.eye(3)[axis]
        ts.append(t); ns.append(bn)
    ts = np.stack(ts)
    hit = ts.argmin(0)
    t = ts.min(0)
    normal = np.take_along_axis(np.stack(ns), hit[None, ..., None], 0)[0]
    hit = np.where(np.isinf(t), -1, hit).astype(np.int32)
    normal = np.where((hit >= 0)[..., None], normal, 0.0)
    return t.astype(F), normal.astype(F), hit


def colour(hit):
    """Noise-free colour: a constant per hit id, the sky a vertical ramp."""
    h, w = hit.shape
    ramp = (0.5 + ((np.arange(h) + 0.5) / h - 0.5))[:, None, None]
    return np.where((hit >= 0)[..., None], PALETTE[np.clip(hit, 0, 3)], SKY * ramp).astype(F)


def make_sequence(res_x, res_y, n, seed=1, history=False, static_camera=False, noise=0.1, records=world, camera=None):
    """n frames of the moving world -> dict(rgb32f, depth, normal, hit_id, cams, clean, prim_type, prim_data (n, 4, 12), history).
    history: None, or the frame before frame 0 with a noisy colour, lengths between 1 and 6 and its prim_data (4, 12)."""
    rng = np.random.default_rng(seed * 7919 + res_x * 131 + res_y)
    frames = [-1] * bool(history) + list(range(n))
    camera = camera or (lambda f: R.sequence_camera(f, res_x, res_y, static_camera))
    cams = [camera(f) for f in frames]
    recs = np.stack([records(f) for f in frames]).astype(F)
    planes = [trace(c, r) for c, r in zip(cams, recs)]
    z, nr, hit = (np.stack([p[k] for p in planes]) for k in range(3))
    clean = np.stack([colour(hh) for hh in hit])
    c = (clean + rng.normal(size=clean.shape).astype(F) * F(noise)).astype(F)
    seq = dict(history=None, prim_type=PRIM_TYPE.copy())
    if history:
        seq["history"] = dict(rgb32f=c[0], depth=z[0], normal=nr[0], hit_id=hit[0], cam=cams[0], prim_data=recs[0],
                              length=(F(1) + rng.random(z[0].shape, dtype=F) * F(5)).astype(F))
        c, z, nr, hit, clean, cams, recs = c[1:], z[1:], nr[1:], hit[1:], clean[1:], cams[1:], recs[1:]
    seq.update(rgb32f=np.ascontiguousarray(c), depth=np.ascontiguousarray(z), normal=np.ascontiguousarray(nr),
               hit_id=np.ascontiguousarray(hit), clean=clean, cams=cams, prim_data=np.ascontiguousarray(recs))
    return seq


def spread_over_many_primitives(seq, copies=175):
    """The sequence with its 4 primitives copied `copies` times (ids k, k + 4, k + 8, ... carry the record of kind k) and every
    pixel's id moved to the copy of its 3 x 3 screen block: neighbouring blocks read records that share no cache line.  The
    planes change in their ids alone; equal records give equal arithmetic."""
    out = dict(seq)
    h, w = seq["hit_id"].shape[-2:]
    ys, xs = np.mgrid[0:h, 0:w]
    copy = ((xs // 3) * 37 + (ys // 3) * 101) % copies

    def spread(hit):
        return np.where(hit >= 0, hit + 4 * copy, hit).astype(np.int32)

    out["hit_id"] = np.ascontiguousarray(spread(seq["hit_id"]))
    out["prim_type"] = np.tile(seq["prim_type"], copies)
    out["prim_data"] = np.ascontiguousarray(np.tile(seq["prim_data"], (1, copies, 1)))
    if seq["history"] is not None:
        out["history"] = dict(seq["history"], hit_id=spread(seq["history"]["hit_id"]), prim_data=np.tile(seq["history"]["prim_data"], (copies, 1)))
    return out


def args(seq, history="own"):
    """The positional arguments of api.host_accumulate_moving / DeviceScene.accumulate_moving for a sequence."""
    h = seq["history"] if history == "own" else history
    return (seq["rgb32f"], seq["depth"], seq["normal"], seq["cams"], seq["hit_id"], seq["prim_type"], seq["prim_data"], h)
