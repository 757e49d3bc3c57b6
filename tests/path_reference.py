"""NumPy restatement of p3d_indirect_paths' definition (include/p3d_hip.h), steps 3 to 5, written from the header text:
float32 IEEE basic operations in the order given there, rng_mix in uint32.  Not a test module.  It shares no code with the
C++: the host restatement (p3dh_path_next, p3dh_path_add) is compared with it bit for bit, and the device with both.  Step 1,
vertex 0, is indirect_reference.rays; step 2, a ray's answer, is p3d_trace_rays': the tests ask DeviceScene.trace_rays or the
oracle; step 5 is indirect_reference.resolve."""
import ctypes as C

import numpy as np

import ao_reference as AO
import indirect_reference as R

F = np.float32
U = np.uint32
BOUNCE_KEY = 0x80000000


def cosine_direction(Ns, pk, s):
    """Steps 5 and 6 of p3d_ambient_occlusion at radius 1 from Ns (m, 3) with the keys rng_mix(pk, s), pk and s (m,)."""
    Ns = np.asarray(Ns, F)
    with np.errstate(all="ignore"):
        k = AO.rng_mix(pk, s)
        v = Ns.copy()
        open_ = np.ones(len(Ns), bool)
        for j in range(AO.TRIES):
            c = np.stack([F(2.0) * AO.rng_u01(k, U(3 * j + i)) - F(1.0) for i in range(3)], axis=-1).astype(F)
            q = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
            take = open_ & (q <= F(1.0)) & (q >= AO.TINY)
            v[take] = AO.normalized(c)[take]
            open_ &= ~take
            if not open_.any():
                break
        w = (Ns + v).astype(F)
        ww = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
        w = np.where((ww >= AO.TINY)[..., None], w, Ns).astype(F)
        return (AO.normalized(w) * F(1.0)).astype(F)


def path_next(b, bias, o, d, t, n, hit_id, prim_material, materials12, pk0, s, T=None):
    """Step 4 for m paths that just traced ray b: -> next origin, direction (m, 3), T_(b+1) (m, 3), alive (m,) uint8.  Where the
    path has no next vertex (hit_id < 0) the ray is zeros and T is left as it was."""
    o, d, n = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3), np.asarray(n, F).reshape(-1, 3)
    m = len(o)
    t, hit_id = np.asarray(t, F).reshape(m), np.asarray(hit_id, np.int32).reshape(m)
    T = np.zeros((m, 3), F) if T is None else np.array(T, F).reshape(m, 3)
    alive = hit_id >= 0
    materials12 = np.asarray(materials12, F).reshape(-1, 12)
    with np.errstate(all="ignore"):
        P = (o + (d * t[:, None]).astype(F)).astype(F)
        a = materials12[np.asarray(prim_material)[np.where(alive, hit_id, 0)], 0:3]
        Tn = a.copy() if b == 0 else (T * a).astype(F)
        away = ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]) > 0
        Ns = np.where(away[:, None], -n, n).astype(F)
        O = (P + (Ns * F(bias)).astype(F)).astype(F)
        pk = AO.rng_mix(np.asarray(pk0, U), U((BOUNCE_KEY + b + 1) & 0xFFFFFFFF))
        D = cosine_direction(Ns, pk, np.asarray(s, U))
    live = alive[:, None]
    return (np.ascontiguousarray(np.where(live, O, F(0)), F), np.ascontiguousarray(np.where(live, D, F(0)), F),
            np.ascontiguousarray(np.where(live, Tn, T), F), alive.astype(np.uint8))


def path_add(b, T, r, alive, total):
    """Step 3: R = r_0 for b == 0, else R + T_b * r_b, where alive."""
    r, total = np.asarray(r, F).reshape(-1, 3), np.asarray(total, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        new = r if b == 0 else (total + (np.asarray(T, F).reshape(-1, 3) * r).astype(F)).astype(F)
    return np.ascontiguousarray(np.where(np.asarray(alive).astype(bool)[:, None], new, total), F)


def paths(answer, cams, planes, S, B, bias, seed, materials, next_fn=path_next, add_fn=path_add):
    """The whole definition over n frames.  answer(o (m, 3), d (m, 3)) -> (rgb (m, 3), hit_id (m,), t (m,), normal (m, 3)) is
    step 2; planes: depth (n, H, W), normal (n, H, W, 3) and optionally albedo, rgb32f (n, H, W, 3); materials:
    (prim_material, materials12) of the scene description.  Rays are asked for live paths only, compacted.  Returns indirect
    and rgb32f (n, H, W, 3), R (n, H, W, S, 3) per-sample sums, prefix (B, n, H, W, S, 3) -- R after every bounce --, valid
    (n, H, W), and the census: traced[b] = paths that traced
    ray b, missed[b] = those of them that missed, nonzero[b] = those whose term T_b * r_b is not zero."""
    prim_material, materials12 = materials
    depth, normal = np.asarray(planes["depth"], F), np.asarray(planes["normal"], F)
    n, H, W = depth.shape
    prefix, valid = np.zeros((B, n, H, W, S, 3), F), np.zeros((n, H, W), np.uint8)
    traced, missed, nonzero = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    for f in range(n):
        o, d, v = R.rays(cams[f], depth[f], normal[f], S, bias, seed, f)
        valid[f] = v
        q = v.astype(bool)
        if not q.any():
            continue
        pix = (np.arange(H, dtype=U)[:, None] * U(W) + np.arange(W, dtype=U)[None, :]).astype(U)
        pk0 = np.repeat(AO.rng_mix(U((int(seed) + f) & 0xFFFFFFFF), pix)[q], S)
        s = np.tile(np.arange(S, dtype=U), int(q.sum()))
        o, d = o[q].reshape(-1, 3), d[q].reshape(-1, 3)
        m = len(o)
        total, T = np.zeros((m, 3), F), np.zeros((m, 3), F)
        live = np.arange(m)                                    # indices of the paths still alive, compacted
        for b in range(B):
            if len(live):
                rgb, hit_id, t, nrm = answer(o, d)
                rgb = np.asarray(rgb, F).reshape(-1, 3)
                total[live] = add_fn(b, T[live], rgb, np.ones(len(live), np.uint8), total[live])
                traced[b] += len(live)
                missed[b] += int((np.asarray(hit_id) < 0).sum())
                with np.errstate(all="ignore"):
                    term = rgb if b == 0 else (T[live] * rgb).astype(F)
                nonzero[b] += int((term != 0).any(axis=-1).sum())
            prefix[b, f][q] = total.reshape(-1, S, 3)
            if b + 1 < B and len(live):
                o2, d2, T2, alive = next_fn(b, bias, o, d, t, nrm, hit_id, prim_material, materials12, pk0[live], s[live], T[live])
                T[live] = T2
                keep = alive.astype(bool)
                live, o, d = live[keep], np.ascontiguousarray(o2[keep]), np.ascontiguousarray(d2[keep])
    Rs = prefix[B - 1]
    out = R.resolve(Rs, valid, planes.get("albedo"), planes.get("rgb32f"))
    out.update(R=Rs, prefix=prefix, valid=valid, traced=traced, missed=missed, nonzero=nonzero)
    return out


def device_answer(ds, accel, **mode):
    """answer() of paths through DeviceScene.trace_rays at max_depth 1."""
    def answer(o, d):
        r = ds.trace_rays(o, d, max_depth=1, accel=accel, **mode)
        return r["rgb32f"], r["hit_id"], r["t"], r["normal"]
    return answer


def oracle_answer(osc, oracle_lib, accel):
    """answer() of paths through the CPU oracle: the closest hit from a loop over p3o_intersect, the lowest index winning
    ties (t and the normal at O + D t are that intersector's), the colour from rayTracing(ray, 1, 1.0) with MAX_DEPTH 1."""
    ptype, prim, _ = osc.prims()
    fp = C.POINTER(C.c_float)
    keep = [np.ascontiguousarray(prim[j]) for j in range(len(ptype))]
    pp = [a.ctypes.data_as(fp) for a in keep]

    def answer(o, d):
        m = len(o)
        rgb, hit_id, ts, nrm = np.zeros((m, 3), F), np.full(m, -1, np.int32), np.full(m, np.inf, F), np.zeros((m, 3), F)
        t, nn = np.zeros(1, F), np.zeros(3, F)
        for i in range(m):
            ro, rd = np.ascontiguousarray(o[i], F), np.ascontiguousarray(d[i], F)
            for j in range(len(keep)):
                if oracle_lib.p3o_intersect(int(ptype[j]), pp[j], ro.ctypes.data_as(fp), rd.ctypes.data_as(fp), t.ctypes.data_as(fp),
                                            nn.ctypes.data_as(fp)) and t[0] < ts[i]:
                    ts[i], hit_id[i], nrm[i] = t[0], j, nn
            rgb[i] = osc.trace(accel, ro, rd, max_depth=1)
        return rgb, hit_id, ts, nrm
    return answer
