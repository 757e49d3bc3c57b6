"""NumPy restatement of p3d_indirect_diffuse's definition (include/p3d_hip.h), steps 8 and 9, written from the header text:
float32 IEEE additions in the order of the balanced tree, one product by 1 / samples, a product and a sum per output channel.
Not a test module.  It shares no code with the C++: the host restatement (p3dh_indirect_resolve) is compared with it bit for
bit, and the device with both.  Steps 1 to 6 are ao_reference.segments at radius 1; step 7, the radiance, is p3d_trace_rays':
the tests ask DeviceScene.trace_rays or the oracle's rayTracing()."""
import ctypes as C

import numpy as np

import ao_reference as AO

F = np.float32


def rays(cam, depth, normal, samples, bias, seed, frame=0):
    """Steps 1 to 6 for one frame: origin, dir (H, W, samples, 3) and valid (H, W) uint8."""
    return AO.segments(cam, depth, normal, samples, 1.0, bias, seed, frame)


def tree_sum(r):
    """Step 8's sum over axis -2 of r (..., S, 3), S a power of two: t[i] = t[2 i] + t[2 i + 1] until one term is left."""
    t = np.asarray(r, F)
    with np.errstate(all="ignore"):
        while t.shape[-2] > 1:
            t = (t[..., 0::2, :] + t[..., 1::2, :]).astype(F)
    return t[..., 0, :]


def serial_sum(r):
    """The left-to-right sum the definition does NOT use (the tests show that it differs)."""
    r = np.asarray(r, F)
    t = r[..., 0, :].copy()
    with np.errstate(all="ignore"):
        for s in range(1, r.shape[-2]):
            t = (t + r[..., s, :]).astype(F)
    return t


def resolve(radiance, valid, albedo=None, rgb32f=None):
    """Steps 8 and 9: radiance (..., S, 3), valid (...) -> {"indirect" (..., 3), "rgb32f" (..., 3)}."""
    radiance = np.asarray(radiance, F)
    S = radiance.shape[-2]
    q = np.asarray(valid).astype(bool)[..., None]
    with np.errstate(all="ignore"):
        m = (tree_sum(radiance) * (F(1.0) / F(S))).astype(F)
        m = np.where(q, m, F(0.0)).astype(F)
        am = m if albedo is None else (np.asarray(albedo, F) * m).astype(F)
        if rgb32f is None:
            rgb = np.where(q, am, F(0.0))
        else:
            c = np.asarray(rgb32f, F)
            rgb = np.where(q, (c + am).astype(F), c)
    return {"indirect": np.ascontiguousarray(m, F), "rgb32f": np.ascontiguousarray(rgb, F)}


def radiance_from(answer, rays_of_frames, samples):
    """(n, H, W, S, 3) radiances from answer(o [m, 3], d [m, 3]) -> (m, 3) colours, asked for the rays of valid pixels only
    (zeros elsewhere: they are not read)."""
    out = []
    for o, d, v in rays_of_frames:
        m = v.astype(bool)
        full = np.zeros(m.shape + (samples, 3), F)
        if m.any():
            full[m] = np.asarray(answer(o[m].reshape(-1, 3), d[m].reshape(-1, 3)), F).reshape(-1, samples, 3)
        out.append(full)
    return np.stack(out)


def oracle_radiance(osc, accel):
    """answer() of radiance_from through the CPU oracle: rayTracing(ray, 1, 1.0) with MAX_DEPTH 1 per ray."""
    return lambda o, d: np.array([osc.trace(accel, a, b, max_depth=1) for a, b in zip(o, d)], F)


def census(osc, oracle_lib, o, d):
    """What the rays (m, 3) meet, from the oracle's intersectors and its BVH shadow query alone: hit (m,) bool, and shadowed
    (m,) bool -- the ray hits, a light lies on the hit's side (L . N > 0) and the shadow query from the hit towards that
    light answers "occluded", so the sample is darker than its unshadowed term."""
    ptype, prim, _ = osc.prims()
    lights = osc.lights()
    fp = C.POINTER(C.c_float)
    keep = [np.ascontiguousarray(prim[j]) for j in range(len(ptype))]
    pp = [a.ctypes.data_as(fp) for a in keep]
    t, nrm = np.zeros(1, F), np.zeros(3, F)
    hit, shadowed = np.zeros(len(o), bool), np.zeros(len(o), bool)
    for i in range(len(o)):
        ro, rd = np.ascontiguousarray(o[i], F), np.ascontiguousarray(d[i], F)
        best, n = np.inf, None
        for j in range(len(keep)):
            if oracle_lib.p3o_intersect(int(ptype[j]), pp[j], ro.ctypes.data_as(fp), rd.ctypes.data_as(fp), t.ctypes.data_as(fp),
                                        nrm.ctypes.data_as(fp)) and t[0] < best:
                best, n = float(t[0]), nrm.copy()
        if n is None:
            continue
        hit[i] = True
        point = (ro + rd * F(best)).astype(F)
        for li in lights:
            L = (li[:3] - point).astype(F)
            if float(np.dot(L.astype(np.float64), n.astype(np.float64))) > 0 and osc.refbvh_shadow((point + n * F(0.001)).astype(F), L):
                shadowed[i] = True
    return hit, shadowed
