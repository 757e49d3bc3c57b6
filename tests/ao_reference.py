"""NumPy restatement of p3d_ambient_occlusion's definition (include/p3d_hip.h), steps 1 to 6 and 8, written from the header
text: float32 IEEE basic operations in the order given there, rng_mix in uint32.  Not a test module.  It shares no code with
the C++: the host restatement (p3dh_ao_segments, p3dh_ao_resolve) is compared with it bit for bit, and the device with both.
Step 7, the query, is p3d_occluded's: the tests ask DeviceScene.occluded or the oracle's traversals."""
import numpy as np

F = np.float32
U = np.uint32
TINY = F(2.0 ** -20)
TRIES = 32


def rng_mix(a, b):
    with np.errstate(over="ignore"):
        a, b = np.asarray(a, U), np.asarray(b, U)
        h = (a ^ U(0x9E3779B9)) * U(0x85EBCA6B) + b
        h = h ^ (h >> U(16)); h = h * U(0x7FEB352D); h = h ^ (h >> U(15)); h = h * U(0x846CA68B); h = h ^ (h >> U(16))
        return h


def rng_u01(key, k):
    return (rng_mix(key, k) >> U(8)).astype(F) * F(2.0 ** -24)


def valid_depth(z):
    return np.isfinite(z) & (z > 0)


def normalized(a):
    """The project's normalized(): l = 1 / sqrt((x^2 + y^2) + z^2), a * l."""
    with np.errstate(all="ignore"):
        s = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
        l = F(1.0) / np.sqrt(s, dtype=F)
        return (a * l[..., None]).astype(F)


def camera_fields(cam):
    """eye, u * w, v * h, n * -plane_dist of a p3d_camera (ctypes), as float32 vectors."""
    g = lambda v: np.array(list(v), F)
    return g(cam.eye), g(cam.u) * F(cam.w), g(cam.v) * F(cam.h), g(cam.n) * -F(cam.plane_dist)


def segments(cam, depth, normal, samples, radius, bias, seed, frame=0):
    """Steps 1 to 6 for one frame: depth (H, W), normal (H, W, 3) -> origin, dir (H, W, samples, 3) float32 and valid (H, W)
    uint8; zeros where the pixel has no query."""
    depth = np.asarray(depth, F)
    normal = np.asarray(normal, F)
    H, W = depth.shape
    S = int(samples)
    radius, bias = F(radius), F(bias)
    eye, uw, vh, vz = camera_fields(cam)
    valid = valid_depth(depth)                                                    # 1.
    with np.errstate(all="ignore"):
        x, y = np.arange(W, dtype=F)[None, :], np.arange(H, dtype=F)[:, None]
        fx = ((x + F(0.5)) / F(W) - F(0.5)) + np.zeros((H, 1), F)                 # 2.
        fy = ((y + F(0.5)) / F(H) - F(0.5)) + np.zeros((1, W), F)
        D = (uw[None, None, :] * fx[..., None] + vh[None, None, :] * fy[..., None]) + vz[None, None, :]
        d = normalized(D.astype(F))
        Z = np.where(valid, depth, F(1.0))
        P = eye[None, None, :] + d * Z[..., None]
        away = (normal[..., 0] * d[..., 0] + normal[..., 1] * d[..., 1]) + normal[..., 2] * d[..., 2] > 0      # 3.
        Ns = np.where(away[..., None], -normal, normal).astype(F)
        O = (P + Ns * bias).astype(F)
        pix = (np.arange(H, dtype=U)[:, None] * U(W) + np.arange(W, dtype=U)[None, :]).astype(U)               # 4.
        pk = rng_mix(U((int(seed) + int(frame)) & 0xFFFFFFFF), pix)
        k = rng_mix(pk[..., None], np.arange(S, dtype=U)[None, None, :])         # (H, W, S)
        v = np.broadcast_to(Ns[:, :, None, :], (H, W, S, 3)).astype(F).copy()     # 5.
        open_ = np.ones((H, W, S), bool)
        for j in range(TRIES):
            c = np.stack([F(2.0) * rng_u01(k, U(3 * j + i)) - F(1.0) for i in range(3)], axis=-1).astype(F)
            q = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
            take = open_ & (q <= F(1.0)) & (q >= TINY)
            v[take] = normalized(c)[take]
            open_ &= ~take
            if not open_.any():
                break
        w = (Ns[:, :, None, :] + v).astype(F)                                     # 6.
        ww = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
        w = np.where((ww >= TINY)[..., None], w, Ns[:, :, None, :]).astype(F)
        L = (normalized(w) * radius).astype(F)
    origin = np.where(valid[:, :, None, None], np.broadcast_to(O[:, :, None, :], (H, W, S, 3)), F(0)).astype(F)
    direction = np.where(valid[:, :, None, None], L, F(0)).astype(F)
    return np.ascontiguousarray(origin), np.ascontiguousarray(direction), valid.astype(np.uint8)


def tries_needed(samples, seed, frame, H, W):
    """How many tries the slowest sample of a frame needed (TRIES + 1: none was accepted)."""
    pix = (np.arange(H, dtype=U)[:, None] * U(W) + np.arange(W, dtype=U)[None, :]).astype(U)
    k = rng_mix(rng_mix(U((int(seed) + int(frame)) & 0xFFFFFFFF), pix)[..., None], np.arange(int(samples), dtype=U)[None, None, :])
    need = np.full(k.shape, TRIES + 1)
    for j in range(TRIES):
        c = [F(2.0) * rng_u01(k, U(3 * j + i)) - F(1.0) for i in range(3)]
        q = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        need = np.where((need > TRIES) & (q <= F(1.0)) & (q >= TINY), j + 1, need)
    return int(need.max())


def resolve(occluded, samples, rgb32f=None):
    """Step 8: occluded (...) counts -> {"ao" (...), "rgb32f" (..., 3)}."""
    occluded = np.asarray(occluded)
    ao = ((int(samples) - occluded).astype(F) / F(int(samples))).astype(F)
    if rgb32f is None:
        rgb = np.repeat(ao[..., None], 3, axis=-1)
    else:
        rgb = (ao[..., None] * np.asarray(rgb32f, F)).astype(F)
    return {"ao": ao, "rgb32f": np.ascontiguousarray(rgb, F)}


def counts(answers, valid, samples):
    """Per-pixel occluded counts from the answers (H * W * samples,) of the queries, pixels without a query counting 0."""
    a = np.asarray(answers).reshape(valid.shape + (int(samples),)).astype(np.int32)
    return np.where(valid.astype(bool), a.sum(axis=-1), 0).astype(np.int32)
