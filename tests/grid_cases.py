"""Inputs of the device grid build's tests: boxes (lo, hi, ref) as p3d_debug_grid_build and p3dh_grid_dump take them."""
import numpy as np

F = np.float32
EPS = F(0.001)                     # EPSILON, RT/macros.h:1


def scene_boxes(ptype, data12):
    """GRID mode's box of every primitive of a flattened scene (HostScene.arrays()), with the float32 operations of
    csrc/grid_builder.h (grid_box_rule), and the description's references (kind << 30 | index within the kind)."""
    t = np.minimum(np.asarray(ptype, np.uint32), 3)
    d = np.ascontiguousarray(data12, F).reshape(-1, 12)
    n = len(t)
    lo, hi = np.full((n, 3), -1, F), np.full((n, 3), 1, F)          # planes
    s = t == 0
    lo[s], hi[s] = d[s, :3] - d[s, 3:4], d[s, :3] + d[s, 3:4]
    tr = t == 1
    pts = d[tr, :9].reshape(-1, 3, 3)
    lo[tr], hi[tr] = pts.min(1) - EPS, pts.max(1) + EPS
    b = t == 2
    lo[b], hi[b] = d[b, :3], d[b, 3:6]
    ref = np.zeros(n, np.uint32)
    for k in range(4):
        ref[t == k] = (k << 30) | np.arange(int((t == k).sum()), dtype=np.uint32)
    return lo, hi, ref


def empty():
    return np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, np.uint32)


def one_box():
    return np.array([[-0.5, 0.25, 1.0]], F), np.array([[0.75, 2.0, 1.5]], F), np.array([(2 << 30) | 7], np.uint32)


def spheres_on_a_line(n=65):
    """n unit spheres 1.5 apart: the primitives cross a wave of the device build, and n is no multiple of 64."""
    c = np.zeros((n, 3), F)
    c[:, 0] = np.arange(n, dtype=F) * F(1.5)
    return c - F(1), c + F(1), np.arange(n, dtype=np.uint32)


def identical_boxes(n=300):
    """Every item in the same cells: scene order inside a cell is all there is to get right."""
    lo, hi = np.tile(np.array([[0.1, -0.2, 0.3]], F), (n, 1)), np.tile(np.array([[1.3, 0.9, 0.8]], F), (n, 1))
    return lo, hi, ((2 << 30) | np.arange(n, dtype=np.uint32)[::-1]).astype(np.uint32)


def heavy(seed=3, n=200):
    """n small boxes, a box enclosing those, a [-1, 1]^3 far away, and last a box enclosing everything: a primitive that
    covers every cell of the grid (far more than one lane is given to write), long runs of cells that hold nothing else
    between the cluster and the far box, and upper corners that land in cell n - 1."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-4, 4, (n, 3)).astype(F)
    h = rng.uniform(0.02, 0.2, (n, 3)).astype(F)
    lo, hi = c - h, c + h
    lo = np.concatenate([lo, lo.min(0, keepdims=True), np.array([[39, 39, 39]], F)])
    hi = np.concatenate([hi, hi.max(0, keepdims=True), np.array([[41, 41, 41]], F)])
    lo, hi = np.concatenate([lo, lo.min(0, keepdims=True)]), np.concatenate([hi, hi.max(0, keepdims=True)])
    ref = np.arange(n + 3, dtype=np.uint32)
    ref[n] |= 2 << 30
    ref[n + 1] = 3 << 30
    ref[n + 2] |= 2 << 30
    return lo.astype(F), hi.astype(F), ref


def coplanar_triangles(seed=5, n=100):
    """n triangles in the plane z = 0.7: every box is 2 EPSILON thick there."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-3, 3, (n, 3, 3)).astype(F)
    pts[:, :, 2] = F(0.7)
    return (pts.min(1) - EPS).astype(F), (pts.max(1) + EPS).astype(F), ((1 << 30) | np.arange(n, dtype=np.uint32)).astype(np.uint32)
