"""Small sphere scenes whose centroids are degenerate for a Morton-code builder (csrc/bvh_device.hip): written with
scene_gen.write_scene (camera, lights, materials, a floor plane) and scene_motion.rewrite_p3f (the spheres put where the
case wants them).  Each has 64 to 128 spheres, so p3d_scene_create lets the device builder run, and is small enough to be
served from LDS."""
import numpy as np

from scene_gen import write_scene
from scene_motion import rewrite_p3f

N_SPHERES = 96


def geometric_sphere(m):
    """Sphere m of the geometric-series scene: on axis m % 3 at 1.5 * 2^-(m // 3), zero on the other two.  The builder's
    21-bit cell on that axis is then a single bit that moves down one place every three spheres, so the sorted 63-bit keys
    leave one leaf per level: a chain.  Past 2^-21 of the extent the spheres share cell 0 and only the index separates them."""
    v = np.zeros(4)
    v[m % 3] = 1.5 * 2.0 ** -(m // 3)
    v[3] = max(0.3 * v[m % 3], 0.004)
    return v


def _place(kind):
    def move(cmd, k, vals):
        if cmd != "s":
            return None
        if kind == "geometric":
            return geometric_sphere(k - 1)                       # (primitive 0 is the floor plane)
        if kind == "concentric":                                 # one centre, growing radii: every key is equal
            return np.array([0.0, 0.0, 0.0, 0.2 + 0.01 * (k - 1)])
        if kind == "coplanar":                                   # centres in the plane z = 0: no extent on one axis
            return np.array([vals[0], vals[1], 0.0, 0.5 * vals[3]])
        return None                                              # uniform: write_scene's own random spheres
    return move


KINDS = ("geometric", "concentric", "coplanar", "uniform")


def write_lbvh_scene(path, kind, seed=11):
    assert kind in KINDS
    tmp = path + ".src"
    write_scene(tmp, np.random.default_rng(seed), N_SPHERES, 0, 0, 1, 2, 2)
    rewrite_p3f(tmp, path, _place(kind))
    return path
