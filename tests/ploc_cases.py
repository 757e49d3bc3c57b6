"""Build primitives for the builder-2 tests (tests/ploc_reference.py, csrc/bvh_ploc.hip): each case is the smallest shape
at which one mechanism of the clustering rounds can break.  Every case returns (lo, hi) [n, 3] float32."""
import numpy as np

F32 = np.float32


def boxes(c, h):
    c, h = np.asarray(c, F32), np.asarray(h, F32)
    return c - h, c + h


def uniform(n, seed):
    rng = np.random.default_rng(seed)
    return boxes(rng.uniform(-1, 1, (n, 3)), rng.uniform(0.01, 0.3, (n, 3)))


def concentric(n=130):
    """Cubes [-h, h]^3 with h growing by a fifth: every centroid is +0, every key equal, the sort keeps the input order and
    leaf k is cube 2k + 1.  The union of two leaves is the larger, so d(i, j) = area(max(i, j)): slot 0 and slot 1 choose
    each other, every other slot chooses the lowest slot in reach, and a round merges exactly once -- L - 1 rounds, a chain
    L - 1 deep."""
    h = (0.01 * 1.2 ** np.arange(n)).astype(F32)
    h3 = np.repeat(h[:, None], 3, 1)
    return -h3, h3.copy()


def lattice(side=40):
    """side x side equal boxes on a unit lattice in the plane z = 0 (all dyadic): distances tie by the dozen, so nn is
    decided by the lowest-j rule."""
    x, y = np.meshgrid(np.arange(side), np.arange(side))
    c = np.stack([x.ravel(), y.ravel(), np.zeros(side * side)], 1)
    return boxes(c, np.full((side * side, 3), 0.25))


def clusters_and_floor(seed=3):
    """Two dense clusters of 600 small boxes and one floor box under both: 1 201 primitives.  Morton order puts the floor into
    a leaf between cluster boxes, and every ancestor of that leaf covers the floor."""
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.uniform(-0.5, 0.5, (600, 3)) + (-3.0, 0.0, 1.0), rng.uniform(-0.5, 0.5, (600, 3)) + (3.0, 0.5, 1.0)])
    lo, hi = boxes(c, rng.uniform(0.01, 0.03, (1200, 3)))
    floor_lo, floor_hi = np.array([[-6.5, -6.5, -0.05]], F32), np.array([[6.5, 6.5, 0.0]], F32)
    at = 600                                            # scene order: between the clusters
    return np.concatenate([lo[:at], floor_lo, lo[at:]]), np.concatenate([hi[:at], floor_hi, hi[at:]])


def growing_chain(n):
    """Cubes on the x axis, centre 1.1^k and half-size 0.05 * 1.1^k: each is nearest to its smaller neighbour, so only the
    low end of the array merges and the rounds run out for a long enough chain."""
    k = np.arange(n)
    c = np.zeros((n, 3))
    c[:, 0] = 1.1 ** k
    return boxes(c, np.repeat((0.05 * 1.1 ** k)[:, None], 3, 1))


def default_refs(n):
    return np.arange(n, dtype=np.uint32) * np.uint32(2654435761)          # distinct (an odd multiplier), unordered


PROBE_CASES = {
    "uniform_4": lambda: uniform(4, 104), "uniform_5": lambda: uniform(5, 105), "uniform_7": lambda: uniform(7, 107),
    "concentric_130": concentric,
    "uniform_1042": lambda: uniform(1042, 1142),      # L = 521: three workgroups, both inner edges, both clamped ends
    "lattice_40x40": lattice,
    "clusters_and_floor_1201": clusters_and_floor,
    "chain_192": lambda: growing_chain(192),
    "chain_200": lambda: growing_chain(200),
}


def write_chain_scene(path, n=200, seed=13):
    """growing_chain(n) as spheres (scene_gen's camera, lights, materials and floor plane): builder 2 gives up on it."""
    from scene_gen import write_scene
    from scene_motion import rewrite_p3f
    tmp = path + ".src"
    write_scene(tmp, np.random.default_rng(seed), n, 0, 0, 1, 2, 2)

    def move(cmd, k, vals):
        if cmd != "s":
            return None
        return np.array([1.1 ** (k - 1), 0.0, 0.0, 0.05 * 1.1 ** (k - 1)])          # (primitive 0 is the floor plane)
    rewrite_p3f(tmp, path, move)
    return path
