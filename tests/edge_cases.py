"""The edge-case battery (not a test module): rays and primitives OFF general position, stated once.

tests/golden/make_edge_vectors.py records what the reference's object code answers for it, tests/test_edge_vectors.py pins the
oracle to those answers and checks that the battery keeps its properties, tests/test_gpu_edge_rays.py runs it on the device.
Plain numpy, no randomness: every value is written down or derived from the grid's box by float32 arithmetic.

  pairs()                     (type, prim12, origin, dir) for the four intersectors
  write_edge_lattice(path)    a .p3f scene whose coordinates are all dyadic
  ray_families(grid)          named sets of rays on that scene, placed from the grid's box and dimensions
  undefined_in_grid(...)      the ONE exclusion rule, on the inputs alone
"""
import hashlib
import itertools

import numpy as np

F = np.float32
EPS = F(0.001)                                   # RT/macros.h:1
FLT_MAX = F(3.402823466e+38)
SPHERE, TRIANGLE, BOX, PLANE = 0, 1, 2, 3
TYPE_NAMES = ("sphere", "triangle", "box", "plane")
FAMILIES = ("axis", "diagonal", "outside", "on_surface", "ties", "scale", "nonfinite")
GRID_FAMILIES = tuple(f for f in FAMILIES if f != "nonfinite")
# nonfinite is left out of GRID mode as a family: Grid::Init_Traverse converts (p - min) * n / (max - min) of such a ray to
# int (RT/grid.cpp:178-186), which C++ leaves undefined for NaN.


def f32(*v):
    return np.array(v, F)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def digest(*arrays):
    """sha256 over shape, dtype and bytes of the arrays: what the fixture stores in place of the inputs."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s %s|" % (a.shape, a.dtype.str)).encode() + a.tobytes())
    return np.frombuffer(h.digest(), np.uint8)


# ------------------------------------------------------------------ intersector pairs
PRODUCT_COMPONENTS = f32(0.0, -0.0, 1.0, -1.0, 1e-30, 1e30, 1e-40, 0.5)         # 1e-40 is subnormal
PRODUCT_ORIGINS = f32((0, 0, 0), (0, 0, -2), (1, -2, 0), (0.5, 0.5, 0.5), (-1, -1, -1), (1, 0, 0), (0.25, -0.5, 3),
                      (2, 2, 2), (0, 1, 0), (-0.5, 0, 0.5))
UNIT_TRI = (0, 0, 0, 1, 0, 0, 0, 1, 0)           # e1 = x, e2 = y: det = -d.z exactly, u = o.x, v = o.y for a ray along z
PRODUCT_PRIMS = (
    (SPHERE, (0, 0, 0, 1)), (SPHERE, (0.5, 0.5, 0.5, 0.5)), (SPHERE, (0, 0, 0, 0)),
    (TRIANGLE, UNIT_TRI), (TRIANGLE, (-1, -1, 1, 1, -1, 1, 0, 1, 1)),
    (BOX, (-1, -1, -1, 1, 1, 1)), (BOX, (0, 0, 0, 1, 1, 1)), (BOX, (-1, -1, 0.5, 1, 1, 0.5)),
    (PLANE, (0, 0, 0, 1, 0, 0, 0, 1, 0)),        # three points, as the loader has them: z = 0, normal +z
)
SIGNED_ZERO_ONE = f32(0.0, -0.0, 1.0, -1.0)


def _extra_pairs():
    out = []

    def add(kind, prim, o, d):
        out.append((kind, tuple(prim), tuple(o), tuple(d)))

    # sphere: tangent rays (discriminant exactly 0: b * b == 4 * a * c == 16), origin on the surface and inside, radius 0,
    # a zero direction
    for perm in itertools.permutations(range(3)):
        o, d = np.zeros(3, F), np.zeros(3, F)
        o[perm[0]], o[perm[1]], d[perm[1]] = 1, -2, 1
        add(SPHERE, (0, 0, 0, 1), o, d)
        add(SPHERE, (0, 0, 0, 1), -o, -d)
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, -1), (0.5, 0.5, 0), (0, 0, 0), (-0.0, 0, 0)):
        add(SPHERE, (0, 0, 0, 1), (1, 0, 0), d)                  # on the surface
        add(SPHERE, (0, 0, 0, 1), (0, 0, 0), d)                  # at the centre
        add(SPHERE, (0, 0, 0, 1), (0.25, -0.5, 0.5), d)          # inside
        add(SPHERE, (0, 0, 0, 1), (0, 3, 0), d)                  # outside
        add(SPHERE, (0.5, 0.25, -1, 0), (0.5, 0.25, 1), d)       # radius 0
        add(SPHERE, (0.5, 0.25, -1, 0), (0.5, 0.25, -1), d)
    add(SPHERE, (0.5, 0.25, -1, 0), (0.5, 0.25, 1), (0, 0, -1))  # through the point that is the sphere

    # triangle: through the vertices, through the edges, along an edge, in its plane (u, v, u + v exactly 0 or 1)
    for x, y in ((0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.25), (1, 1), (-0.25, 0.5), (0.75, 0.5)):
        add(TRIANGLE, UNIT_TRI, (x, y, 1), (0, 0, -1))
        add(TRIANGLE, UNIT_TRI, (x, y, -2), (0, 0, 0.5))
        add(TRIANGLE, UNIT_TRI, (x, y, 0), (0, 0, -1))           # origin on it: t == 0
    for o, d in (((-1, 0, 0), (1, 0, 0)), ((0, -1, 0), (0, 1, 0)), ((2, -1, 0), (-1, 1, 0)), ((0.25, 0.25, 0), (1, 0, 0)),
                 ((0.25, 0.25, 0), (0, 0, 0)), ((-1, 0, 1), (1, 0, -1)), ((0, 0, 1), (1, 0, -1))):
        add(TRIANGLE, UNIT_TRI, o, d)
    # det = -d.z: at +-EPS and one ulp either side (the test is det > -EPS && det < EPS), subnormal, zero, and where frcp()
    # leaves its plain path (|det| >= 2^126); origins chosen so that the accepted ones give t = 2^-6 or 1
    dets = [EPS, up(EPS), down(EPS), -EPS, up(-EPS), down(-EPS), F(1e-40), F(-1e-40), F(0.0), F(-0.0), F(2.0 ** -126),
            down(F(2.0 ** -126)), F(2.0 ** 126), down(F(2.0 ** 126)), F(-2.0 ** 126), F(2.0 ** 127), F(-2.0 ** 127), F(1.0), F(-1.0), F(0.5)]
    for det in dets:
        dz = -det
        for t in (F(2.0 ** -6), F(1.0)):
            add(TRIANGLE, UNIT_TRI, (0.25, 0.25, -dz * t), (0, 0, dz))
        add(TRIANGLE, UNIT_TRI, (0.25, 0.25, 1 if dz < 0 else -1), (0.5, 0, dz))
    # t exactly at EPS and one ulp either side: a triangle accepts t > EPS, a box enters at tIn > EPS and needs tOut > EPS
    for tz in (EPS, up(EPS), down(EPS)):
        add(TRIANGLE, UNIT_TRI, (0.25, 0.25, tz), (0, 0, -1))
        add(TRIANGLE, UNIT_TRI, (0.25, 0.25, -tz), (0, 0, 1))
        add(BOX, (0, 0, 0, 1, 1, 1), (0.5, 0.5, -tz), (0, 0, 1))
        add(BOX, (0, 0, -1, 1, 1, 0), (0.5, 0.5, -tz), (0, 0, 1))
    # zero-area triangles
    for o, d in (((0.25, 0, 1), (0, 0, -1)), ((0, 0, 1), (0, 0, -1)), ((0.5, 0, 0), (0, 0, 0))):
        add(TRIANGLE, (0, 0, 0, 0, 0, 0, 1, 0, 0), o, d)
        add(TRIANGLE, (0, 0, 0, 1, 0, 0, 2, 0, 0), o, d)
        add(TRIANGLE, (0, 0, 0, 0, 0, 0, 0, 0, 0), o, d)

    # box: origin on a face, an edge, a corner, inside and outside; every direction of {+0, -0, 1, -1}^3 -- a zero
    # component while the origin lies on that slab's plane is 0 * inf
    dirs = list(itertools.product(SIGNED_ZERO_ONE, repeat=3))
    for box in ((0, 0, 0, 1, 1, 1), (0, 0, 0.5, 1, 1, 0.5)):                     # the second is flat: mn == mx in z
        for o in ((0, 0.5, 0.5), (0, 0, 0.5), (0, 0, 0), (1, 1, 1), (0.5, 0.5, 0.5), (0.5, 0.5, 1), (0.5, 0.5, -1), (1, 0.5, 2)):
            for d in dirs:
                add(BOX, box, o, d)

    # plane z = 0: direction parallel to it, origin in it, denominators at +-EPS and one ulp either side
    # (fabs(denominator) < EPS rejects)
    plane = PRODUCT_PRIMS[-1][1]
    for o in ((0, 0, 1), (0, 0, -1), (0, 0, 0), (0.25, -3, 0.5)):
        for dz in (EPS, up(EPS), down(EPS), -EPS, up(-EPS), down(-EPS), F(0.0), F(-0.0), F(1.0), F(-1.0), F(1e-40)):
            add(PLANE, plane, o, (0, 0, dz))
            add(PLANE, plane, o, (1, 1, dz))
    return out


_pairs = None


def pairs():
    """(type [n] uint32, prim12 [n, 12] in loader form, origin [n, 3], dir [n, 3]).  The product of PRODUCT_COMPONENTS^3
    directions, PRODUCT_ORIGINS and PRODUCT_PRIMS with the primitive innermost, and the written-down cases spread evenly
    through it: every wave of 64 pairs mixes the primitive kinds, and the triangle lanes of a wave mix determinants that
    take frcp()'s plain path with ones that do not."""
    global _pairs
    if _pairs is None:
        prod = [(k, p, tuple(o), d) for d in itertools.product(PRODUCT_COMPONENTS, repeat=3) for o in PRODUCT_ORIGINS
                for k, p in PRODUCT_PRIMS]
        extra = _extra_pairs()
        # one written-down case after every `gap` product pairs, taken with a stride coprime to their number
        gap = len(prod) // len(extra)
        assert gap >= 8
        stride = 389
        assert np.gcd(stride, len(extra)) == 1
        rows = []
        for i, e in enumerate(prod):
            rows.append(e)
            if i % gap == gap - 1 and i // gap < len(extra):
                rows.append(extra[(i // gap) * stride % len(extra)])
        assert len(rows) == len(prod) + len(extra)
        n = len(rows)
        kind = np.array([r[0] for r in rows], np.uint32)
        prim = np.zeros((n, 12), F)
        for i, r in enumerate(rows):
            prim[i, :len(r[1])] = r[1]
        o = np.array([r[2] for r in rows], F)
        d = np.array([r[3] for r in rows], F)
        for a in (kind, prim, o, d):
            a.setflags(write=False)
        _pairs = (kind, prim, o, d)
    return _pairs


def device_prims(kind, prim12):
    """prim12 as p3d_debug_intersect takes it: a plane is (unit normal, D) there.  The battery's planes have a cross product
    that is a signed axis vector, so Plane::Plane's normalize() and D = -(PN * P0) (RT/scene.cpp:94-113) are exact."""
    out = np.array(prim12, F)
    for i in np.flatnonzero(np.asarray(kind) == PLANE):
        p = np.asarray(prim12[i][:9], F).reshape(3, 3)
        n = np.cross(p[1] - p[0], p[2] - p[0]).astype(F)
        assert sorted(np.abs(n)) == [0, 0, 1], "a plane of the battery must have an axis-parallel unit cross product"
        out[i] = 0
        out[i, :3] = n
        out[i, 3] = -F(n @ p[0])
    return out


# ------------------------------------------------------------------ the scene
LATTICE_XY = (-1.5, -0.5, 0.5, 1.5)
LATTICE_Z = (0.0, 1.0)
LATTICE_R = 0.25
BOX_A, BOX_B = (2, -1, -0.5, 3, 0, 0.5), (3, -1, -0.5, 4, 0, 0.5)              # share the face x == 3
BOX_C, SPHERE_IN_C = (2, 1, -0.5, 3.5, 2.5, 1), (2.75, 1.75, 0.25, 0.5)
PLANE_Z = -0.75
QUAD_Z = 2.0
DIFFUSE = "f 0.75 0.5 0.25 0.75 1 1 1 0.25 32 0 1"
MIRROR = "f 0.5 0.5 0.75 0.25 1 1 1 0.75 64 0 1"
GLASS = "f 0.75 0.75 1 0.125 1 1 1 0.25 64 1 1.5"


def quads():
    """Each quad as two triangles that share the diagonal p0 - p2: (p0, p1, p2), (p0, p2, p3)."""
    q = []
    for i in range(4):                                            # axis-aligned, z == QUAD_Z, side 1
        for j in range(2):
            x, y = -2.0 + i, -1.0 + j
            q.append(((x, y, QUAD_Z), (x + 1, y, QUAD_Z), (x + 1, y + 1, QUAD_Z), (x, y + 1, QUAD_Z)))
    for i in range(4):                                            # tilted: z rises by 1 over y
        x = -2.0 + i
        q.append(((x, 1.5, 2.5), (x + 1, 1.5, 2.5), (x + 1, 2.5, 3.5), (x, 2.5, 3.5)))
    for i in range(4):                                            # upright, in the plane y == -2
        x = -2.0 + i
        q.append(((x, -2, 0), (x + 1, -2, 0), (x + 1, -2, 1), (x, -2, 1)))
    return q


def num(v):
    """A float32 as text that parses back to it (the shortest repr of the double it equals)."""
    return repr(float(F(v)))


def write_edge_lattice(path, eye=(0.5, 0.25, 8.0), at=(0.5, 0.25, 0.0), res=(65, 33)):
    """69 primitives in scene order: the plane, 32 lattice spheres (one glass, one mirror), boxes A and B sharing a face,
    box C with a sphere inside, 16 quads = 32 triangles.  Every coordinate is dyadic."""
    L = ["accel 2", "spp 0", "bclr 0.125 0.25 0.5", "v", "from %s %s %s" % tuple(num(v) for v in eye),
         "at %s %s %s" % tuple(num(v) for v in at), "up 0 1 0", "angle 40", "hither 0.0078125", "resolution %d %d" % res,
         "aperture 0", "focal 1", "l 3 4 8 1 1 1", "l -2.5 0.25 6 0.5 0.5 0.5"]
    L += [DIFFUSE, "pl 8 8 %s -8 8 %s -8 -8 %s" % ((num(PLANE_Z),) * 3)]
    k = 0
    for z in LATTICE_Z:
        for y in LATTICE_XY:
            for x in LATTICE_XY:
                L.append(GLASS if k == 5 else MIRROR if k == 10 else DIFFUSE)
                L.append("s %s %s %s %s" % (num(x), num(y), num(z), num(LATTICE_R)))
                k += 1
    L.append(DIFFUSE)
    for b in (BOX_A, BOX_B, BOX_C):
        L.append("box " + " ".join(num(v) for v in b))
    L.append("s " + " ".join(num(v) for v in SPHERE_IN_C))
    for p0, p1, p2, p3 in quads():
        for tri in ((p0, p1, p2), (p0, p2, p3)):
            L.append("p 3\n" + "\n".join(" ".join(num(v) for v in p) for p in tri))
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")
    return path


# ------------------------------------------------------------------ the grid, as far as placing rays needs it
def cell_plane(grid, axis, k):
    """The float32 coordinate of the grid's k-th cell plane on `axis` as the reference's own cell formula sees it: the
    SMALLEST float v for which (v - min) * n / (max - min), in float (RT/grid.cpp:178), reaches k -- the first coordinate
    that belongs to cell k (the box's faces for k == 0 and k == n)."""
    x0, x1, n = F(grid["mn"][axis]), F(grid["mx"][axis]), int(grid["dims"][axis])
    if k == 0:
        return x0
    if k == n:
        return x1
    reaches = lambda c: F(F(c - x0) * F(n)) / F(x1 - x0) >= F(k)
    v = F(x0 + F(k) * F(x1 - x0) / F(n))
    for _ in range(64):
        if reaches(v) and not reaches(down(v)):
            return v
        v = down(v) if reaches(v) else up(v)
    raise AssertionError("no float found on cell plane %d of axis %d" % (k, axis))


def grid_entry(o, d, grid):
    """Grid::Init_Traverse (RT/grid.cpp:101-245) in numpy, float for float, for rays o, d [n, 3]: dict of `enters` (the ray
    is not rejected at :171), `p` (the point whose cell is taken, :178-186) and `next` (tx_next, ty_next, tz_next)."""
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    mn, mx, dims = np.asarray(grid["mn"], F), np.asarray(grid["mx"], F), np.asarray(grid["dims"], np.int64)
    with np.errstate(all="ignore"):
        inv = (np.float64(1.0) / d.astype(np.float64)).astype(F)
        lo, hi = (mn - o) * inv, (mx - o) * inv
        pos = inv >= 0
        tmin, tmax = np.where(pos, lo, hi), np.where(pos, hi, lo)
        t0 = np.where(tmin[:, 0] > tmin[:, 1], tmin[:, 0], tmin[:, 1])
        t0 = np.where(tmin[:, 2] > t0, tmin[:, 2], t0)
        t1 = np.where(tmax[:, 0] < tmax[:, 1], tmax[:, 0], tmax[:, 1])
        t1 = np.where(tmax[:, 2] < t1, tmax[:, 2], t1)
        enters = ~((t0 > t1) | (t1 < 0))
        inside = ((o > mn) & (o < mx)).all(1)                                   # AABB::isInside is strict
        p = np.where(inside[:, None], o, o + d * t0[:, None]).astype(F)
        cell_f = ((p - mn) * dims.astype(F) / (mx - mn)).astype(F)
        cell = np.clip(np.nan_to_num(cell_f, nan=0.0).astype(np.float64), 0, (dims - 1).astype(np.float64)).astype(np.int64)
        dt = ((tmax - tmin) / dims.astype(F)).astype(np.float64)
        nxt = np.where(d > 0, tmin.astype(np.float64) + (cell + 1) * dt, tmin.astype(np.float64) + (dims - cell) * dt)
        nxt = np.where(d == 0, np.float64(FLT_MAX), nxt)
    return {"enters": enters, "inside": inside, "p": p, "cell_f": cell_f, "next": nxt}


UNDEFINED_IN_GRID = ("the cell coordinate (p - min) * n / (max - min) of the ray's entry point is NaN, for the direction as given "
                     "(closest hit) or normalised (shadow query, RT/grid.cpp:313-316), and Grid::Init_Traverse converts it to int "
                     "(RT/grid.cpp:178-186): undefined in C++")


def normalized(d):
    """Vector::normalize (RT/vector.cpp:9-12, 66-71) in float: l = 1 / sqrt(x * x + y * y + z * z), then three products."""
    d = np.asarray(d, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(F)
        l = (np.float64(1.0) / np.sqrt(s, dtype=F).astype(np.float64)).astype(F)
        return (d * l[:, None]).astype(F)


def undefined_in_grid(o, d, grid):
    """[n] bool, from the inputs alone: rays whose first cell RT/grid.cpp:178-186 takes from a NaN, as a closest-hit ray or as
    the shadow ray of the same origin and direction.  Only GRID mode leaves them out."""
    bad = np.zeros(len(o), bool)
    for dd in (d, normalized(d)):
        e = grid_entry(o, dd, grid)
        bad |= e["enters"] & np.isnan(e["cell_f"]).any(1)
    return bad


def dda_ties(o, d, grid):
    """[n] int: how many of tx_next, ty_next, tz_next tie for the smallest when the walk starts (0 where the ray is rejected)."""
    e = grid_entry(o, d, grid)
    nxt = e["next"]
    with np.errstate(all="ignore"):
        ties = (nxt == np.nanmin(np.where(np.isnan(nxt), np.inf, nxt), axis=1)[:, None]).sum(1)
    return np.where(e["enters"], ties, 0)


# ------------------------------------------------------------------ ray families
def _axis_dirs():
    d = []
    for a in range(3):                                            # two zero components, both signs of each
        for s in (1.0, -1.0):
            for z1, z2 in itertools.product((0.0, -0.0), repeat=2):
                v = [z1, z2]
                v.insert(a, s)
                d.append(v)
    for a in range(3):                                            # one zero component
        for z in (0.0, -0.0):
            for s1, s2 in itertools.product((1.0, -1.0), repeat=2):
                v = [s1, s2]
                v.insert(a, z)
                d.append(v)
    return np.array(d, F)


def _diagonal_dirs(grid):
    d = [v for v in itertools.product((1.0, -1.0), repeat=3)]
    for a in range(3):
        for z in (0.0, -0.0):
            for s1, s2 in itertools.product((1.0, -1.0), repeat=2):
                v = [s1, s2]
                v.insert(a, z)
                d.append(tuple(v))
    d = np.array(d, F)
    # the same directions along the CELL's diagonals: the three planes of a cell corner are then reached together
    w = ((np.asarray(grid["mx"], F) - np.asarray(grid["mn"], F)) / np.asarray(grid["dims"], F)).astype(F)
    return np.concatenate([d, (d * w).astype(F)])


def _cross(origins, dirs):
    o = np.repeat(np.asarray(origins, F), len(dirs), axis=0)
    d = np.tile(np.asarray(dirs, F), (len(origins), 1))
    return o, d


def ray_families(grid):
    """{family: (origin [n, 3], dir [n, 3])} float32, read-only, placed from the grid's box `mn`, `mx` and `dims`."""
    mn, mx, dims = np.asarray(grid["mn"], F), np.asarray(grid["mx"], F), np.asarray(grid["dims"], np.int64)
    assert (dims >= 3).all(), "the families place origins on interior cell planes"
    cp = lambda axis, k: cell_plane(grid, axis, k)
    mid = (mn + (mx - mn) * F(0.3125)).astype(F)                  # inside, on no cell plane
    pk = [max(1, int(dims[a]) // 2) for a in range(3)]
    on = f32(cp(0, pk[0]), cp(1, pk[1]), cp(2, pk[2]))           # an interior cell corner
    axis_origins = f32(
        mid, (on[0], mid[1], mid[2]), (on[0], on[1], mid[2]), on, (mid[0], mid[1], on[2]),
        (mn[0], mid[1], mid[2]), (mx[0], mid[1], mid[2]), (mn[0], mn[1], mid[2]), mn, mx,             # face, edge, corners
        (mn[0] - 1, mn[1], mid[2]), (mid[0], mn[1] - 1, mx[2]), (mn[0] - 1, mid[1], mid[2]),          # outside, along a face
        (-3, -0.5, 0), (0.5, 0.5, 5), (-1.5, -3, 1), (2.5, -0.5, 0), (2.75, 1.75, 0.25))               # through centres
    fam = {"axis": _cross(axis_origins, _axis_dirs())}

    corners = [on, mn, mx]
    for i, j, k in ((1, 1, 1), (1, 2, 1), (2, 1, 2), (0, 1, 1), (1, 0, 2)):
        corners.append(f32(cp(0, min(i, dims[0])), cp(1, min(j, dims[1])), cp(2, min(k, dims[2]))))
    corners += [f32(-1.5, -1.5, 0), f32(0.5, 0.5, 1), f32(-4, -4, -2.5), f32(0, 0, 2)]
    fam["diagonal"] = _cross(corners, _diagonal_dirs(grid))

    # rays that miss the grid's box: pointing away from it, passing beside it, parallel to a face outside it
    o, d = [], []
    for a in range(3):
        for side in (0, 1):
            base = mid.copy()
            base[a] = (mx[a] + 1) if side else (mn[a] - 1)
            away = np.zeros(3, F)
            away[a] = 1 if side else -1
            beside = np.ones(3, F)                                # parallel to that face: the component across it is +-0
            beside[a] = -0.0 if side else 0.0
            for v in (away, away + f32(0.5, 0.25, 0.125), np.roll(f32(0, 1, 0), a), np.roll(f32(0, 1, -1), a), beside, -beside):
                o.append(base)
                d.append(v)
    for v in ((1, 1, 1), (1, 0, 0), (0, 0, 0), (1, -1, 0.5)):
        o.append(mx + 2)
        d.append(f32(*v))
    fam["outside"] = (np.array(o, F), np.array(d, F))

    # origins exactly on a surface, leaving along +-normal and tangentially
    o, d = [], []
    c = f32(-1.5, -1.5, 0)
    for a in range(3):
        for s in (1, -1):
            nrm = np.zeros(3, F)
            nrm[a] = s
            p = c + nrm * F(LATTICE_R)
            for v in (nrm, -nrm, np.roll(nrm, 1), np.roll(nrm, 2) + nrm):
                o.append(p)
                d.append(v)
    for p, nrm, tan in ((f32(-1.25, -0.75, QUAD_Z), f32(0, 0, 1), f32(1, 0, 0)),       # inside a triangle of a quad
                        (f32(-1.5, -0.5, QUAD_Z), f32(0, 0, 1), f32(1, 1, 0)),         # on the shared diagonal, along it
                        (f32(-2, -1, QUAD_Z), f32(0, 0, 1), f32(1, 0, 0)),             # on a vertex, along an edge
                        (f32(2, -0.5, 0), f32(-1, 0, 0), f32(0, 1, 0)),                # box A's face x == 2
                        (f32(3, -0.5, 0), f32(1, 0, 0), f32(0, 0, 1)),                 # the face A and B share
                        (f32(2, -1, -0.5), f32(-1, -1, -1), f32(0, 0, 1)),             # a corner of box A
                        (f32(2.75, 1.75, 0.75), f32(0, 0, 1), f32(1, 0, 0)),           # the sphere inside box C
                        (f32(0.25, 0.25, PLANE_Z), f32(0, 0, 1), f32(1, 0, 0)),        # the plane, inside its [-1, 1]^3 box
                        (f32(3.25, -3, PLANE_Z), f32(0, 0, 1), f32(0, 1, 0))):         # the plane, outside that box
        for v in (nrm, -nrm, tan, -tan, tan + nrm * F(0.5)):
            o.append(p)
            d.append(v)
    for li in (f32(3, 4, 8), f32(-2.5, 0.25, 6)):                # from a light, and a zero direction on a surface
        o.append(li)
        d.append(f32(-1.5, -1.5, 0.25) - li)
    o.append(f32(-1.5, -1.5, 0.25))
    d.append(f32(0, 0, 0))
    fam["on_surface"] = (np.array(o, F), np.array(d, F))

    # equal t on two primitives: the shared diagonal of a quad, the face two boxes share; tangent points of lattice spheres
    o, d = [], []
    for x, y in ((-1.5, -0.5), (-1.75, -0.75), (-0.5, 0.5), (1.25, -0.75), (0, 0), (-1, 0), (0.5, 0.5)):
        for z, dz in ((5, -1), (-0.5, 1), (QUAD_Z + 0.5, -0.5)):
            o.append(f32(x, y, z))
            d.append(f32(0, 0, dz))
    for x in (-1.5, -0.5, 0.5):                                   # the tilted quads' diagonals, from straight above
        o.append(f32(x, 2, 6))
        d.append(f32(0, 0, -1))
    for p, v in (((2.5, -0.5, 0), (1, 0, 0)), ((3.5, -0.5, 0), (-1, 0, 0)), ((3, -2, 0), (0, 1, 0)), ((3, -0.5, 2), (0, 0, -1)),
                 ((2.5, -0.75, 0.25), (0.5, 0, 0)), ((3.75, -0.25, -0.25), (-2, 0, 0)), ((3, -1, -0.5), (0, 1, 1)),
                 ((5, -0.5, 0), (-1, 0, 0)), ((2.5, -0.5, 0), (1, 0.5, 0)), ((3, 0.5, 0), (0, -1, 0)),
                 # the same lines leaving the scene: misses
                 ((5, -0.5, 0), (1, 0, 0)), ((3, -2, 0), (0, -1, 0)), ((3, -0.5, 2), (0, 0, 1)), ((-1.5, -0.5, 5), (0, 0, 1)),
                 ((-1.25, 3, 1), (0, 1, 0)), ((3, 3, 3), (0, 0.5, 0.5))):
        o.append(f32(*p))
        d.append(f32(*v))
    for s in (LATTICE_R, -LATTICE_R):                             # tangent to a row of the lattice: discriminant exactly 0
        for p, v in (((-1.5 + s, -3, 0), (0, 1, 0)), ((-3, -1.5 + s, 0), (1, 0, 0)), ((-1.5 + s, -1.5, 4), (0, 0, -1)),
                     ((-1.5 + s, -3, 1), (0, 0.25, 0))):
            o.append(f32(*p))
            d.append(f32(*v))
    fam["ties"] = (np.array(o, F), np.array(d, F))

    # the axis and diagonal directions scaled far from 1, subnormal components included
    # (the length of such a direction under- or overflows, so the shadow query's normalised direction is 0, inf or NaN: from
    # an origin strictly inside the grid's box that is still defined, from the box's face or outside it mostly not -- the
    # origins are inside or on cell planes, and two others take the diagonal directions at one scale only)
    base_o = axis_origins[[0, 1, 3, 4]]
    base_d = np.concatenate([_axis_dirs(), _diagonal_dirs(grid)[:32]])
    o, d = [], []
    for s in (F(2.0 ** -100), F(2.0 ** 100), F(2.0 ** -140)):
        oo, dd = _cross(base_o, (base_d * s).astype(F))
        o.append(oo)
        d.append(dd)
    oo, dd = _cross(axis_origins[[5, 13]], (_diagonal_dirs(grid)[:32] * F(2.0 ** -100)).astype(F))
    o.append(oo)
    d.append(dd)
    # and at 2^40, where nothing under- or overflows: segments that long are occluded wherever they point at something, so the
    # family has both shadow answers in BVH and GRID mode too
    oo, dd = _cross(axis_origins[[0, 13]], (base_d * F(2.0 ** 40)).astype(F))
    o.append(oo)
    d.append(dd)
    fam["scale"] = (np.concatenate(o), np.concatenate(d))

    # NaN and +-inf in one component of the origin or the direction (BVH and NONE only)
    o, d = [], []
    for bo, bd in ((f32(-3, -0.5, 0), f32(1, 0, 0)), (f32(0.5, 0.5, 5), f32(0, 0, -1)), (mid, f32(1, 1, 1)),
                   (f32(2.5, -0.5, 0), f32(1, 0, 0)), (f32(-1.25, -0.75, 5), f32(0.25, 0.125, -1)), (f32(0, 0, 0), f32(0, 1, 0))):
        for bad in (F(np.nan), F(np.inf), F(-np.inf)):
            for comp in range(3):
                for which in (0, 1):
                    oo, dd = bo.copy(), bd.copy()
                    (oo if which == 0 else dd)[comp] = bad
                    o.append(oo)
                    d.append(dd)
    fam["nonfinite"] = (np.array(o, F), np.array(d, F))

    assert tuple(fam) == FAMILIES
    for k in fam:
        o, d = (np.ascontiguousarray(a, F) for a in fam[k])
        assert o.shape == d.shape and o.shape[1] == 3
        o.setflags(write=False)
        d.setflags(write=False)
        fam[k] = (o, d)
    return fam


def battery(grid):
    """All families in FAMILIES order as one stream: (origin, dir, {family: slice})."""
    fam = ray_families(grid)
    at, where = 0, {}
    for k in FAMILIES:
        where[k] = slice(at, at + len(fam[k][0]))
        at += len(fam[k][0])
    o = np.concatenate([fam[k][0] for k in FAMILIES])
    d = np.concatenate([fam[k][1] for k in FAMILIES])
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d, where


def mode_mask(o, d, where, grid, accel):
    """[n] bool: the rays of the battery that run in `accel`; every one is left out by a rule on the inputs (printed by the
    tests with its count).  Accel 0 and 2 run everything."""
    keep = np.ones(len(o), bool)
    if accel == 1:
        keep[where["nonfinite"]] = False
        keep &= ~undefined_in_grid(o, d, grid)
    return keep


def exclusion_report(o, d, where, grid):
    """Lines for the tests to print, and the caps of the battery checked: apart from nonfinite in GRID mode, at most 5 % of
    the battery and at most a quarter of any family."""
    und = undefined_in_grid(o, d, grid)
    lines, total = [], 0
    for k in GRID_FAMILIES:
        n, x = where[k].stop - where[k].start, int(und[where[k]].sum())
        lines.append("family %-10s %5d rays, GRID excludes %d" % (k, n, x))
        assert 4 * x <= n, "more than a quarter of family %s is excluded" % k
        total += x
    n = where["nonfinite"].stop - where["nonfinite"].start
    lines.append("family %-10s %5d rays, GRID excludes all of them (family rule)" % ("nonfinite", n))
    n_grid = len(o) - n
    assert 20 * total <= n_grid, "more than 5 %% of the battery is excluded: %d of %d" % (total, n_grid)
    lines.append("excluded by rule in GRID mode: %d of %d; rule: %s" % (total, n_grid, UNDEFINED_IN_GRID))
    return lines
