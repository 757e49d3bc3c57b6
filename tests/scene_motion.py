"""Moving scenes for the p3d_scene_update tests: a .p3f file rewritten with moved geometry (same primitives, same order,
same materials), the bounding boxes the tests' preconditions are stated on, and a generated scene too large for LDS."""
import numpy as np

# tokens that follow each command of the .p3f grammar (csrc/host/p3d_scene.cpp: Scene::load_p3f); "p" is "p 3" + 9
ARITY = {"accel": 1, "spp": 1, "f": 11, "bclr": 3, "env": 1, "v": 23, "s": 4, "box": 6, "pl": 9, "l": 6}


def rewrite_p3f(src, dst, move):
    """Copy scene file src to dst with geometry replaced: move(kind, k, values) -> values, where kind is "s" (x y z r),
    "box" (min max), "p" (three points), "pl" (three points) with k the primitive's scene index, or "l" (position,
    colour) with k the light's index.  Returning None keeps the values."""
    tokens = []
    for line in open(src).read().splitlines():
        line = line.split("#")[0]
        tokens += line.split()
    out, i, n_prim, n_light = [], 0, 0, 0
    while i < len(tokens):
        cmd = tokens[i]
        if cmd == "p":
            assert tokens[i + 1] == "3"
            head, n = ["p", "3"], 9
            i += 2
        else:
            head, n = [cmd], ARITY[cmd]
            i += 1
        vals = tokens[i:i + n]
        i += n
        if cmd in ("s", "box", "p", "pl", "l"):
            k = n_light if cmd == "l" else n_prim
            new = move(cmd, k, np.array([float(v) for v in vals], np.float64))
            if new is not None:
                vals = ["%.9g" % v for v in new]
            if cmd == "l":
                n_light += 1
            else:
                n_prim += 1
        out.append(" ".join(head + list(vals)))
    open(dst, "w").write("\n".join(out) + "\n")


def bounds(ptype, data12):
    """(lo [n, 3], hi [n, 3], bounded [n]) of flattened primitives (HostScene.arrays()): planes are unbounded."""
    d = np.asarray(data12, np.float64)
    t = np.asarray(ptype)
    lo, hi = np.zeros((len(t), 3)), np.zeros((len(t), 3))
    s = t == 0
    lo[s], hi[s] = d[s, :3] - np.abs(d[s, 3:4]), d[s, :3] + np.abs(d[s, 3:4])
    tr = t == 1
    pts = d[tr, :9].reshape(-1, 3, 3)
    lo[tr], hi[tr] = pts.min(1), pts.max(1)
    b = t == 2
    lo[b], hi[b] = np.minimum(d[b, :3], d[b, 3:6]), np.maximum(d[b, :3], d[b, 3:6])
    return lo, hi, t != 3


def assert_boxes_disjoint(ptype, data_a, data_b, moved):
    """Every moved bounded primitive's new bounding box is disjoint from its old one."""
    lo_a, hi_a, bounded = bounds(ptype, data_a)
    lo_b, hi_b, _ = bounds(ptype, data_b)
    moved = np.asarray(moved)
    moved = moved[bounded[moved]]
    assert len(moved), "no bounded primitive moved"
    apart = ((lo_a[moved] > hi_b[moved]) | (lo_b[moved] > hi_a[moved])).any(-1)
    assert apart.all(), "primitives %s overlap their old boxes" % (moved[~apart][:8],)


def assert_frames_differ(frame_a, frame_b, share=0.05):
    """A's frame differs from B's in at least `share` of the pixels (rgb32f bits)."""
    a = np.ascontiguousarray(frame_a, np.float32).view(np.uint32)
    b = np.ascontiguousarray(frame_b, np.float32).view(np.uint32)
    frac = float((a != b).any(-1).mean())
    assert frac >= share, "only %.1f %% of the pixels differ" % (100 * frac)


def shift_out_of_own_box(kind, vals, margin=0.25):
    """A primitive translated along its thinnest axis, towards the origin, by its extent there + margin."""
    if kind == "s":
        lo, hi = vals[:3] - abs(vals[3]), vals[:3] + abs(vals[3])
    elif kind == "box":
        lo, hi = np.minimum(vals[:3], vals[3:]), np.maximum(vals[:3], vals[3:])
    else:
        pts = vals.reshape(3, 3)
        lo, hi = pts.min(0), pts.max(0)
    a = int(np.argmin(hi - lo))
    step = np.zeros(3)
    step[a] = (hi[a] - lo[a] + margin) * (-1.0 if lo[a] + hi[a] > 0 else 1.0)
    out = vals.copy()
    if kind == "s":
        out[:3] += step
    else:
        out += np.tile(step, len(vals) // 3)
    return out


LATTICE_NX, LATTICE_NY, LATTICE_PITCH = 31, 20, 0.2


def lattice_cell(c):
    """Centre (x, y) of lattice cell c."""
    return ((c % LATTICE_NX) - (LATTICE_NX - 1) / 2) * LATTICE_PITCH, ((c // LATTICE_NX) - (LATTICE_NY - 1) / 2) * LATTICE_PITCH


def write_lattice_scene(path, rng, n_tri=600, n_sph=12, res=(96, 64)):
    """n_tri small triangles and n_sph small spheres, each inside its own cell of a 31 x 20 lattice (pitch 0.2, primitives
    within 0.09 of the cell centre in x and y, so no two primitives' boxes touch), at random heights over a floor plane: one material per
    primitive, far more records than the 24 KiB a scene served from LDS may have.  Returns each primitive's cell."""
    assert n_tri + n_sph <= LATTICE_NX * LATTICE_NY
    L = ["accel 2", "spp 0", "bclr 0.1 0.3 0.6", "v", "from 0.3 -0.4 5.0", "at 0 0 0", "up 0 1 0", "angle 60",
         "hither 0.01", "resolution %d %d" % res, "aperture 0", "focal 1", "l 3 -4 8 1 1 1", "l -4 2 6 0.6 0.6 0.5"]
    cells = rng.permutation(LATTICE_NX * LATTICE_NY)[:n_tri + n_sph]
    for k, c in enumerate(cells):
        x, y = lattice_cell(int(c))
        z = rng.uniform(-0.5, 0.5)
        col = rng.uniform(0.2, 1, 3)
        if rng.uniform() < 0.3:
            L.append("f %.3f %.3f %.3f 0.5 1 1 1 0.6 40 0 1" % tuple(col))
        else:
            L.append("f %.3f %.3f %.3f 0.8 1 1 1 0 20 0 1" % tuple(col))
        if k < n_tri:
            p = np.array([x, y, z]) + rng.uniform(-0.09, 0.09, (3, 3))
            L.append("p 3\n" + "\n".join("%.4f %.4f %.4f" % tuple(q) for q in p))
        else:
            L.append("s %.4f %.4f %.4f %.4f" % (x + rng.uniform(-0.01, 0.01), y + rng.uniform(-0.01, 0.01), z, rng.uniform(0.04, 0.07)))
    L += ["f 0.7 0.7 0.6 0.8 1 1 1 0.2 30 0 1", "pl 10 10 -0.8 -10 10 -0.8 -10 -10 -0.8"]      # the last primitive: a floor
    open(path, "w").write("\n".join(L) + "\n")
    return cells
