"""Scenes for the p3d_scene_rebuild tests: the lattice of the update tests with any number of further positions, and a scene
whose coordinates are all dyadic, so that the bounds a rebuild derives from the device records (p0, p0 + e1, p0 + e2) are,
bit for bit, the bounds creation derives from the description (p0, p1, p2)."""
import numpy as np

import scene_motion as M

# ---- the lattice of test_gpu_scene_update.lattice(), with the cells kept so that further positions can be written


def write_lattice(path, seed=4, res=(96, 64)):
    """Scene A of test_gpu_scene_update.lattice() (same generator, same seed); returns each primitive's cell."""
    return M.write_lattice_scene(path, np.random.default_rng(seed), res=res)


def write_lattice_moved(src, dst, cells, target, only=None):
    """src with primitive k (of those in `only`; None: all) moved from cell cells[k] to cell target[k]."""
    def move(kind, k, v):
        if kind in ("l", "pl") or (only is not None and k not in only):
            return None
        (x0, y0), (x1, y1) = M.lattice_cell(int(cells[k])), M.lattice_cell(int(target[k]))
        step = np.array([x1 - x0, y1 - y0, 0.0])
        out = v.copy()
        if kind == "s":
            out[:3] += step
        else:
            out += np.tile(step, 3)
        return out
    M.rewrite_p3f(src, dst, move)


# ---- the dyadic scene

DY_NX, DY_NY = 21, 17                  # cells of pitch 1/4
DY_TRI, DY_SPH, DY_BOX = 320, 12, 5    # 337 bounded primitives: odd, so the last leaf holds one
Q = 1.0 / 256.0


def _dy_cell(c):
    return ((c % DY_NX) - (DY_NX - 1) / 2) * 0.25, ((c // DY_NX) - (DY_NY - 1) / 2) * 0.25


def dyadic_primitives(seed=11):
    """(kinds, values, cells): "p" / "s" / "box" per primitive with its 9 / 4 / 6 numbers, every one a multiple of 2^-8
    below 8 in size, each primitive within 0.11 of its own cell's centre in x and y."""
    rng = np.random.default_rng(seed)
    n = DY_TRI + DY_SPH + DY_BOX
    assert n % 2 == 1 and n <= DY_NX * DY_NY
    cells = rng.permutation(DY_NX * DY_NY)[:n]
    order = rng.permutation(n)                    # kinds interleaved in scene order: neighbours of different kinds
    kind_of = np.array(["p"] * DY_TRI + ["s"] * DY_SPH + ["box"] * DY_BOX)[order]
    kinds, values = [], []
    for k in range(n):
        x, y = _dy_cell(int(cells[k]))
        z = rng.integers(-128, 129) * Q
        c = np.array([x, y, z])
        if kind_of[k] == "p":
            v = (c + rng.integers(-28, 29, (3, 3)) * Q).ravel()
        elif kind_of[k] == "s":
            v = np.concatenate([c, [rng.integers(12, 25) * Q]])
        else:
            h = rng.integers(8, 25, 3) * Q
            v = np.concatenate([c - h, c + h])
        kinds.append(str(kind_of[k])); values.append(v)
    return kinds, values, cells


def move_dyadic(values, kinds, cells, target):
    """Every primitive translated from its cell to target's: the steps are multiples of 1/4, so the values stay dyadic."""
    out = []
    for k, v in enumerate(values):
        (x0, y0), (x1, y1) = _dy_cell(int(cells[k])), _dy_cell(int(target[k]))
        step = np.array([x1 - x0, y1 - y0, 0.0])
        w = v.copy()
        if kinds[k] == "s":
            w[:3] += step
        else:
            w += np.tile(step, len(v) // 3)
        out.append(w)
    return out


def write_dyadic_scene(path, kinds, values, res=(96, 64), seed=12):
    """One material per primitive (far more records than a scene served from LDS may have) and a floor plane behind them."""
    rng = np.random.default_rng(seed)
    L = ["accel 2", "spp 0", "bclr 0.1 0.3 0.6", "v", "from 0.25 -0.5 5.0", "at 0 0 0", "up 0 1 0", "angle 60",
         "hither 0.01", "resolution %d %d" % res, "aperture 0", "focal 1", "l 3 -4 8 1 1 1", "l -4 2 6 0.6 0.6 0.5"]
    for kind, v in zip(kinds, values):
        col = rng.uniform(0.2, 1, 3)
        if rng.uniform() < 0.3:
            L.append("f %.3f %.3f %.3f 0.5 1 1 1 0.6 40 0 1" % tuple(col))
        else:
            L.append("f %.3f %.3f %.3f 0.8 1 1 1 0 20 0 1" % tuple(col))
        assert np.array_equal(np.round(v * 256), v * 256) and np.abs(v).max() < 8
        L.append(("p 3\n" if kind == "p" else kind + " ") + " ".join("%.9g" % x for x in v))
    L += ["f 0.7 0.7 0.6 0.8 1 1 1 0.2 30 0 1", "pl 10 10 -0.75 -10 10 -0.75 -10 -10 -0.75"]
    open(path, "w").write("\n".join(L) + "\n")


def assert_edges_exact(ptype, data12):
    """The precondition the builder-tree test rests on, in float32: p0 + (p1 - p0) == p1 and p0 + (p2 - p0) == p2, bitwise,
    for every triangle."""
    d = np.ascontiguousarray(data12, np.float32)[np.asarray(ptype) == 1]
    assert len(d) >= 300
    p0, p1, p2 = d[:, 0:3], d[:, 3:6], d[:, 6:9]
    for p in (p1, p2):
        back = (p0 + (p - p0).astype(np.float32)).astype(np.float32)
        assert np.array_equal(back.view(np.uint32), np.ascontiguousarray(p).view(np.uint32))
