"""Cameras for the tile coverage mask tests (test_tile_coverage_host.py, test_gpu_sky_tiles.py): a scene file rewritten with
another `from` / `at` / `angle`, so that the host layer's camera and the oracle's are the same file's."""
import os

import numpy as np

SPHERE, TRIANGLE, BOX, PLANE = 0, 1, 2, 3


def write_view(src, out, eye, at, angle):
    """src's scene seen from `eye` towards `at` with the opening `angle` (degrees), written to `out`."""
    with open(src) as f:
        lines = f.read().splitlines()
    new = {"from": "from %.9g %.9g %.9g" % tuple(float(v) for v in eye), "at": "at %.9g %.9g %.9g" % tuple(float(v) for v in at),
           "angle": "angle %.9g" % float(angle)}
    seen = set()
    for i, l in enumerate(lines):
        key = l.split(" ")[0] if l else ""
        if key in new and key not in seen:          # the viewpoint block comes first in a .p3f: its first `from` / `at` / `angle`
            lines[i] = new[key]
            seen.add(key)
    assert seen == set(new), (src, seen)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return out


def bounds(ptype, data12):
    """(lo, hi) of the bounded primitives of a flattened scene (HostScene.arrays())."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for t, d in zip(ptype, data12.astype(np.float64)):
        if t == SPHERE:
            pts = [d[:3] - d[3], d[:3] + d[3]]
        elif t == TRIANGLE:
            pts = [d[0:3], d[3:6], d[6:9]]
        elif t == BOX:
            pts = [d[0:3], d[3:6]]
        else:
            continue
        for p in pts:
            lo, hi = np.minimum(lo, p), np.maximum(hi, p)
    return lo, hi


def first_bounded_centre(ptype, data12):
    """a point inside the first bounded primitive: a sphere's or a box's centre, a triangle's centroid"""
    for t, d in zip(ptype, data12.astype(np.float64)):
        if t == SPHERE:
            return d[:3]
        if t == TRIANGLE:
            return (d[0:3] + d[3:6] + d[6:9]) / 3.0
        if t == BOX:
            return (d[0:3] + d[3:6]) / 2.0
    raise ValueError("no bounded primitive")


def seeded_views(ptype, data12, n, seed):
    """n views (name, eye, at, angle) of a scene: three fixed ones -- turned away from the scene, inside its bounds, and one
    whose eye plane cuts through a primitive -- and seeded ones around it, near and far, aimed at and past the scene, so
    that primitives leave the frame on every side."""
    lo, hi = bounds(ptype, data12)
    c, r = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo)) / 2.0
    rng = np.random.default_rng(seed)
    far = c + np.array([2.2, 1.4, 1.1]) * r
    inside = first_bounded_centre(ptype, data12)
    out = [("turned_away", far, far + (far - c), 45.0),
           ("inside_bounds", c + np.array([0.013, 0.007, 0.011]) * r, c + np.array([1.0, 0.3, 0.1]) * r, 50.0),
           # the eye sits beside a primitive and looks past it sideways: part of the primitive is behind the eye plane
           ("straddles_eye_plane", inside + np.array([0.0, 0.0, 0.02]) * r + np.array([1e-3, 0.0, 0.0]), inside + np.array([0.0, 5.0, 0.02]) * r, 60.0)]
    while len(out) < n:
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        if abs(d[2]) > 0.95:                          # `up` is the z axis in every scene used: keep off it
            continue
        eye = c + d * r * rng.uniform(1.3, 5.0)
        at = c + rng.uniform(-1.0, 1.0, 3) * r * rng.choice([0.2, 1.0, 2.5])
        out.append(("seed%d_%02d" % (seed, len(out)), eye, at, float(rng.uniform(15.0, 75.0))))
    return out


def gpu_views(ptype, data12, file_view):
    """The handful of views the GPU tests render (name, eye, at, angle): the file's own; the scene small in the middle of
    the frame, at its edge, and out of it altogether (every primitive in front of the eye, none in the frame: all sky); and
    two that must run without a mask -- the eye inside the scene's bounds, and the scene behind the eye."""
    lo, hi = bounds(ptype, data12)
    c, r = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo)) / 2.0
    d = np.array([0.74, 0.52, 0.43])
    far = c + d / np.linalg.norm(d) * 4.0 * r
    side = np.cross(d, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    return [("file",) + tuple(file_view),
            ("middle", far, c, 40.0),
            ("near", c + d / np.linalg.norm(d) * 2.0 * r, c, 55.0),
            ("edge", far, c + side * 1.1 * r + np.array([0.0, 0.0, 0.5 * r]), 40.0),
            ("upper", far, c - np.array([0.0, 0.0, 1.1 * r]), 40.0),
            ("lower", far, c + np.array([0.0, 0.0, 1.1 * r]), 40.0),
            ("all_sky", far, c + side * 6.0 * r, 15.0),
            ("inside_bounds", c + np.array([0.013, 0.007, 0.011]) * r, c + np.array([1.0, 0.3, 0.1]) * r, 50.0),
            ("behind_eye", far, far + (far - c), 45.0)]


def file_view(path):
    """(eye, at, angle) of a scene file's viewpoint block"""
    got = {}
    with open(path) as f:
        for l in f.read().splitlines():
            w = l.split()
            if w and w[0] in ("from", "at", "angle") and w[0] not in got:
                got[w[0]] = [float(v) for v in w[1:]]
    return np.array(got["from"]), np.array(got["at"]), got["angle"][0]


def workgroup_patterns(active, tiles):
    """What the workgroups of the level-1 launch with `tiles` tiles each see of a mask [tiles_y, tiles_x]: the set of
    tuples (first tile active, second tile active, ...) over workgroups (bx, by), whose tiles are rows by, by + gy, ... of
    column bx, gy = ceil(tiles_y / tiles) (csrc/p3d_kernel_variant.h: primary_grid); rows past the band are left out."""
    ty_n, tx_n = active.shape
    gy = (ty_n + tiles - 1) // tiles
    seen = set()
    for by in range(gy):
        rows = [by + k * gy for k in range(tiles) if by + k * gy < ty_n]
        for bx in range(tx_n):
            seen.add(tuple(bool(active[ty, bx]) for ty in rows))
    return seen


def tile_has_hit(hit_id, tile_h=16):
    """[tiles_y, tiles_x] bool: the 16 x tile_h tile holds a pixel with hit_id >= 0 (rows beyond the image count as empty)."""
    H, W = hit_id.shape
    th, tw = (H + tile_h - 1) // tile_h, (W + 15) // 16
    pad = np.zeros((th * tile_h, tw * 16), bool)
    pad[:H, :W] = hit_id >= 0
    return pad.reshape(th, tile_h, tw, 16).any(axis=(1, 3))


def view_path(tmpdir, scene, name):
    return os.path.join(str(tmpdir), "%s_%s.p3f" % (scene, name))
