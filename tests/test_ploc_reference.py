"""Builder 2 without a GPU: the restatement (tests/ploc_reference.py) has the properties the clustering rules promise on
every probe case (tests/ploc_cases.py), the fixtures have the properties the GPU tests (tests/test_gpu_ploc.py) rely on, and
the C interface is there: the header declares the new entries, the library exports them, the ABI version is still 4, and
the argument checks that need no device answer with a message."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
import ploc_cases as K
import ploc_reference as R
import u_4a_2s_p3d_raytracer_template2_amd as P
from u_4a_2s_p3d_raytracer_template2_amd import api

ERR_ARG = -1
NEW_SYMBOLS = ("p3d_scene_rebuild_with", "p3d_scene_last_builder", "p3d_debug_ploc_build")
_TREES = {}


def trees(name):
    """(builder 2's restated tree, builder 1's) of a probe case, computed once."""
    if name not in _TREES:
        lo, hi = K.PROBE_CASES[name]()
        _TREES[name] = (lo, hi, R.ploc_tree(lo, hi), R.lbvh_tree(lo, hi))
    return _TREES[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(K.PROBE_CASES))
def test_restated_tree_is_a_tree_over_the_sorted_leaves(name):
    lo, hi, t, _ = trees(name)
    n, L = len(lo), (len(lo) + 1) // 2
    child = t["child"]
    assert child.shape == (L - 1, 2) and t["n"] == n and np.array_equal(np.sort(t["order"]), np.arange(n))
    # each leaf and each inner node but the root is a child exactly once; the root, node 0, never is
    assert np.array_equal(np.sort(~child[child < 0]), np.arange(L))
    assert np.array_equal(np.sort(child[child >= 0]), np.arange(1, L - 1))
    if not t["fell_back"]:
        inner = child >= 0
        assert (child[inner] > np.repeat(np.arange(L - 1)[:, None], 2, 1)[inner]).all(), "a child's index is not above its parent's"
    # the boxes are exact unions, and the leaves' are those of their primitives
    slo, shi = lo[t["order"]], hi[t["order"]]
    for j in range(L):
        assert np.array_equal(bits(t["leaf_lo"][j]), bits(slo[2 * j:2 * j + 2].min(0)))
        assert np.array_equal(bits(t["leaf_hi"][j]), bits(shi[2 * j:2 * j + 2].max(0)))
    clo, chi = R.child_boxes(t)
    assert np.array_equal(bits(t["node_lo"]), bits(np.minimum(clo[:, 0], clo[:, 1])))
    assert np.array_equal(bits(t["node_hi"]), bits(np.maximum(chi[:, 0], chi[:, 1])))
    # max_depth is 1 + the most inner nodes on a path from the root, found here from the top down
    depth = np.zeros(L - 1, np.int64)
    depth[0] = 1
    stack = [0]
    while stack:
        node = stack.pop()
        for c in child[node]:
            if c >= 0:
                depth[c] = depth[node] + 1
                stack.append(int(c))
    assert (depth > 0).all() and t["max_depth"] == depth.max() + 1
    assert 1 <= t["rounds"] <= R.MAX_ROUNDS
    if not t["fell_back"]:
        assert t["max_depth"] <= t["rounds"] + 1
    assert t["max_depth"] <= 96                      # builder 1's bound, which every schedule holds (tests/test_gpu_lbvh.py)
    pairs = R.node_pairs(t)
    assert pairs.shape == (L - 1, 16) and not pairs[:, 14:].any()


def test_fallback_is_builder_1s_tree():
    _, _, t, one = trees("chain_200")
    assert t["fell_back"] == 1 and t["rounds"] == R.MAX_ROUNDS
    assert np.array_equal(R.node_pairs(t), R.node_pairs(one)) and t["max_depth"] == one["max_depth"] and t["cost"] == one["cost"]


def test_what_the_gpu_tests_rely_on():
    _, _, t, one = trees("clusters_and_floor_1201")
    print("clusters and floor: builder 2 %.4f builder 1 %.4f" % (t["cost"], one["cost"]))
    assert not t["fell_back"] and t["cost"] < one["cost"]
    assert trees("chain_200")[2]["fell_back"] == 1
    t = trees("chain_192")[2]
    assert t["fell_back"] == 0 and t["rounds"] == 94
    lo, hi, t, _ = trees("concentric_130")
    assert len(np.unique(R.morton_keys(lo, hi))) == 1
    assert t["fell_back"] == 0 and t["max_depth"] >= 60 and t["rounds"] == 64
    lo, hi, t, _ = trees("uniform_1042")
    assert (len(lo) + 1) // 2 == 521 > 2 * 256
    for name in K.PROBE_CASES:                       # no bound of a box is a zero of either sign next to the other: fminf / fmaxf
        lo, hi = trees(name)[:2]                     # leave that sign open, and the boxes are compared bit for bit
        for v in (lo, hi):
            z = v[v == 0]
            assert len(z) == 0 or np.signbit(z).all() or not np.signbit(z).any(), name


def header():
    return open(os.path.join(REPO, "include", "p3d_hip.h")).read()


def test_header_declares_and_library_exports_the_new_entries():
    h = header()
    assert re.search(r"int\s+p3d_scene_rebuild_with\s*\(\s*p3d_scene\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*p3d_rebuild_info\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"int\s+p3d_scene_last_builder\s*\(\s*const\s+p3d_scene\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"int\s+p3d_debug_ploc_build\s*\([^)]*int32_t\s*\*\s*rounds\s*,\s*int32_t\s*\*\s*fell_back\s*\)\s*;", h)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert name in api.C_ABI_SYMBOLS and hasattr(P.lib(), name)
        assert re.search(r"\bT %s\b" % name, exported)


def test_abi_version_is_still_4():
    assert P.lib().p3d_abi_version() == 4
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4\b", header())
    assert hasattr(api, "ploc_build") and hasattr(P.DeviceScene, "last_builder")


def test_arguments_are_refused_without_a_device():
    L = P.lib()
    info = api.RebuildInfo()
    builder = C.c_int32(7)
    not_a_scene = C.cast((C.c_ubyte * 64)(), C.c_void_p)       # never read: the NULL output is refused first
    buf = (C.c_uint32 * 64)()
    p = C.cast(buf, C.c_void_p)
    calls = [(L.p3d_scene_rebuild_with, (None, b, i)) for b in (0, 1, 2, 3) for i in (C.byref(info), None)]
    calls += [(L.p3d_scene_last_builder, (None, C.byref(builder))), (L.p3d_scene_last_builder, (not_a_scene, None)),
              (L.p3d_debug_ploc_build, (0, 8, p, p, p, p, p, p, p, None, p)), (L.p3d_debug_ploc_build, (0, 8, p, p, p, p, p, p, p, p, None)),
              (L.p3d_debug_ploc_build, (0, 8, None, p, p, p, p, p, p, p, p)), (L.p3d_debug_ploc_build, (0, 3, p, p, p, p, p, p, p, p, p))]
    for fn, args in calls:
        assert fn(*args) == ERR_ARG
        assert L.p3d_last_error().decode() != ""
    assert builder.value == 7
