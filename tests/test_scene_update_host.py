"""p3d_scene_update without a GPU: the header declares it, the library exports it, the ctypes structure of api.py has the
layout the header's C structure has (asked of the C compiler), the ABI version is still 4 (the entry only adds to the
interface), and the argument checks that need no device answer with a message."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import REPO
import u_4a_2s_p3d_raytracer_template2_amd as P
from u_4a_2s_p3d_raytracer_template2_amd import api

ERR_ARG = -1
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "p3d_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(p3d_prim_update), offsetof(p3d_prim_update, n), offsetof(p3d_prim_update, index),
           offsetof(p3d_prim_update, prim_data), offsetof(p3d_prim_update, memory), offsetof(p3d_prim_update, lights));
    return 0;
}
"""


def test_header_declares_p3d_scene_update():
    header = open(os.path.join(REPO, "include", "p3d_hip.h")).read()
    assert re.search(r"int\s+p3d_scene_update\s*\(\s*p3d_scene\s*\*\s*\w+\s*,\s*const\s+p3d_prim_update\s*\*\s*\w+\s*\)\s*;", header)
    assert "typedef struct p3d_prim_update" in header
    assert "p3d_scene_update" in api.C_ABI_SYMBOLS


def test_library_exports_p3d_scene_update():
    assert hasattr(P.lib(), "p3d_scene_update")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    assert re.search(r"\bT p3d_scene_update\b", exported)


def test_abi_version_is_still_4():
    assert P.lib().p3d_abi_version() == 4
    header = open(os.path.join(REPO, "include", "p3d_hip.h")).read()
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4\b", header)


def test_update_structure_has_the_headers_layout(tmp_path):
    (tmp_path / "layout.c").write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-I", str(REPO) + "/include", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "layout")]).decode().split()]
    U = api.PrimUpdate
    assert got == [C.sizeof(U), U.n.offset, U.index.offset, U.prim_data.offset, U.memory.offset, U.lights.offset]


def test_null_arguments_are_refused_without_a_device():
    L = P.lib()
    data = np.zeros((2, 12), np.float32)
    u = api.PrimUpdate(2, None, data.ctypes.data, 0, None)
    not_a_scene = (C.c_ubyte * 64)()                       # never read: the NULL update is refused first
    for args in ((None, C.byref(u)), (None, None), (C.cast(not_a_scene, C.c_void_p), None)):
        assert L.p3d_scene_update(*args) == ERR_ARG
        assert L.p3d_last_error().decode() != ""
