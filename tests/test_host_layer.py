"""CPU-side tests of the product's host layer and of the C-ABI library surface (no GPU calls)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, scene_path
from oracle import oracle_py as O
import u_4a_2s_p3d_raytracer_template2_amd as P
from u_4a_2s_p3d_raytracer_template2_amd import api

SCENES = ["mount_low", "balls_low", "balls_medium", "balls_box", "dof", "mount_high", "dragon"]


def test_library_loads_and_exports_every_declared_symbol():
    L = P.lib()
    header = open(os.path.join(REPO, "include", "p3d_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(p3d_[a-z_]+)\s*\(", header)))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(L, name), "libp3d_hip.so does not export %s" % name
    assert sorted(api.C_ABI_SYMBOLS) == declared
    assert L.p3d_abi_version() == 4
    pt_header = open(os.path.join(REPO, "include", "p3d_pathtracer.h")).read()
    pt_declared = sorted(set(re.findall(r"\b(p3d_pt_[a-z_]+)\s*\(", pt_header)))
    assert pt_declared == sorted(api.PT_C_ABI_SYMBOLS)
    for name in pt_declared:
        assert hasattr(L, name), "libp3d_hip.so does not export %s" % name


def test_library_links_rccl_and_the_gather_rejects_bad_arguments():
    """the frame gather lives behind the C-ABI (csrc/p3d_comm.cpp) and is RCCL's
    ncclSend/ncclRecv, not a Python-side collective.  No GPU here: only linkage and argument checks."""
    import subprocess
    dyn = subprocess.check_output(["readelf", "-d", api.LIB_PATH]).decode()
    assert "librccl.so" in dyn, "libp3d_hip.so is not linked against RCCL"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", api.LIB_PATH]).decode()
    for sym in ("ncclCommInitAll", "ncclCommInitRank", "ncclGetUniqueId", "ncclSend", "ncclRecv",
                "ncclGroupStart", "ncclGroupEnd", "ncclReduce"):
        assert sym in und, sym
    L = P.lib()
    h = C.c_void_p()
    ident = (C.c_ubyte * api.COMM_ID_BYTES)()
    for (rank, world) in ((2, 2), (-1, 4), (0, 0), (0, 65)):
        assert L.p3d_comm_create(ident, rank, world, 0, C.byref(h)) == -1          # P3D_ERR_ARG
        assert h.value is None and L.p3d_last_error()
    assert L.p3d_comm_create(None, 0, 1, 0, C.byref(h)) == -1
    hs = (C.c_void_p * 4)()
    assert L.p3d_comm_create_all(None, 0, hs) == -1
    assert L.p3d_comm_create_all(None, 100, hs) == -1
    assert L.p3d_gather(None, None, None, None, 16) == -1
    assert L.p3d_gather_all(None, None, None, 2, None, 16) == -1
    assert L.p3d_comm_destroy(None) == 0
    with pytest.raises(P.P3DError):                 # no GPU in the build container: an error, never a fallback
        if P.device_count() == 0:
            P.Comm.create_all([0])
        else:
            raise P.P3DError("GPU present: the hardware path is covered by tests/test_gpu_multigpu.py")


@pytest.mark.parametrize("name", SCENES)
def test_host_grid_is_the_reference_grid(name):
    """csrc/grid_builder.cpp (what GRID mode walks on the device) == Grid::Build: the oracle's restatement is
    bit-checked against the reference's own grid.o in tests/test_oracle_vs_ref.py, so equality with it is
    equality with the reference: same dimensions, same population in every cell."""
    hs = P.HostScene(scene_path(name))
    dims, counts = api.host_grid(hs.desc())
    sc = O.Scene(scene_path(name))
    d_o, c_o = sc.refgrid_dims(with_cells=True)
    assert np.array_equal(dims, d_o)
    assert np.array_equal(counts, c_o.astype(np.uint32))


def test_set_skybox_rejects_bad_arguments():
    L = P.lib()
    assert L.p3d_scene_set_skybox(None, None, None, None, None) == -1          # P3D_ERR_ARG, no GPU touched
    assert b"NULL" in L.p3d_last_error()


def test_tune_schedule_and_powf_probe_reject_bad_arguments():
    L = P.lib()
    best = C.c_int32(7)
    assert L.p3d_tune_schedule(None, 1, None, None, None, 3, None, C.byref(best)) == -1      # P3D_ERR_ARG, no GPU touched
    assert L.p3d_tune_schedule(None, 0, None, None, None, 3, None, None) == -1
    assert L.p3d_debug_powf(0, 4, None, None, None) == -1
    assert L.p3d_debug_powf(0, 0, (C.c_float * 1)(), (C.c_float * 1)(), (C.c_float * 1)()) == 0   # nothing to do: not an error


def test_host_grid_of_an_empty_and_of_a_flat_scene():
    """Grid::Build's cell-count formula on no primitives is (int)NaN -- undefined behaviour in the reference; the host
    builder answers with ONE empty cell.  A scene with no extent on one axis still gets the reference's grid (every
    bounding box is padded by EPSILON, so the volume is never zero)."""
    mats = np.zeros((1, 12), np.float32)
    none = np.zeros((0, 12), np.float32)
    desc, keep = api.make_desc(np.zeros(0, np.uint32), none, np.zeros(0, np.uint32), mats, np.zeros((0, 6), np.float32), (0, 0, 0))
    dims, counts = api.host_grid(desc)
    assert dims.tolist() == [1, 1, 1] and counts.tolist() == [0]
    # two coplanar triangles and a zero-thickness box in the plane z = 0.5
    data = np.zeros((3, 12), np.float32)
    data[0, :9] = [0, 0, 0.5, 1, 0, 0.5, 0, 1, 0.5]
    data[1, :9] = [1, 1, 0.5, 1, 0, 0.5, 0, 1, 0.5]
    data[2, :6] = [0.2, 0.2, 0.5, 0.4, 0.4, 0.5]
    desc, keep = api.make_desc(np.array([1, 1, 2], np.uint32), data, np.zeros(3, np.uint32), mats, np.zeros((0, 6), np.float32), (0, 0, 0))
    dims, counts = api.host_grid(desc)
    assert (dims >= 1).all() and int(np.prod(dims)) == len(counts) and counts.sum() >= 3
    assert dims[2] == 1                      # 2 * wz * s + 1 with wz = 4 EPSILON


def test_host_triangle_normals_are_the_reference_normals():
    """The device shades triangles with a normal the host computed once (csrc/scene_flatten.cpp) instead of
    re-deriving it per hit: it must be, bit for bit, what the reference's getNormal(hit).normalize() returns --
    the `normal` column of the known-answer table, which tests/golden/make_golden.py took from the reference's
    own Triangle objects."""
    with np.load(os.path.join(REPO, "tests", "golden", "kat.npz")) as z:
        k = {n: z[n] for n in z.files}
    sel = np.nonzero((k["type"] == O.TRIANGLE) & (k["hit"] == 1))[0]
    assert len(sel) > 500
    data = np.zeros((len(sel), 12), np.float32)
    data[:, :9] = k["prim12"][sel, :9]
    mats = np.zeros((1, 12), np.float32)
    desc, keep = api.make_desc(np.full(len(sel), 1, np.uint32), data, np.zeros(len(sel), np.uint32), mats,
                               np.zeros((0, 6), np.float32), (0, 0, 0))
    L = P.lib()
    L.p3dh_triangle_normals.restype = C.c_int64
    L.p3dh_triangle_normals.argtypes = [C.POINTER(api.SceneDesc), C.c_void_p, C.c_uint64]
    out = np.zeros((len(sel), 3), np.float32)
    assert L.p3dh_triangle_normals(C.byref(desc), out.ctypes.data, len(sel)) == len(sel)
    assert np.array_equal(out.view(np.uint32), k["normal"][sel].view(np.uint32))


def test_missing_extension_fails_loudly(monkeypatch):
    monkeypatch.setattr(api, "_lib", None)
    monkeypatch.setattr(api, "LIB_PATH", "/nonexistent/libp3d_hip.so")
    with pytest.raises(P.P3DError):
        api.lib()


@pytest.mark.parametrize("name", SCENES)
def test_loader_matches_oracle_loader(name):
    hs = P.HostScene(scene_path(name))
    sc = O.Scene(scene_path(name))
    assert (hs.n_prims, hs.n_lights, hs.res_x, hs.res_y, hs.accel, hs.spp) == \
           (sc.n_prims, sc.n_lights, sc.res_x, sc.res_y, sc.accel, sc.spp)
    t, d, m, mats, li, bg = hs.arrays()
    to, do, mo = sc.prims()
    assert np.array_equal(t, to.astype(np.uint32)) and np.array_equal(m, mo.astype(np.uint32))
    nonplane = to != O.PLANE
    assert np.array_equal(d[nonplane].view(np.uint32), do[nonplane].view(np.uint32))
    assert np.array_equal(mats.view(np.uint32), sc.materials().view(np.uint32))
    assert np.array_equal(li.view(np.uint32), sc.lights().view(np.uint32))
    assert np.array_equal(bg, sc.bg())
    for (w, h) in ((hs.res_x, hs.res_y), (1920, 1080), (37, 23)):
        hs.set_resolution(w, h)
        sc.set_resolution(w, h)
        c = hs.camera()
        got = np.array(list(c.eye) + list(c.u) + list(c.v) + list(c.n) +
                       [c.w, c.h, c.plane_dist, c.aperture, c.focal_ratio, c.res_x, c.res_y], np.float32)
        assert np.array_equal(got.view(np.uint32), sc.camera().view(np.uint32))
        o1, d1 = hs.primary_ray(3.5, 7.5)
        o2, d2 = sc.primary_ray(3.5, 7.5)
        assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32)) and np.array_equal(o1, o2)


def test_plane_record_is_unit_normal_and_offset():
    hs = P.HostScene(scene_path("balls_medium"))
    t, d, *_ = hs.arrays()
    i = int(np.where(t == 3)[0][0])
    n = d[i, :3]
    assert abs(float(np.linalg.norm(n)) - 1) < 1e-6
    # the plane of balls_medium is z = -0.5
    assert abs(abs(n[2]) - 1) < 1e-6 and abs(d[i, 3] * n[2] - 0.5) < 1e-6


def test_sample_stream_follows_reference_rng_order():
    hs = P.HostScene(scene_path("dof"))
    hs.set_resolution(5, 4)
    spp = 2
    got = hs.samples(777, spp)
    s = O.rand_floats(777, 4096)
    ap = np.float32(hs.camera().aperture)
    k = 0
    exp = np.zeros_like(got)
    for y in range(4):
        for x in range(5):
            for i in range(spp):
                for j in range(spp):
                    px = np.float32(np.float32(x) + np.float32(np.float32(i) + s[k]) / np.float32(spp))
                    py = np.float32(np.float32(y) + np.float32(np.float32(j) + s[k + 1]) / np.float32(spp))
                    k += 2
                    while True:
                        ry, rx = s[k], s[k + 1]   # right-to-left argument evaluation
                        k += 2
                        dx = np.float32(rx * np.float32(2) - np.float32(1))
                        dy = np.float32(ry * np.float32(2) - np.float32(1))
                        if np.float32(np.float32(dx * dx) + np.float32(dy * dy)) < 1.0:
                            break
                    exp[y, x, i * spp + j] = (px, py, np.float32(dx * ap), np.float32(dy * ap))
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def decode_bvh(b):
    nodes = b["nodes"]
    f = nodes.view(np.float32)
    out = []
    for i in range(len(nodes)):
        lo0, hi0 = f[i, 0:3], np.array([f[i, 3], f[i, 4], f[i, 5]])
        lo1, hi1 = np.array([f[i, 6], f[i, 7], f[i, 8]]), f[i, 9:12]
        c = nodes[i, 12:14].view(np.int32)
        out.append(((lo0, hi0, int(c[0])), (lo1, hi1, int(c[1]))))
    return out


@pytest.mark.parametrize("name,leaf_max", [("mount_low", 0), ("balls_medium", 0), ("balls_box", 2),
                                            ("mount_high", 8), ("dragon", 0)])
def test_bvh_builder_invariants(name, leaf_max):
    hs = P.HostScene(scene_path(name))
    t, d, *_ = hs.arrays()
    b = P.host_bvh(hs.desc(), leaf_max)
    tree = decode_bvh(b)
    refs = b["refs"]
    bounded = int((t != 3).sum())
    assert b["n_prims"] == bounded == len(refs)
    # map typed reference -> scene index
    per_kind = {k: np.where(t == k)[0] for k in (0, 1, 2)}
    seen = np.zeros(len(t), np.int32)
    lm = leaf_max or 4

    def prim_box(si):
        k, v = t[si], d[si]
        if k == 0:
            return v[:3] - v[3], v[:3] + v[3]
        if k == 1:
            p = v[:9].reshape(3, 3)
            return p.min(0), p.max(0)
        return np.minimum(v[:3], v[3:6]), np.maximum(v[:3], v[3:6])

    max_depth = 0
    stack = [(0, 1, None, None)]
    while stack:
        ni, depth, plo, phi = stack.pop()
        for (lo, hi, c) in tree[ni]:
            if np.isnan(lo).any():
                continue       # absent child
            assert (lo <= hi).all()
            if plo is not None:
                assert (lo >= plo).all() and (hi <= phi).all()
            if c >= 0:
                stack.append((c, depth + 1, lo, hi))
            else:
                code = (~c) & 0xFFFFFFFF
                first, n = code >> 3, (code & 7) + 1
                assert n <= lm
                max_depth = max(max_depth, depth + 1)
                sids = []
                for r in refs[first:first + n]:
                    si = int(per_kind[int(r) >> 30][int(r) & 0x3FFFFFFF])
                    seen[si] += 1
                    sids.append(si)
                    blo, bhi = prim_box(si)
                    # boxes are PADDED (>= 1e-3) so float rounding in the slab test stays conservative
                    assert (blo - lo >= 0.9e-3).all() and (hi - bhi >= 0.9e-3).all()
                assert sids == sorted(sids)
    assert (seen[t != 3] == 1).all() and (seen[t == 3] == 0).all()
    assert max_depth <= b["max_depth"] + 1 <= 64


@pytest.mark.parametrize("name", ["mount_low", "balls_box", "mount_high"])
def test_build_prims_dump_is_the_padded_scene(name):
    """api.host_build_prims: what both BVH builders are given -- one entry per bounded primitive in scene order, its
    reference kind << 30 | index within the kind, and its bounds padded by max(1e-3, 1e-5 * largest |coordinate|) in f32
    (csrc/scene_flatten.cpp), restated here operation by operation, so equal bit for bit."""
    hs = P.HostScene(scene_path(name))
    t, d, *_ = hs.arrays()
    lo, hi, ref = api.host_build_prims(hs.desc())
    keep = np.flatnonzero(t != 3)
    assert len(ref) == len(keep) and lo.shape == hi.shape == (len(keep), 3) and lo.dtype == np.float32
    f32 = np.float32
    count = {0: 0, 1: 0, 2: 0}
    for k, si in enumerate(keep):
        kind, v = int(t[si]), d[si].astype(f32)
        assert int(ref[k]) == (kind << 30) | count[kind]
        count[kind] += 1
        if kind == 0:
            r = np.abs(v[3])
            blo, bhi = v[:3] - r, v[:3] + r
        elif kind == 1:
            p = v[:9].reshape(3, 3)
            blo, bhi = p.min(0), p.max(0)
        else:
            blo, bhi = np.minimum(v[:3], v[3:6]), np.maximum(v[:3], v[3:6])
        pad = max(f32(1e-3), f32(1e-5) * max(np.abs(blo).max(), np.abs(bhi).max()))
        assert np.array_equal((blo - pad).view(np.uint32), lo[k].view(np.uint32)), (k, si)
        assert np.array_equal((bhi + pad).view(np.uint32), hi[k].view(np.uint32)), (k, si)


def test_device_bvh_probe_rejects_bad_arguments():
    """p3d_debug_lbvh_build answers P3D_ERR_ARG to fewer than 4 primitives and to NULL pointers before it touches a device."""
    L = P.lib()
    lo, hi = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    ref, nodes, refs, st, sah = np.arange(4, dtype=np.uint32), np.zeros((1, 16), np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32), C.c_float()
    ptrs = [lo.ctypes.data, hi.ctypes.data, ref.ctypes.data, nodes.ctypes.data, refs.ctypes.data, st.ctypes.data, C.addressof(sah)]
    for n in (0, 1, 3):
        assert L.p3d_debug_lbvh_build(0, n, *ptrs) == -1 and b"4 primitives" in L.p3d_last_error()
    for k in range(len(ptrs)):
        assert L.p3d_debug_lbvh_build(0, 4, *[None if j == k else p for j, p in enumerate(ptrs)]) == -1
        assert b"NULL" in L.p3d_last_error()
    with pytest.raises(P.P3DError):
        api.device_bvh(lo[:3], hi[:3], ref[:3])


@pytest.mark.parametrize("name", ["mount_low", "balls_box", "mount_high", "dragon"])
def test_quantised_nodes_contain_the_f32_boxes(name):
    """Scenes read from HBM walk 32-byte node pairs of 16-bit plane codes (plane = base + code * scale).  Every coded
    box must contain the builder's padded f32 box with a full code of margin on each side -- evaluated here in the f32
    arithmetic of the kernel's de-quantisation -- keep the child references, and code absent children as the point 0."""
    hs = P.HostScene(scene_path(name))
    b = P.host_bvh(hs.desc(), 0)
    f = b["nodes"].view(np.float32)
    q, sc, ba = b["qnodes"], b["qscale"], b["qbase"]
    assert q.shape == (len(f), 8) and (sc > 0).all()
    lo = np.stack([f[:, 0:3], np.stack([f[:, 6], f[:, 7], f[:, 8]], 1)], 1)               # [node, child, axis]
    hi = np.stack([np.stack([f[:, 3], f[:, 4], f[:, 5]], 1), f[:, 9:12]], 1)
    code = np.stack([q[:, 0:3], q[:, 4:7]], 1)
    qlo, qhi = (code & 0xFFFF).astype(np.float32), (code >> 16).astype(np.float32)
    absent = np.isnan(lo[:, :, 0])
    assert (code[absent] == 0).all()
    real = ~absent
    # a full code of margin on each side: exact in double, >= 0.99 of a code when evaluated in float32
    d64 = ba.astype(np.float64), sc.astype(np.float64)
    assert ((d64[0] + (qlo.astype(np.float64) + 1) * d64[1])[real] <= lo[real]).all()
    assert ((d64[0] + (qhi.astype(np.float64) - 1) * d64[1])[real] >= hi[real]).all()
    dlo = (ba + qlo * sc).astype(np.float32)[real]
    dhi = (ba + qhi * sc).astype(np.float32)[real]
    assert ((lo[real] - dlo) >= 0.99 * sc).all() and ((dhi - hi[real]) >= 0.99 * sc).all()
    assert (qlo[real] >= 1).all() and (qhi[real] <= 65534).all() and (qlo[real] < qhi[real]).all()
    # not looser than three codes per side
    assert ((lo[real] - (ba + qlo[real] * sc)) <= 3.01 * sc).all() and (((ba + qhi[real] * sc) - hi[real]) <= 3.01 * sc).all()
    assert np.array_equal(q[:, 3], b["nodes"][:, 12]) and np.array_equal(q[:, 7], b["nodes"][:, 13])


def test_local_rows():
    assert P.local_rows(1080, 16, 1) == 1088
    assert P.local_rows(1080, 16, 8) == 144      # 68 blocks -> 9 per rank
    assert P.local_rows(4096, 16, 8) == 512
    assert P.local_rows(10, 16, 4) == 16


@pytest.mark.skipif(P.device_count() > 0, reason="needs a machine without a GPU")
def test_no_device_is_an_error_not_a_fallback():
    hs = P.HostScene(scene_path("mount_low"))
    with pytest.raises(P.P3DError) as e:
        P.DeviceScene.from_host(hs)
    assert "device" in str(e.value).lower()


def test_png_writer_round_trip(tmp_path):
    """saveImgFile() replacement (RT/main.cpp:261-276): a valid PNG whose rows are img_Data top-down."""
    import struct, zlib
    from u_4a_2s_p3d_raytracer_template2_amd import api
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (37, 211, 3), dtype=np.uint8)          # > 65535 raw bytes: several stored blocks
    path = str(tmp_path / "RT_Output.png")
    api.save_png(path, img)
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, typ = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(typ + body) & 0xFFFFFFFF
        chunks.append((typ, body)); at += 12 + n
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, _, _, _ = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (w, h, depth, colour) == (211, 37, 8, 2)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(37, 1 + 211 * 3)
    assert (raw[:, 0] == 0).all()
    assert np.array_equal(raw[:, 1:].reshape(37, 211, 3), img[::-1])


def test_synthetic_scene_text_and_array_forms_agree(tmp_path):
    """The scaling scene of SURVEY section 8d: the .p3f the oracle reads and the arrays bench.py uploads
    describe the same primitives, materials and lights, and the host BVH over it is well formed."""
    from u_4a_2s_p3d_raytracer_template2_amd import synthetic as S
    n = 3000
    path = S.write_p3f(str(tmp_path / "synthetic.p3f"), n, 64, 48)
    ptype, data, material, mats, lights, bg = S.arrays(n)
    hs = P.HostScene(path)
    arr = hs.arrays()
    assert np.array_equal(arr[0], ptype)
    d = np.asarray(arr[1]).reshape(-1, 12)
    sph = ptype == 0
    assert np.array_equal(d[sph, :4], data[sph, :4]) and np.array_equal(d[~sph, :9], data[~sph, :9])
    m = np.asarray(arr[3]).reshape(-1, 12)
    assert np.array_equal(m[np.asarray(arr[2])], mats[material])
    assert np.array_equal(np.asarray(arr[4]).reshape(-1, 6), lights)
    sc = O.Scene(path)
    assert sc.n_prims == n
    desc, keep = api.make_desc(ptype, data, material, mats, lights, bg)
    bvh = api.host_bvh(desc)
    assert bvh["n_prims"] == n and len(bvh["refs"]) == n and bvh["max_depth"] <= 40
    assert sorted((bvh["refs"] & 0x3FFFFFFF).tolist()) == sorted(list(range(n // 2)) * 2)   # every sphere and triangle once
