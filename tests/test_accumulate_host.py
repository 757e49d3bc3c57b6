"""p3d_accumulate without a GPU: the host restatement (p3dh_accumulate) against the NumPy restatement of the definition
(tests/accumulate_reference.py), bit for bit, every rejection path of the definition by a constructed case, and the
properties a temporal accumulation must have."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accumulate_reference as R                           # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P            # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api        # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
KW = dict(depth_tolerance=0.1, normal_min=0.8, max_history=4.5)    # 4.5: the generated histories (lengths 1 to 6) reach the cap
# (res_x, res_y): one pixel; smaller than a block; no multiple of any block size in either axis
SHAPES = [(1, 1), (5, 3), (17, 33), (37, 23), (64, 48), (131, 77)]
ERR_ARG, ERR_LIMIT = -1, -4
W, H = 37, 23


def same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def both(seq, hit_ids=True, history="own", **kw):
    """(host layer, NumPy) on a sequence of accumulate_reference.make_sequence()."""
    h = seq["history"] if history == "own" else history
    if not hit_ids:
        h = R.without_hit_ids(h)
    args = (seq["rgb32f"], seq["depth"], seq["normal"], seq["cams"], seq["hit_id"] if hit_ids else None, h)
    return api.host_accumulate(*args, **kw), R.accumulate(*args, kw["depth_tolerance"], kw["normal_min"], kw["max_history"])


@pytest.mark.parametrize("hit_ids", [True, False])
@pytest.mark.parametrize("history", [False, True])
@pytest.mark.parametrize("n_frames", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_equals_the_numpy_restatement(shape, n_frames, history, hit_ids):
    seq = R.make_sequence(*shape, n_frames, seed=n_frames, history=history)
    got, ref = both(seq, hit_ids, **KW)
    same_bits(got["rgb32f"], ref["rgb32f"], "rgb32f")
    same_bits(got["length"], ref["length"], "length")
    # neither branch is vacuous, on the NumPy result alone.  A frame of one pixel cannot do both: there the pixel of every
    # frame f >= 1 takes history, and the refusal is that of frame 0 of the cases without a history.
    took = ref["length"] > 1
    assert not took[0].any() or history
    for f in range(0 if history else 1, n_frames):
        assert took[f].mean() >= 0.1, "frame %d: only %.3f of the pixels took history" % (f, took[f].mean())
        if shape != (1, 1):
            assert (~took[f]).mean() >= 0.01, "frame %d: only %.3f of the pixels refused history" % (f, (~took[f]).mean())
        assert not np.array_equal(ref["rgb32f"][f][took[f]], seq["rgb32f"][f][took[f]])
        same_bits(ref["rgb32f"][f][~took[f]], seq["rgb32f"][f][~took[f]], "no history: the colour is copied")
    if shape == (1, 1) and not history:
        assert not took[0].any()
    if history and shape != (1, 1):
        assert (ref["length"] == F(KW["max_history"])).any(), "max_history was never reached"


def test_hit_ids_change_the_result():
    seq = R.make_sequence(64, 48, 4, seed=2, history=True)
    assert not np.array_equal(both(seq, True, **KW)[1]["length"], both(seq, False, **KW)[1]["length"])


# ---- every rejection path, by a constructed case: a frame and the frame it looks back at, one of them damaged
def pair(cam, prev_cam):
    """(frame, prev): the planes of accumulate_reference.trace() through cam, and those through prev_cam as a history of
    length 3."""
    z, n, hit, c = R.trace(cam)
    pz, pn, phit, pc = R.trace(prev_cam)
    return dict(rgb32f=c, depth=z, normal=n, hit_id=hit, cam=cam), dict(rgb32f=pc, depth=pz, normal=pn, hit_id=phit, cam=prev_cam,
                                                                         length=np.full(pz.shape, 3.0, F))


def run_pair(frame, prev, **kw):
    """The pair through both restatements, compared; -> (colour, length, probe) of the NumPy one."""
    kw = {**KW, "max_history": 32.0, **kw}
    got = api.host_accumulate(frame["rgb32f"], frame["depth"], frame["normal"], frame["cam"], frame["hit_id"], prev, **kw)
    probe = {}
    c, ln = R.accumulate_frame(frame["cam"], frame["rgb32f"], frame["depth"], frame["normal"], frame["hit_id"], prev,
                               kw["depth_tolerance"], kw["normal_min"], kw["max_history"], probe=probe)
    same_bits(got["rgb32f"][0] if got["rgb32f"].ndim == 4 else got["rgb32f"], c, "rgb32f")
    same_bits(got["length"].reshape(ln.shape), ln, "length")
    return c, ln, probe


def static_pair():
    cam = R.sequence_camera(0, W, H)
    return pair(cam, cam)


def test_the_undamaged_pair_takes_history_on_every_hit():
    frame, prev = static_pair()
    c, ln, probe = run_pair(frame, prev)
    hit = frame["hit_id"] >= 0
    assert hit.any() and (~hit).any()
    assert (ln[hit] > 1).all() and (ln[~hit] == 1).all()
    assert np.abs(probe["px"][hit] - np.broadcast_to(np.arange(W, dtype=F), (H, W))[hit]).max() < 1e-4       # a static camera lands on the pixel centres


@pytest.mark.parametrize("bad", [np.inf, 0.0, -1.0, np.nan])
def test_an_invalid_current_depth(bad):
    frame, prev = static_pair()
    at = frame["hit_id"] == 1
    frame["depth"][at] = bad
    c, ln, _ = run_pair(frame, prev)
    assert at.any() and (ln[at] == 1).all() and (ln[frame["hit_id"] % 2 == 0] > 1).all()
    same_bits(c[at], frame["rgb32f"][at], "copied")


def test_a_previous_camera_turned_away():
    frame, prev = static_pair()
    prev["cam"] = R.look_at((0.3, 1.6, 5.0), (0.6, 2.4, 10.0), W, H)      # looks the other way: c <= 0
    c, ln, probe = run_pair(frame, prev)
    assert not (probe["c"][frame["hit_id"] >= 0] > 0).any() and (ln == 1).all()
    same_bits(c, frame["rgb32f"], "copied")


def test_a_huge_depth_out_of_range_and_nan():
    frame, prev = pair(R.sequence_camera(0, W, H), R.sequence_camera(-8, W, H))
    frame["depth"][:] = 1e30                                   # no parallax left: the view's turn alone decides
    prev["depth"][:] = 1e30
    c, ln, probe = run_pair(frame, prev)
    out = ~((probe["px"] > -1) & (probe["px"] < W) & (probe["py"] > -1) & (probe["py"] < H))
    assert out.any() and (~out).any() and not np.isnan(probe["px"]).any()
    assert (ln[out] == 1).all() and (ln[~out] > 1).any()
    far = R.sequence_camera(0, W, H)                           # an eye 2e38 behind: q overflows, px is inf / inf
    for k in range(3):
        far.eye[k] = far.eye[k] + 2e38 * far.n[k]
    prev["cam"] = far
    frame["depth"][:] = 3e38
    prev["depth"][:] = 3e38
    c, ln, probe = run_pair(frame, prev)
    assert np.isnan(probe["px"]).all() and (probe["c"] > 0).all() and (ln == 1).all()
    same_bits(c, frame["rgb32f"], "copied")


def test_a_tap_outside_the_frame():
    frame, prev = pair(R.sequence_camera(0, W, H), R.sequence_camera(1, W, H))       # the sequence backwards: the view moves left
    c, ln, probe = run_pair(frame, prev)
    edge = (probe["x0"] == -1) & probe["took"]
    assert edge.any(), "no pixel took history through the taps of column 0 alone"
    assert ((probe["y0"] == -1) & probe["took"]).any()
    assert (ln[edge] > 1).all()


def test_an_invalid_tap_depth():
    frame, prev = static_pair()
    prev["depth"][:] = np.inf
    c, ln, _ = run_pair(frame, prev)
    assert (ln == 1).all()
    frame, prev = static_pair()
    prev["depth"][:, ::2] = np.nan                             # every other column: the taps that are left carry the history
    c, ln, probe = run_pair(frame, prev)
    hit = frame["hit_id"] >= 0
    assert (ln[hit] > 1).any() and (ln[hit] == 1).any()


def test_depth_normal_and_hit_id_mismatches():
    hit = static_pair()[0]["hit_id"] >= 0
    frame, prev = static_pair()
    prev["depth"] = (prev["depth"] * F(1.5)).astype(F)         # |Z' - dist| = 0.5 dist > 0.1 dist
    assert (run_pair(frame, prev)[1] == 1).all()
    assert (run_pair(frame, prev, depth_tolerance=0.6)[1][hit] > 1).all()
    frame, prev = static_pair()
    prev["normal"] = -prev["normal"]
    assert (run_pair(frame, prev)[1] == 1).all()
    assert (run_pair(frame, prev, normal_min=-1.0)[1][hit] > 1).all()
    frame, prev = static_pair()
    prev["hit_id"] = prev["hit_id"] + 7
    assert (run_pair(frame, prev)[1] == 1).all()
    assert (run_pair(frame, R.without_hit_ids(prev))[1][hit] > 1).all(), "without both planes the ids are not compared"
    frame["hit_id"] = None
    assert (run_pair(frame, prev)[1][hit] > 1).all()


def test_max_history_is_reached():
    frame, prev = static_pair()
    hit = frame["hit_id"] >= 0
    prev["length"][:] = 10.0
    c, ln, _ = run_pair(frame, prev, max_history=4.0)
    assert (ln[hit] == 4).all()
    c2, ln2, _ = run_pair(frame, prev, max_history=32.0)
    assert (np.abs(ln2[hit] - 11) < 1e-4).all() and not np.array_equal(c, c2)
    c1, ln1, _ = run_pair(frame, prev, max_history=1.0)       # alpha = 1: the current colour alone
    assert (ln1 == 1).all()
    assert np.abs(c1 - frame["rgb32f"]).max() < 1e-6


# ---- the sequence
@pytest.mark.parametrize("hit_ids", [True, False])
def test_one_call_equals_frame_by_frame_with_the_outputs_fed_back(hit_ids):
    seq = R.make_sequence(W, H, 4, seed=5, history=True)
    hid = seq["hit_id"] if hit_ids else None
    h0 = seq["history"] if hit_ids else R.without_hit_ids(seq["history"])
    whole = api.host_accumulate(seq["rgb32f"], seq["depth"], seq["normal"], seq["cams"], hid, h0, **KW)
    h = h0
    for f in range(4):
        one = api.host_accumulate(seq["rgb32f"][f], seq["depth"][f], seq["normal"][f], seq["cams"][f], None if hid is None else hid[f], h, **KW)
        same_bits(one["rgb32f"], whole["rgb32f"][f], "frame %d rgb32f" % f)
        same_bits(one["length"], whole["length"][f], "frame %d length" % f)
        h = dict(rgb32f=one["rgb32f"], length=one["length"], depth=seq["depth"][f], normal=seq["normal"][f], cam=seq["cams"][f])
        if hit_ids:
            h["hit_id"] = hid[f]
    assert (whole["length"][3] > 1).any()


def exact_camera(res):
    """A camera whose reprojection onto itself is exact at 8 x 8 with depths that are powers of two: at the origin, along
    -z, w = h = plane_dist = 1."""
    c = api.Camera()
    for k in range(3):
        c.eye[k], c.u[k], c.v[k], c.n[k] = 0.0, float(k == 0), float(k == 1), float(k == 2)
    c.w, c.h, c.plane_dist, c.aperture, c.focal_ratio, c.res_x, c.res_y = 1.0, 1.0, 1.0, 0.0, 1.0, res, res
    return c


@pytest.mark.parametrize("max_history", [32.0, 4.0])
def test_a_static_sequence_averages_and_counts(max_history):
    """8 frames of equal geometry through a static camera, independent zero-mean colour noise: no tolerance anywhere.  The
    camera and the depth (a shell of radius 4 around the eye) are chosen so that every pixel reprojects onto its own centre
    EXACTLY (asserted): one tap then carries weight 1 and the lengths are whole numbers; with two taps of equal length L the
    mean (w0 L + w1 L) / (w0 + w1) is L only to an ulp."""
    res, n = 8, 8
    rng = np.random.default_rng(11)
    cam = exact_camera(res)
    z = np.full((n, res, res), 4.0, F)
    z[:, 0, :3] = np.inf                                       # three misses
    nr = np.zeros((n, res, res, 3), F)
    nr[..., 2] = 1.0
    clean = np.broadcast_to(rng.random((res, res, 3), dtype=F), (n, res, res, 3))
    c = (clean + rng.normal(size=clean.shape).astype(F) * F(0.1)).astype(F)
    kw = dict(KW, max_history=max_history)
    probe = {}
    prev = dict(rgb32f=c[0], depth=z[0], normal=nr[0], length=np.ones((res, res), F), hit_id=None, cam=cam)
    R.accumulate_frame(cam, c[1], z[1], nr[1], None, prev, kw["depth_tolerance"], kw["normal_min"], max_history, probe=probe)
    hit = np.isfinite(z[0])
    xs, ys = np.meshgrid(np.arange(res, dtype=F), np.arange(res, dtype=F))
    assert (probe["px"][hit] == xs[hit]).all() and (probe["py"][hit] == ys[hit]).all(), "the reprojection is not exact"
    got = api.host_accumulate(c, z, nr, [cam] * n, None, None, **kw)
    ref = R.accumulate(c, z, nr, [cam] * n, None, None, kw["depth_tolerance"], kw["normal_min"], max_history)
    same_bits(got["rgb32f"], ref["rgb32f"], "rgb32f")
    same_bits(got["length"], ref["length"], "length")
    for f in range(n):
        assert (got["length"][f][hit] == min(f + 1, max_history)).all(), (f, np.unique(got["length"][f][hit]))
        assert (got["length"][f][~hit] == 1).all()
    err = [float(np.abs(got["rgb32f"][f][hit] - clean[f][hit]).mean()) for f in range(n)]
    assert err[7] < err[0], err
    if max_history == 32.0:                                    # the running mean of 8 samples
        mean = c[:, hit].astype(np.float64).mean(0)
        assert np.abs(got["rgb32f"][7][hit] - mean).max() < 1e-5


def test_a_moving_sequence_loses_noise():
    seq = R.make_sequence(64, 48, 8, seed=4)
    got = api.host_accumulate(seq["rgb32f"], seq["depth"], seq["normal"], seq["cams"], seq["hit_id"], None, **dict(KW, max_history=32.0))
    took = got["length"][7] > 1
    smooth = seq["hit_id"][7] == 1                             # the sphere's colour varies slowly: bilinear taps do not blur it
    at = took & smooth
    assert at.sum() > 50
    assert np.abs(got["rgb32f"][7][at] - seq["clean"][7][at]).mean() < 0.6 * np.abs(seq["rgb32f"][7][at] - seq["clean"][7][at]).mean()


# ---- the interface
def test_the_symbols_are_exported_declared_and_listed():
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    for name in ("p3d_accumulate", "p3d_debug_accumulate", "p3dh_accumulate"):
        assert re.search(r"\bT %s$" % name, dyn, re.M), "libp3d_hip.so does not export " + name
        assert hasattr(P.lib(), name)
    header = open(os.path.join(REPO, "include", "p3d_hip.h")).read()
    assert re.search(r"\bint p3d_accumulate\(p3d_scene\* scene, const p3d_accumulate_params\* params, const p3d_accumulate_frames\* frames,\s*"
                     r"const p3d_accumulate_history\* history, const p3d_accumulate_outputs\* out\);", header)
    assert re.search(r"\bint p3d_debug_accumulate\(int device, const p3d_accumulate_params\* params,", header)
    for name in ("p3d_accumulate_params", "p3d_accumulate_frames", "p3d_accumulate_history", "p3d_accumulate_outputs"):
        assert "} %s;" % name in header
    assert "p3d_accumulate" in api.C_ABI_SYMBOLS and "p3d_debug_accumulate" in api.C_ABI_SYMBOLS
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4\b", header) and P.lib().p3d_abi_version() == 4
    assert C.sizeof(api.AccumulateParams) == 24 and api.AccumulateParams.max_history.offset == 20
    assert C.sizeof(api.AccumulateFrames) == 48 and api.AccumulateFrames.cams.offset == 32 and api.AccumulateFrames.memory.offset == 40
    assert C.sizeof(api.AccumulateHistory) == 56 and api.AccumulateHistory.cam.offset == 40 and api.AccumulateHistory.memory.offset == 48
    assert C.sizeof(api.AccumulateOutputs) == 24 and api.AccumulateOutputs.memory.offset == 16
    for name in ("accumulate", "accumulate_device"):
        assert hasattr(P.DeviceScene, name)
    assert hasattr(P, "host_accumulate") and hasattr(P, "debug_accumulate")
    assert api.ACCUMULATE_DEPTH_TOLERANCE > 0 and -1 <= api.ACCUMULATE_NORMAL_MIN <= 1 and api.ACCUMULATE_MAX_HISTORY >= 1


def refusal_cases():
    """(name, expected status, keyword changes of call()) for every refusal the structs imply."""
    good = (5, 3, 1, 0.1, 0.8, 4.0)
    cases = [("params NULL", ERR_ARG, dict(params=None)), ("frames NULL", ERR_ARG, dict(frames=None)), ("out NULL", ERR_ARG, dict(out=None))]
    for k in ("rgb32f", "depth", "normal", "cams"):
        cases.append(("frames->%s NULL" % k, ERR_ARG, dict(frames_null=k)))
    for k in ("rgb32f", "depth", "normal", "length", "cam"):
        cases.append(("history->%s NULL" % k, ERR_ARG, dict(history_null=k)))
    cases.append(("both outputs NULL", ERR_ARG, dict(out_planes=(False, False))))
    for bad in ((0, 3, 1), (5, 0, 1), (5, 3, 0), (-5, 3, 1)):
        cases.append(("shape %s" % (bad,), ERR_ARG, dict(params=bad + good[3:])))
    for field, values in ((3, (0.0, -1.0, np.inf, np.nan)), (4, (-1.5, 1.5, np.nan, np.inf)), (5, (0.5, 0.0, -2.0, np.inf, np.nan))):
        for v in values:
            cases.append(("params[%d] = %r" % (field, v), ERR_ARG, dict(params=good[:field] + (v,) + good[field + 1:])))
    for where in ("frames", "history", "out"):
        for v in (2, -1):
            cases.append(("%s->memory = %d" % (where, v), ERR_ARG, dict(memory={where: v})))
    cases.append(("a camera of another resolution", ERR_ARG, dict(cam_res=(6, 3))))
    cases.append(("the history's camera of another resolution", ERR_ARG, dict(hist_cam_res=(5, 4))))
    for o in ("rgb32f", "length"):
        for k in ("depth", "normal", "hit_id"):
            cases.append(("out->%s == frames->%s" % (o, k), ERR_ARG, dict(alias=(o, "frames", k))))
        for k in ("rgb32f", "depth", "normal", "length", "hit_id"):
            cases.append(("out->%s == history->%s" % (o, k), ERR_ARG, dict(alias=(o, "history", k))))
    cases.append(("out->length == frames->rgb32f", ERR_ARG, dict(alias=("length", "frames", "rgb32f"))))
    cases.append(("out->rgb32f == out->length", ERR_ARG, dict(alias=("length", "out", "rgb32f"))))
    cases.append(("46341 x 46341", ERR_LIMIT, dict(params=(46341, 46341, 1) + good[3:])))
    cases.append(("2 x 2 x 2^30", ERR_LIMIT, dict(params=(2, 2, 1 << 30) + good[3:])))
    # two defects in one request: the recorded text says which check comes first
    cases.append(("frames->depth NULL, out->memory = 2", ERR_ARG, dict(frames_null="depth", memory={"out": 2})))
    cases.append(("history->length NULL, res_x = 0", ERR_ARG, dict(history_null="length", params=(0,) + good[1:])))
    cases.append(("depth_tolerance = -1, out->length == frames->rgb32f", ERR_ARG, dict(params=good[:3] + (-1.0,) + good[4:], alias=("length", "frames", "rgb32f"))))
    return cases


def recorded_refusals(entry):
    """{case name: (status, p3d_last_error() text)} of the probe `entry`, as tests/golden/make_accumulate_refusals.py recorded
    them while each of the three accumulate entries still had a check function of its own."""
    with open(os.path.join(REPO, "tests", "golden", "accumulate_refusals.json")) as f:
        return {r["case"]: (r["status"], r["text"]) for r in json.load(f) if r["entry"] == entry}


def make_call(entry):
    """call(**changes) -> the status of `entry` (a function of (params, frames, history, out) pointers) on a good 5 x 3 request
    with the changes of refusal_cases() applied."""
    seq = R.make_sequence(5, 3, 1, seed=7, history=True)
    hist = seq["history"]
    out32, outl = np.zeros((3, 5, 3), F), np.zeros((3, 5), F)

    def call(params=(5, 3, 1, 0.1, 0.8, 4.0), frames=True, out=True, frames_null=None, history_null=None, out_planes=(True, True),
             memory={}, cam_res=None, hist_cam_res=None, alias=None, history=True):
        cam, hcam = (api.Camera * 1)(seq["cams"][0]), (api.Camera * 1)(hist["cam"])
        if cam_res:
            cam[0].res_x, cam[0].res_y = cam_res
        if hist_cam_res:
            hcam[0].res_x, hcam[0].res_y = hist_cam_res
        ptr = dict(frames={k: seq[k].ctypes.data for k in ("rgb32f", "depth", "normal", "hit_id")},
                   history={k: hist[k].ctypes.data for k in ("rgb32f", "depth", "normal", "length", "hit_id")},
                   out=dict(rgb32f=out32.ctypes.data if out_planes[0] else None, length=outl.ctypes.data if out_planes[1] else None))
        ptr["frames"]["cams"], ptr["history"]["cam"] = cam, hcam
        if frames_null:
            ptr["frames"][frames_null] = None
        if history_null:
            ptr["history"][history_null] = None
        if alias:
            ptr["out"][alias[0]] = ptr[alias[1]][alias[2]]
        fr = api.AccumulateFrames(*[ptr["frames"][k] for k in ("rgb32f", "depth", "normal", "hit_id", "cams")], memory.get("frames", 0))
        hi = api.AccumulateHistory(*[ptr["history"][k] for k in ("rgb32f", "depth", "normal", "length", "hit_id", "cam")], memory.get("history", 0))
        o = api.AccumulateOutputs(ptr["out"]["rgb32f"], ptr["out"]["length"], memory.get("out", 0))
        p = api.AccumulateParams(*params) if params is not None else None
        return entry(C.byref(p) if p else None, C.byref(fr) if frames else None, C.byref(hi) if history else None, C.byref(o) if out else None)

    return call


@pytest.mark.parametrize("name,status,change", refusal_cases(), ids=[c[0] for c in refusal_cases()])
def test_every_refusal_by_status_code_without_a_device(name, status, change):
    L = P.lib()
    call = make_call(lambda p, fr, hi, o: L.p3d_debug_accumulate(0, p, fr, hi, o))
    assert call(**change) == status, name
    assert L.p3d_last_error(), "every refusal has a text"
    if status == ERR_LIMIT:
        assert b"31 bits" in L.p3d_last_error()
    assert (status, L.p3d_last_error().decode()) == recorded_refusals("p3d_debug_accumulate")[name]


def test_a_null_scene_is_refused():
    L = P.lib()
    call = make_call(lambda p, fr, hi, o: L.p3d_accumulate(None, p, fr, hi, o))
    assert call() == ERR_ARG and b"scene" in L.p3d_last_error()
