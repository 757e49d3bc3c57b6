"""p3d_accumulate_variance without a GPU: the host restatement (p3dh_accumulate_variance) against the NumPy restatement of
the definition (tests/accumulate_variance_reference.py), bit for bit; its colour, length and prev_xy against the entries it
extends; and the properties the moments and the two variance estimates must have."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accumulate_moving_reference as M                    # noqa: E402
import accumulate_reference as R                           # noqa: E402
import accumulate_variance_reference as RV                 # noqa: E402
import u_4a_2s_p3d_raytracer_template2_amd as P            # noqa: E402
from denoise_reference import _lum                         # noqa: E402
from test_accumulate_host import exact_camera, recorded_refusals     # noqa: E402
from u_4a_2s_p3d_raytracer_template2_amd import api        # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
KW = dict(depth_tolerance=0.1, normal_min=0.8, max_history=4.5)    # 4.5: the generated histories (lengths 1 to 6) reach the cap
KWT = (KW["depth_tolerance"], KW["normal_min"], KW["max_history"])
SPATIAL = dict(sigma_depth=0.5, normal_power_log2=2)
SHAPES = [(1, 1), (5, 3), (17, 33), (37, 23)]              # (res_x, res_y)
ERR_ARG, ERR_LIMIT = -1, -4
KEYS = ("rgb32f", "length", "moments", "variance")


def same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def static_args(seq, hit_ids=True, seed=1):
    """(rgb32f, depth, normal, cams, hit_id, history with moments) of an accumulate_reference sequence."""
    h = RV.with_moments(seq["history"], seed)
    if not hit_ids:
        h = R.without_hit_ids(h)
    return (seq["rgb32f"], seq["depth"], seq["normal"], seq["cams"], seq["hit_id"] if hit_ids else None, h)


def moving_args(seq, seed=1):
    """... and of an accumulate_moving_reference sequence, with its motion."""
    return (seq["rgb32f"], seq["depth"], seq["normal"], seq["cams"], seq["hit_id"], RV.with_moments(seq["history"], seed),
            dict(prim_type=seq["prim_type"], prim_data=seq["prim_data"]))


def reference(args, motion=None, probes=None, min_temporal=3.0, radius=3):
    return RV.accumulate_variance(*args, motion, *KWT, min_temporal, radius, SPATIAL["sigma_depth"], SPATIAL["normal_power_log2"], probes)


def assert_the_mix(probes, depth, min_temporal, n_frames, history, shape):
    """Neither estimate is vacuous, on the NumPy result alone, wherever the definition lets both occur: with min_temporal 3
    a history (lengths 1 to 6, so 2 to 4.5 after a frame) or a fourth frame (lengths 3 and 4) gives pixels on both sides.
    min_temporal 1 has no spatial pixel by definition, and two frames from nothing have no history of 3."""
    spatial = np.stack([p["spatial"] for p in probes])
    temporal = R.valid_depth(depth) & ~spatial & np.stack([p["took"] for p in probes])
    if min_temporal == 1.0:
        assert not spatial.any()
    elif shape != (1, 1):
        assert spatial.any(), "no pixel took the spatial estimate"
    if shape != (1, 1) and (min_temporal == 1.0 and (history or n_frames > 1) or min_temporal == 3.0 and (history or n_frames == 4)):
        assert temporal.any(), "no pixel with a history took the temporal variance"


@pytest.mark.parametrize("min_temporal", [1.0, 3.0])
@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("hit_ids", [True, False])
@pytest.mark.parametrize("history", [False, True])
@pytest.mark.parametrize("n_frames", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_equals_the_numpy_restatement(shape, n_frames, history, hit_ids, radius, min_temporal):
    seq = R.make_sequence(*shape, n_frames, seed=n_frames, history=history)
    args = static_args(seq, hit_ids)
    probes = []
    ref = reference(args, None, probes, min_temporal, radius)
    got = api.host_accumulate_variance(*args, min_temporal=min_temporal, radius=radius, **KW, **SPATIAL)
    assert "prev_xy" not in got
    for k in KEYS:
        same_bits(got[k], ref[k], k)
    assert_the_mix(probes, seq["depth"], min_temporal, n_frames, history, shape)
    assert (ref["variance"] >= 0).all() and (ref["variance"][~R.valid_depth(seq["depth"])] == 0).all()


@pytest.mark.parametrize("history", [False, True])
@pytest.mark.parametrize("n_frames", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_equals_the_numpy_restatement_through_moved_primitives(shape, n_frames, history):
    seq = M.make_sequence(*shape, n_frames, seed=n_frames, history=history)
    args = moving_args(seq)
    probes = []
    ref = reference(args[:6], args[6], probes)
    got = api.host_accumulate_variance(*args, min_temporal=3.0, radius=3, **KW, **SPATIAL)
    for k in KEYS + ("prev_xy",):
        same_bits(got[k], ref[k], k)
    assert_the_mix(probes, seq["depth"], 3.0, n_frames, history, shape)


@pytest.mark.parametrize("hit_ids", [True, False])
@pytest.mark.parametrize("history", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_colour_and_length_are_those_of_p3dh_accumulate(shape, history, hit_ids):
    seq = R.make_sequence(*shape, 4, seed=3, history=history)
    args = static_args(seq, hit_ids)
    got = api.host_accumulate_variance(*args, min_temporal=3.0, radius=1, **KW, **SPATIAL)
    ref = api.host_accumulate(*args, **KW)
    same_bits(got["rgb32f"], ref["rgb32f"], "rgb32f")
    same_bits(got["length"], ref["length"], "length")
    assert (ref["length"] > 1).any() or shape == (1, 1) and not history


@pytest.mark.parametrize("history", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_colour_length_and_prev_xy_are_those_of_p3dh_accumulate_moving(shape, history):
    seq = M.make_sequence(*shape, 4, seed=3, history=history)
    got = api.host_accumulate_variance(*moving_args(seq), min_temporal=3.0, radius=1, **KW, **SPATIAL)
    ref = api.host_accumulate_moving(*M.args(seq), **KW)
    for k in ("rgb32f", "length", "prev_xy"):
        same_bits(got[k], ref[k], k)


def test_frame_0_without_a_spatial_estimate():
    """No history: out_m = m = (l, l * l), and the temporal variance l * l - l * l is 0 at every pixel."""
    seq = R.make_sequence(37, 23, 1, seed=2)
    got = api.host_accumulate_variance(*static_args(seq), min_temporal=1.0, radius=3, **KW, **SPATIAL)
    assert (got["variance"] == 0).all()
    lum = _lum(seq["rgb32f"])
    same_bits(got["moments"], np.stack([lum, lum * lum], -1).astype(F), "moments")
    # with the estimate switched on, frame 0 has a variance wherever a pixel has a neighbour
    est = api.host_accumulate_variance(*static_args(seq), min_temporal=2.0, radius=3, **KW, **SPATIAL)
    same_bits(est["moments"], got["moments"], "the estimate does not touch the moments")
    valid = R.valid_depth(seq["depth"])
    assert (est["variance"][valid] > 0).mean() > 0.9 and (est["variance"][~valid] == 0).all()


@pytest.mark.parametrize("max_history", [32.0, 4.0])
def test_a_static_sequence_carries_the_running_moments(max_history):
    """The camera and depth of test_a_static_sequence_averages_and_counts: every pixel reprojects onto its own centre exactly,
    one tap carries weight 1, so Hm = (0 + 1 * M') / 1 = M' and the moments after frame f are the sequential recurrence
    m_f = m_{f-1} + (m - m_{f-1}) * alpha, alpha = 1 / len -- the definition's product with alpha, where a division by len
    would round differently -- evaluated here in float32."""
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
    got = api.host_accumulate_variance(c, z, nr, [cam] * n, None, None, min_temporal=1.0, radius=1, **kw, **SPATIAL)
    hit = np.isfinite(z[0])
    m = RV.moments_of(c)
    run = m[0].copy()
    for f in range(n):
        if f:
            length = F(min(f + 1, max_history))
            assert (got["length"][f][hit] == length).all()
            run = np.where(hit[..., None], run + (m[f] - run) * (F(1) / length), m[f]).astype(F)
        same_bits(got["moments"][f], run, "moments after frame %d" % f)
        vt = run[..., 1] - run[..., 0] * run[..., 0]
        same_bits(got["variance"][f], np.where(hit, np.where(vt > 0, vt, F(0)), F(0)).astype(F), "variance after frame %d" % f)
    # 8 independent samples of noise 0.1 per channel: the variance of the luminance is that of the samples' luminance
    if max_history == 32.0:
        sample = _lum(c)[:, hit].astype(np.float64).var(0)
        assert np.abs(got["variance"][7][hit] - sample).max() < 1e-5


def test_the_spatial_estimate_measures_the_noise():
    """A flat grey wall under noise of standard deviation s per channel: the luminance has variance
    (0.2126^2 + 0.7152^2 + 0.0722^2) s^2 = 0.5619 s^2.  With radius 3 an interior pixel weighs 49 samples equally; the
    mean of the estimates over 30 x 20 pixels lies within 10 % of that times 48 / 49 (they overlap, so this is loose)."""
    w, h, s = 30, 20, 0.1
    rng = np.random.default_rng(5)
    c = (F(0.5) + rng.normal(size=(1, h, w, 3)).astype(F) * F(s)).astype(F)
    z = np.full((1, h, w), 4.0, F)
    nr = np.zeros((1, h, w, 3), F)
    nr[..., 2] = 1.0
    got = api.host_accumulate_variance(c, z, nr, [R.look_at((0, 0, 5), (0, 0, 0), w, h)], None, None, min_temporal=2.0, radius=3, **KW, **SPATIAL)
    inner = got["variance"][0, 3:-3, 3:-3]
    expected = 0.5619 * s * s * 48 / 49
    assert abs(float(inner.mean()) / expected - 1) < 0.1, (float(inner.mean()), expected)


@pytest.mark.parametrize("moving", [False, True])
def test_one_call_equals_frame_by_frame_with_the_outputs_fed_back(moving):
    make = M.make_sequence if moving else R.make_sequence
    seq = make(37, 23, 4, seed=5, history=True)
    args = moving_args(seq) if moving else static_args(seq) + (None,)
    kw = dict(min_temporal=3.0, radius=3, **KW, **SPATIAL)
    whole = api.host_accumulate_variance(*args, **kw)
    h = args[5]
    for f in range(4):
        motion = dict(prim_type=seq["prim_type"], prim_data=seq["prim_data"][f]) if moving else None
        one = api.host_accumulate_variance(seq["rgb32f"][f], seq["depth"][f], seq["normal"][f], seq["cams"][f], seq["hit_id"][f], h, motion, **kw)
        for k in KEYS + (("prev_xy",) if moving else ()):
            same_bits(one[k].reshape(whole[k][f].shape), whole[k][f], "frame %d %s" % (f, k))
        h = dict(rgb32f=one["rgb32f"], length=one["length"], moments=one["moments"], depth=seq["depth"][f], normal=seq["normal"][f],
                 cam=seq["cams"][f], hit_id=seq["hit_id"][f])
        if moving:
            h["prim_data"] = seq["prim_data"][f]


def test_outputs_that_are_not_wanted_change_nothing():
    """The planes the caller leaves out are still carried from frame to frame."""
    seq = R.make_sequence(17, 33, 4, seed=6, history=True)
    args = static_args(seq)
    p, vp, fr, hi, hm, mo, out, keep = api._accumulate_variance_request(*args, None, min_temporal=3.0, radius=3, **KW, **SPATIAL)
    whole = api.host_accumulate_variance(*args, min_temporal=3.0, radius=3, **KW, **SPATIAL)
    for k in KEYS:
        only = np.zeros_like(whole[k])
        P.lib().p3dh_accumulate_variance(C.byref(p), C.byref(vp), C.byref(fr), C.byref(hi), hm, None,
                                         *[only.ctypes.data if j == k else None for j in api._VARIANCE_PLANES])
        same_bits(only, whole[k], "%s alone" % k)


# ---- the interface
def refusal_cases():
    """(name, expected status, keyword changes of call()) for every refusal p3d_accumulate_variance adds to its siblings', and
    the siblings' own through this entry."""
    good, vgood = (5, 3, 1, 0.1, 0.8, 4.0), (3.0, 3, 0.5, 2)
    cases = [("params NULL", ERR_ARG, dict(params=None)), ("variance_params NULL", ERR_ARG, dict(vparams=None)),
             ("frames NULL", ERR_ARG, dict(frames=False)), ("out NULL", ERR_ARG, dict(out=False))]
    for k in ("rgb32f", "depth", "normal", "cams"):
        cases.append(("frames->%s NULL" % k, ERR_ARG, dict(frames_null=k)))
    for k in ("rgb32f", "depth", "normal", "length", "cam"):
        cases.append(("history->%s NULL" % k, ERR_ARG, dict(history_null=k)))
    cases.append(("history without history_moments", ERR_ARG, dict(moments=False)))
    cases.append(("history_moments without history", ERR_ARG, dict(history=False)))
    cases.append(("every output NULL", ERR_ARG, dict(out_planes=())))
    cases.append(("prev_xy without a motion", ERR_ARG, dict(out_planes=("rgb32f", "prev_xy"))))
    cases.append(("motion without frames->hit_id", ERR_ARG, dict(motion=True, frames_null="hit_id")))
    cases.append(("motion->prim_data NULL", ERR_ARG, dict(motion=True, motion_null="prim_data")))
    cases.append(("motion->history_prim_data NULL", ERR_ARG, dict(motion=True, motion_null="history_prim_data")))
    for bad in ((0, 3, 1), (5, 0, 1), (5, 3, 0), (-5, 3, 1)):
        cases.append(("shape %s" % (bad,), ERR_ARG, dict(params=bad + good[3:])))
    for field, values in ((3, (0.0, -1.0, np.inf, np.nan)), (4, (-1.5, 1.5, np.nan, np.inf)), (5, (0.5, 0.0, -2.0, np.inf, np.nan))):
        for v in values:
            cases.append(("params[%d] = %r" % (field, v), ERR_ARG, dict(params=good[:field] + (v,) + good[field + 1:])))
    for field, values in ((0, (0.5, 0.0, -1.0, np.inf, np.nan)), (1, (0, 4, -1)), (2, (0.0, -1.0, np.inf, np.nan)), (3, (-1, 9))):
        for v in values:
            cases.append(("variance_params[%d] = %r" % (field, v), ERR_ARG, dict(vparams=vgood[:field] + (v,) + vgood[field + 1:])))
    for where in ("frames", "history", "out"):
        for v in (2, -1):
            cases.append(("%s->memory = %d" % (where, v), ERR_ARG, dict(memory={where: v})))
    for o in ("moments", "variance"):
        for k in ("rgb32f", "depth", "normal", "hit_id"):
            cases.append(("out->%s == frames->%s" % (o, k), ERR_ARG, dict(alias=(o, "frames", k))))
        for k in ("rgb32f", "depth", "normal", "length", "hit_id", "moments"):
            cases.append(("out->%s == history->%s" % (o, k), ERR_ARG, dict(alias=(o, "history", k))))
        for k in ("prim_type", "prim_data", "history_prim_data"):
            cases.append(("out->%s == motion->%s" % (o, k), ERR_ARG, dict(motion=True, alias=(o, "motion", k))))
        for k in ("rgb32f", "length"):
            cases.append(("out->%s == out->%s" % (o, k), ERR_ARG, dict(alias=(o, "out", k))))
    cases.append(("out->variance == out->moments", ERR_ARG, dict(alias=("variance", "out", "moments"))))
    cases.append(("out->prev_xy == out->moments", ERR_ARG, dict(motion=True, alias=("prev_xy", "out", "moments"))))
    for o in ("rgb32f", "length"):
        cases.append(("out->%s == history_moments" % o, ERR_ARG, dict(alias=(o, "history", "moments"))))
        cases.append(("out->%s == history->depth" % o, ERR_ARG, dict(alias=(o, "history", "depth"))))
    cases.append(("out->length == frames->rgb32f", ERR_ARG, dict(alias=("length", "frames", "rgb32f"))))
    cases.append(("46341 x 46341", ERR_LIMIT, dict(params=(46341, 46341, 1) + good[3:])))
    cases.append(("2 x 2 x 2^30", ERR_LIMIT, dict(params=(2, 2, 1 << 30) + good[3:])))
    # two defects in one request: the recorded text says which check comes first
    cases.append(("frames->depth NULL, out->memory = 2", ERR_ARG, dict(frames_null="depth", memory={"out": 2})))
    cases.append(("history->length NULL, res_x = 0", ERR_ARG, dict(history_null="length", params=(0,) + good[1:])))
    cases.append(("depth_tolerance = -1, out->length == frames->rgb32f", ERR_ARG, dict(params=good[:3] + (-1.0,) + good[4:], alias=("length", "frames", "rgb32f"))))
    cases.append(("radius = 9, out->moments == frames->depth", ERR_ARG, dict(vparams=(3.0, 9, 0.5, 2), alias=("moments", "frames", "depth"))))
    cases.append(("history without history_moments, min_temporal = 0.5", ERR_ARG, dict(moments=False, vparams=(0.5,) + vgood[1:])))
    # a new plane wanted alone is also held to the rules of colour, length and prev_xy, before the variance params are looked at
    cases.append(("only out->moments, == frames->depth, radius = 9", ERR_ARG, dict(out_planes=("moments",), vparams=(3.0, 9, 0.5, 2), alias=("moments", "frames", "depth"))))
    cases.append(("only out->variance, == frames->rgb32f", ERR_ARG, dict(out_planes=("variance",), alias=("variance", "frames", "rgb32f"))))
    return cases


def accepted_cases():
    """(name, keyword changes of call()): requests for one of the new planes and nothing else, which pass every check although
    the siblings' rule "every output plane is NULL" would refuse the planes they know."""
    return [("only out->%s%s" % (k, ", with a motion" if motion else ""), dict(out_planes=(k,), motion=motion, prev_xy=False))
            for k in ("moments", "variance") for motion in (False, True)]


def make_call(entry):
    """call(**changes) -> the status of `entry` (a function of the seven pointers after the scene or device) on a good 5 x 3
    request with the changes of refusal_cases() applied."""
    seq = M.make_sequence(5, 3, 1, seed=7, history=True)
    hist = RV.with_moments(seq["history"])
    outs = dict(rgb32f=np.zeros((3, 5, 3), F), length=np.zeros((3, 5), F), moments=np.zeros((3, 5, 2), F), variance=np.zeros((3, 5), F),
                prev_xy=np.zeros((3, 5, 2), F))

    def call(params=(5, 3, 1, 0.1, 0.8, 4.0), vparams=(3.0, 3, 0.5, 2), frames=True, out=True, history=True, moments=True, motion=False,
             frames_null=None, history_null=None, motion_null=None, out_planes=("rgb32f", "length", "moments", "variance"), memory={},
             alias=None, prev_xy=None):
        cam, hcam = (api.Camera * 1)(seq["cams"][0]), (api.Camera * 1)(hist["cam"])
        ptr = dict(frames={k: seq[k].ctypes.data for k in ("rgb32f", "depth", "normal", "hit_id")},
                   history={k: hist[k].ctypes.data for k in ("rgb32f", "depth", "normal", "length", "hit_id", "moments")},
                   motion=dict(prim_type=seq["prim_type"].ctypes.data, prim_data=seq["prim_data"].ctypes.data,
                               history_prim_data=hist["prim_data"].ctypes.data),
                   out={k: outs[k].ctypes.data if k in out_planes or (k == "prev_xy" and (motion if prev_xy is None else prev_xy)) else None for k in api._VARIANCE_PLANES})
        ptr["frames"]["cams"], ptr["history"]["cam"] = cam, hcam
        for group, name in (("frames", frames_null), ("history", history_null), ("motion", motion_null)):
            if name:
                ptr[group][name] = None
        if alias:
            ptr["out"][alias[0]] = ptr[alias[1]][alias[2]]
        fr = api.AccumulateFrames(*[ptr["frames"][k] for k in ("rgb32f", "depth", "normal", "hit_id", "cams")], memory.get("frames", 0))
        hi = api.AccumulateHistory(*[ptr["history"][k] for k in ("rgb32f", "depth", "normal", "length", "hit_id", "cam")], memory.get("history", 0))
        mo = api.AccumulateMotion(4, *[ptr["motion"][k] for k in ("prim_type", "prim_data", "history_prim_data")], 0)
        o = api.AccumulateVarianceOutputs(*[ptr["out"][k] for k in api._VARIANCE_PLANES], memory.get("out", 0))
        p = api.AccumulateParams(*params) if params is not None else None
        vp = api.AccumulateVarianceParams(*vparams) if vparams is not None else None
        return entry(C.byref(p) if p else None, C.byref(vp) if vp else None, C.byref(fr) if frames else None, C.byref(hi) if history else None,
                     ptr["history"]["moments"] if moments else None, C.byref(mo) if motion else None, C.byref(o) if out else None)

    return call


@pytest.mark.parametrize("name,status,change", refusal_cases(), ids=[c[0] for c in refusal_cases()])
def test_every_refusal_by_status_code_without_a_device(name, status, change):
    L = P.lib()
    call = make_call(lambda *a: L.p3d_debug_accumulate_variance(0, *a))
    assert call(**change) == status, name
    assert L.p3d_last_error(), "every refusal has a text"
    if status == ERR_LIMIT:
        assert b"31 bits" in L.p3d_last_error()
    assert (status, L.p3d_last_error().decode()) == recorded_refusals("p3d_debug_accumulate_variance")[name]


@pytest.mark.parametrize("name,change", accepted_cases(), ids=[c[0] for c in accepted_cases()])
def test_a_request_for_a_new_plane_alone_is_accepted(name, change):
    """Accepted means that the probe goes on to look for a device: P3D_OK where one is visible, P3D_ERR_NO_DEVICE where none
    is -- a refused request returns its own status and text before that."""
    L = P.lib()
    call = make_call(lambda *a: L.p3d_debug_accumulate_variance(0, *a))
    rc, text = call(**change), L.p3d_last_error().decode()
    if P.device_count() > 0:
        assert rc == 0, (name, text)
    else:
        assert (rc, text) == (-3, "no HIP device visible") == recorded_refusals("p3d_debug_accumulate_variance")[name]


def test_a_null_scene_is_refused():
    L = P.lib()
    call = make_call(lambda *a: L.p3d_accumulate_variance(None, *a))
    assert call() == ERR_ARG and b"scene" in L.p3d_last_error()


def test_the_symbols_are_exported_declared_and_listed():
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH]).decode()
    for name in ("p3d_accumulate_variance", "p3d_debug_accumulate_variance", "p3dh_accumulate_variance"):
        assert re.search(r"\bT %s$" % name, dyn, re.M), "libp3d_hip.so does not export " + name
        assert hasattr(P.lib(), name)
    header = open(os.path.join(REPO, "include", "p3d_hip.h")).read()
    assert re.search(r"\bint p3d_accumulate_variance\(p3d_scene\* scene, const p3d_accumulate_params\* params, "
                     r"const p3d_accumulate_variance_params\* variance_params,", header)
    assert re.search(r"\bint p3d_debug_accumulate_variance\(int device, const p3d_accumulate_params\* params,", header)
    assert "} p3d_accumulate_variance_params;" in header and "} p3d_accumulate_variance_outputs;" in header
    assert "p3d_accumulate_variance" in api.C_ABI_SYMBOLS and "p3d_debug_accumulate_variance" in api.C_ABI_SYMBOLS
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4\b", header) and P.lib().p3d_abi_version() == 4
    assert C.sizeof(api.AccumulateVarianceParams) == 16 and api.AccumulateVarianceParams.normal_power_log2.offset == 12
    assert C.sizeof(api.AccumulateVarianceOutputs) == 48 and api.AccumulateVarianceOutputs.memory.offset == 40
    for name in ("accumulate_variance", "accumulate_variance_device"):
        assert hasattr(P.DeviceScene, name)
    assert api.VARIANCE_MIN_TEMPORAL >= 1 and 1 <= api.VARIANCE_RADIUS <= 3 and api.VARIANCE_SIGMA_DEPTH == api.DENOISE_SIGMA_DEPTH
