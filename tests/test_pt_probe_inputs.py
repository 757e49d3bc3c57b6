"""CPU checks of the path-tracer probe inputs (tests/pt_probe_cases.py): the cases the GPU tests compare are not trivial,
and the oracle alone stays inside the cap on cases left out for sitting on a branch.  No GPU."""
import numpy as np

from oracle import oracle_py as O
import pt_probe_cases as K


def test_the_hit_world_cases_are_rays_a_frame_can_produce():
    c = K.hit_world_cases()
    _, cls, rough = O.pt_small_spheres()
    d = c["d"].astype(np.float64)
    dd = (d * d).sum(axis=1)
    # unit length to float32 rounding, or unit + rough * v with |v| <= 1 and rough <= the scene's largest
    assert (np.abs(np.sqrt(dd) - 1.0) <= float(rough.max()) + 1e-6).all()
    fuzzy = np.abs(dd - 1.0) > 1e-6
    assert set(np.unique(c["group"][fuzzy])) <= {c["names"].index(n) for n in c["names"] if "fuzzy" in n}
    assert (np.linalg.norm(c["o"].astype(np.float64), axis=1) <= 40.0 + 10.0 * np.sqrt(2)).all()
    assert len(c["seed"]) % 64 == 0 and np.isfinite(c["o"]).all() and np.isfinite(c["d"]).all()
    # the scene does hold fuzzy metals whose rays can come within 1e-3 of unit length without being unit length
    assert (rough[cls == 3] < 0.05).any()


def test_the_hit_world_cases_are_not_trivial():
    c, ref = K.hit_world_cases(), K.hit_world_reference()
    _, cls, _ = O.pt_small_spheres()
    act = c["active"] == 1
    hit = (ref["hit"] == 1) & act
    prim = ref["prim"]
    for k in range(6):
        assert int((hit & (prim == k)).sum()) >= 20, "fixed primitive %d" % k
    small = hit & (prim >= 6)
    small_cls = cls[np.clip(prim - 6, 0, 99)]
    for k in range(5):
        assert int((small & (small_cls == k)).sum()) >= 20, "small-sphere class %d" % k
    assert int((small & (small_cls == 0)).sum()) >= 100
    assert (ref["hit"][act] == 0).mean() >= 0.10
    assert (~act).sum() >= 64
    # every cell of the field that holds a sphere is the closest hit of some case
    assert set(np.unique(prim[small] - 6)) == set(np.flatnonzero(cls >= 0))
    # the same-ray group really is one ray
    s = c["same_ray"]
    for k in ("o", "d", "time", "tmin", "tmax", "seed"):
        assert (c[k][s] == c[k][s[0]]).all()
    assert len(s) == 64 and len(set(s // 64)) == 64 and len(set(s % 64)) == 64


def test_scatter_and_lighting_cases_cover_every_branch_inside_the_cap():
    ray, rec, sd, light = K.record_cases()
    sc, dl = K.scatter_reference(), K.lighting_reference()
    assert (sc["branch"] >= 0).all() and (dl["lit"] >= 0).all()          # float and high-precision variants drew alike
    for b, name in enumerate(K.BRANCHES):
        assert int(((sc["branch"] == b) & (sc["margin"] >= K.MARGIN_CAP)).sum()) >= 50, name
    for mt in (K.MT_DIFFUSE, K.MT_METAL, K.MT_GLASS):
        m = rec["mat_type"] == mt
        assert m.sum() >= 200
        assert (sc["margin"][m] < K.MARGIN_CAP).mean() <= K.LEFT_OUT_CAP, ("scatter", mt, (sc["margin"][m] < K.MARGIN_CAP).mean())
        assert (dl["margin"][m] < K.MARGIN_CAP).mean() <= K.LEFT_OUT_CAP, ("lighting", mt, (dl["margin"][m] < K.MARGIN_CAP).mean())
        for lit in (0, 1, 2):
            assert int(((dl["lit"] == lit) & m).sum()) >= 20, (mt, lit)
    # the high-precision variant is the same function: it differs from the float one by float rounding only
    ok = sc["margin"] >= K.MARGIN_CAP
    assert np.abs(sc["hp_d"][ok] - sc["d"][ok]).max() < 1e-4 and np.abs(sc["hp_atten"][ok] - sc["atten"][ok]).max() < 1e-5
    assert np.abs(sc["hp_o"][ok] - sc["o"][ok]).max() < 1e-5
    okl = dl["margin"] >= K.MARGIN_CAP
    assert np.abs(dl["hp_rgb"][okl] - dl["rgb"][okl]).max() < 1e-4
