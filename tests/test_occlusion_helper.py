"""The occlusion contract against the oracle alone, on the CPU (tests/occlusion.py;
DESIGN.md §4.17).

The contract is stated as "the closest hit has ds < L".  Here it is shown to BE any-hit: on
the golden 149-sphere scene and the 4099 adversarial rays of the cast tests, with
make_limits' mixed limits, it equals a brute force over every sphere with
pyoracle.probe_sphere -- some sphere passes RaySphereIntersection, lies ahead and has
ds < L.  (This scene only: the stress scenes would take 10^8 probes.)  The oracle's answers
must also show the limit classes are live, and the segment restatement must agree with the
ray form on (a, normalize(b - a), lensq(b - a) * scale).
"""
import numpy as np
import pytest

from occlusion import FLT_MAX, contract, make_limits, restate_segments


@pytest.fixture(scope="module")
def side(oracle, native, golden_scenes):
    """The cast tests' oracle answers on the golden scene (computed once, shared with
    tests/test_gpu_occlusion.py when both run) and every sphere's probe of every ray."""
    import simplepathtracer_amd as spt
    from test_gpu_cast import oracle_side
    w = oracle_side(oracle, spt, golden_scenes, "random")
    s, osc, o, d = w["scene"], w["osc"], w["o"], w["d"]
    n = len(o)
    passes, ahead = np.zeros((n, s.n), bool), np.zeros((n, s.n), bool)
    ds = np.zeros((n, s.n), np.float32)
    for i in range(n):
        for j in range(s.n):
            passes[i, j], ds[i, j], ahead[i, j] = oracle.probe_sphere(osc, j, d[i], o[i])
    return dict(w=w, passes=passes, ahead=ahead, ds=ds)


def brute_any_hit(side, L, rows=None):
    p, a, ds = side["passes"], side["ahead"], side["ds"]
    if rows is not None:
        p, a, ds = p[rows], a[rows], ds[rows]
    with np.errstate(invalid="ignore"):
        return (p & a & (ds < np.asarray(L, np.float32)[:, None])).any(axis=1)


def test_the_contract_is_any_hit(side):
    w = side["w"]
    n_spheres = w["scene"].n
    hit, ds = w["hit"], w["want"][:, 1, 3]
    L, cls = make_limits(ds, hit)
    want = contract(w["idx"], ds, L, n_spheres)
    assert np.array_equal(want, brute_any_hit(side, L))
    # the closest hit's ds is the least passing, ahead ds: what makes the two the same
    cand = np.where(side["passes"] & side["ahead"], side["ds"], np.float32(np.inf))
    assert np.array_equal(cand.min(axis=1)[hit], ds[hit]) and np.isinf(cand.min(axis=1)[~hit]).all()
    # liveness, from the oracle's answers
    for c, answer in ((3, False), (4, True), (5, False)):
        m = (cls == c) & hit
        assert m.sum() >= 100, (c, m.sum())
        assert (want[m] == answer).all(), c
    m = (cls == 6) & hit
    assert 0.2 <= want[m].mean() <= 0.8, want[m].mean()
    assert 0.25 <= want.mean() <= 0.75, want.mean()
    assert want[(cls == 1) & hit].all() and want[(cls == 2) & hit].all() and want[(cls == 8) & hit].all()
    assert not want[cls == 7].any() and not want[~hit].any()
    assert min(len(np.unique(cls[k:k + 64])) for k in range(0, len(cls) - 64, 64)) >= 6, "every wave mixes the classes"


def test_limit_edge_values(side):
    w = side["w"]
    n_spheres = w["scene"].n
    hit, ds, n = w["hit"], w["want"][:, 1, 3], len(w["hit"])
    full = lambda v: np.full(n, v, np.float32)
    for v in (np.nan, 0.0, -0.0, -1.0, -np.inf):
        assert not contract(w["idx"], ds, full(v), n_spheres).any(), v
        assert not brute_any_hit(side, full(v)).any(), v
    for v in (np.inf, FLT_MAX):
        assert np.array_equal(contract(w["idx"], ds, full(v), n_spheres), hit), v
        assert np.array_equal(brute_any_hit(side, full(v)), hit), v
    assert not contract(w["idx"], ds, ds, n_spheres).any(), "L == ds: the compare is strict"
    assert ds[hit].max() < FLT_MAX


def test_segments_restate_the_ray_form(oracle, side):
    w = side["w"]
    s, osc, o, d, hit, kind = w["scene"], w["osc"], w["o"], w["d"], w["hit"], w["kind"]
    t = w["want"][:, 0, 3]
    # unit directions, finite, and long enough that b - a keeps the direction to 1e-5
    rows = np.nonzero(hit & np.isin(kind, ("A", "B")) & (t > 0.1))[0][:240]
    assert len(rows) == 240
    a = o[rows]
    f = np.float32

    def answers(b, scale):
        so, sd, L = restate_segments(a, b, scale)
        assert np.array_equal(so, a)
        v = (b[:, :3] - a[:, :3]).astype(f)
        vv = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(f)
        assert np.array_equal(L.view(np.uint32), (vv * f(scale)).view(np.uint32))
        with np.errstate(all="ignore"):
            unit = (v / np.sqrt(vv)[:, None]).astype(f)
        assert np.array_equal(sd[:, :3].view(np.uint32), unit.view(np.uint32)) and not sd[:, 3].any()
        idx = np.array([oracle.find_closest(osc, sd[i], so[i]) for i in range(len(a))], np.uint32)
        ds = np.array([oracle.probe_sphere(osc, min(int(j), s.n - 1), sd[i], so[i])[1] for i, j in enumerate(idx)], f)
        want = contract(idx, ds, L, s.n)
        # and it is any-hit on the restated ray
        for i in range(0, len(a), 8):
            brute = False
            for j in range(s.n):
                p, dsj, ahead = oracle.probe_sphere(osc, j, sd[i], so[i])
                brute = brute or (p and ahead and dsj < L[i])
            assert brute == want[i]
        return want, L

    half, _ = answers((a + d[rows] * (f(0.5) * t[rows])[:, None]).astype(f), 1.0)
    # (b - a rounds, so the restated direction differs from d by up to 1e-5: a grazing ray
    # may change its answer; the others cannot)
    assert half.mean() <= 0.05, "nothing lies before the closest hit"
    far_b = (a + d[rows] * (f(1.5) * t[rows])[:, None]).astype(f)
    far, L1 = answers(far_b, 1.0)
    assert far.mean() >= 0.95, "the closest hit lies within 1.5 t"
    _, Ls = answers(far_b, 0.25)
    assert np.array_equal(Ls, L1 * f(0.25))
    same, L0 = answers(a.copy(), 1.0)  # a == b: L = 0, the answer 0 whatever normalize(0) is
    assert not L0.any() and not same.any()
