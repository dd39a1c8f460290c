"""tests/golden/reference_traces.npz on the CPU: the fixture tests/test_gpu_trace.py traces
on the GPU holds what the reference's own TraceAndSampleColor answered
(tests/golden/make_reference_traces.py).  Its inputs must be what the recipe regenerates,
its colours what the oracle computes (so fixture, oracle and device pin each other), and
where the reference's harness is built, what the harness answers today.  CPU tests: no GPU,
no kernel."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_reference_traces as M  # noqa: E402
from trace_rays import BOUNCES, N_PATHS, FIRST_SEEDS  # noqa: E402

PATH = os.path.join(HERE, "golden", "reference_traces.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(PATH, allow_pickle=False))


def test_fixture_holds_the_recipes_inputs(oracle, fixture):
    f = fixture
    assert sorted(f) == ["bounces", "d", "o", "rgba", "seeds"]
    _, _, o, d, seeds, bounces = M.recipe()
    n = len(o)
    assert n == N_PATHS == 1031
    assert np.array_equal(bits(f["o"]), bits(o)) and np.array_equal(bits(f["d"]), bits(d))
    assert f["seeds"].dtype == np.uint32 and np.array_equal(f["seeds"], seeds)
    assert tuple(int(s) for s in seeds[:4]) == FIRST_SEEDS
    assert np.array_equal(f["bounces"], bounces) and sorted(set(bounces.tolist())) == sorted(BOUNCES)
    assert f["rgba"].shape == (n, 4) and f["rgba"].dtype == np.float32
    assert os.path.getsize(PATH) <= os.path.getsize(os.path.join(HERE, "golden", "golden.npz"))


def test_fixture_equals_the_oracle(oracle, fixture):
    f = fixture
    sc, fr, _, _, _, _ = M.recipe()
    want, info = oracle.trace_rays(sc, fr, f["d"], f["o"], f["bounces"], f["seeds"])
    assert not info[:, 1].any(), "a path of the fixture is cut at the specular cap (the reference has no cap)"
    # no path of the mix gives a NaN colour here; if one did, its payload would still be compared
    bad = np.nonzero((bits(f["rgba"]) != bits(want)).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size} of {len(want)} paths differ; first {bad[0]}: reference {f['rgba'][bad[0]]!r}, "
                           f"oracle {want[bad[0]]!r}")
    # the fixture is live: most paths end in a finite colour that is not black, and every
    # depth has many different ones
    lit = np.isfinite(f["rgba"][:, :3]).all(axis=1) & f["rgba"][:, :3].any(axis=1)
    assert lit.sum() >= len(lit) // 2
    for b in BOUNCES:
        assert len(np.unique(bits(f["rgba"][f["bounces"] == b][:, :3]), axis=0)) >= 20, b


def test_fixture_regenerates(oracle, fixture):
    """The fixture is what the harness answers today."""
    if not oracle.ref_available():
        if os.path.isdir(oracle.REF_INCLUDE):
            pytest.fail(f"the reference's headers are in {oracle.REF_INCLUDE} but {oracle.REF_BIN} is not built")
        pytest.skip("neither the reference's headers nor oracle/_ref/ref_harness are here")
    f = fixture
    sc, _, _, _, _, _ = M.recipe()
    got = oracle.ref_trace(sc, f["d"], f["o"], f["bounces"], f["seeds"])
    assert np.array_equal(bits(got), bits(f["rgba"]))
