"""CPU tests of the temporal accumulation's entry points (spt_temporal_inverse,
spt_temporal_async, spt_temporal): declared in include/spt_hip.h, exported by the library,
bound by _native with the declared argument types; a null context is an argument error
before any device is touched; spt_temporal_inverse, which is host only, against numpy.  The
ABI version stays 11: the entry points are additions.  (What the accumulation computes:
tests/test_temporal_helper.py and tests/test_gpu_temporal.py.)"""
import ctypes
import re

import numpy as np

NAMES = ("spt_temporal_inverse", "spt_temporal_async", "spt_temporal")
F = np.float32
P = ctypes.c_void_p


def test_temporal_entry_points_are_declared_and_exported(native):
    declared = native.declared_symbols()
    L = native.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.spt_abi_version() == native.ABI_VERSION == 11


def test_header_declares_the_signatures_bound(native):
    """The header's parameter lists, type by type, are the argtypes bound (an array parameter
    is a pointer)."""
    text = open(native.HEADER_PATH).read()
    kinds = {"uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    counts = {}
    for name in NAMES:
        m = re.search(r"SPT_API int " + name + r"\(([^;]*)\);", text)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).replace("\n", " ").split(",")]
        want = [P if "*" in p or "[" in p else kinds[p.split()[0]] for p in params]
        fn = getattr(native.lib(), name)
        assert fn.argtypes == want, (name, params)
        assert fn.restype == ctypes.c_int
        counts[name] = len(want)
    assert counts == {"spt_temporal_inverse": 2, "spt_temporal_async": 21, "spt_temporal": 20}


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    n = 2
    rgba, mom = np.full((n, 4), 5.0, F), np.full((n, 4), 2.0, F)
    feat, ids = np.full((n, 8), 0.5, F), np.zeros(n, np.uint32)
    view, eye = np.eye(4, dtype=F).reshape(16), np.zeros(4, F)
    out, out_mom = np.full((n, 4), -7.0, F), np.full((n, 4), -8.0, F)
    p = lambda a: a.ctypes.data_as(P)  # noqa: E731
    cur = (p(rgba), p(mom), p(feat), p(ids), p(view), p(eye))
    hist = (p(rgba), p(mom), p(feat), p(ids), p(view), p(eye))
    for call in (lambda: L.spt_temporal(None, 2, 1, *cur, *hist, 0.25, 0.1, 64.0, p(out), p(out_mom)),
                 lambda: L.spt_temporal_async(None, 2, 1, *cur, *hist, 0.25, 0.1, 64.0, p(out), p(out_mom), None),
                 lambda: L.spt_temporal(None, 0, 0, *([None] * 12), 0.25, 0.1, 64.0, None, None)):
        assert call() == 1
        assert b"null context" in L.spt_last_error(None)
    assert (out == -7.0).all() and (out_mom == -8.0).all()


def inverse(native, view16):
    v = np.ascontiguousarray(view16, F).reshape(16)
    out = np.full(9, -3.0, F)
    rc = native.lib().spt_temporal_inverse(v.ctypes.data_as(P), out.ctypes.data_as(P))
    return rc, out.reshape(3, 3)


def ulps(a, b):
    """The distance of two finite float32 arrays in units in the last place."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def blocks():
    """camera_basis-shaped matrices, and random 3x3 blocks of condition number below 100."""
    r = np.random.default_rng(11)
    out = []
    for _ in range(40):  # orthonormal bases, as camera_basis builds them, turned at random
        q, _ = np.linalg.qr(r.normal(size=(3, 3)))
        out.append(q)
    while len(out) < 240:
        m = r.uniform(-2, 2, (3, 3))
        if np.linalg.cond(m.astype(F).astype(np.float64)) < 100:
            out.append(m)
    return out


def test_inverse_is_numpys_rounded_once(native):
    """Computed in double and rounded once per entry: within 1 fp32 ulp of np.linalg.inv in
    float64 rounded to fp32 (the two double results differ by far less than an fp32 ulp, so
    their roundings are neighbours at worst)."""
    import simplepathtracer_amd as spt
    mats = blocks()
    basis = np.asarray(spt.camera_basis([0, 1, -3, 0], [0, 1, 0, 0], [0, 1, 0, 0]), F).reshape(4, 4)[:3, :3]
    basis2 = np.asarray(spt.camera_basis([0.15, 1.05, -2.9, 0], [0.3, 0.9, 0.1, 0], [0, 1, 0, 0]), F).reshape(4, 4)[:3, :3]
    worst = 0
    for m in [basis, basis2] + mats:
        v = np.zeros((4, 4), F)
        v[:3, :3] = m
        rc, got = inverse(native, v)
        assert rc == 0
        want = np.linalg.inv(v[:3, :3].astype(np.float64)).astype(F)
        d = ulps(got, want)
        assert (d <= 1).all(), (m, got, want)
        worst = max(worst, int(d.max()))
    print(f"spt_temporal_inverse: {len(mats) + 2} matrices, worst distance {worst} ulp")
    assert np.array_equal(spt.temporal_inverse(np.eye(4, dtype=F)), np.eye(3, dtype=F))


def test_inverse_ignores_row_3_and_column_3(native):
    r = np.random.default_rng(5)
    v = np.zeros((4, 4), F)
    v[:3, :3] = blocks()[50]
    rc, base = inverse(native, v)
    assert rc == 0
    w = v.copy()
    w[3, :] = r.normal(size=4)
    w[:, 3] = [np.nan, np.inf, -1e30, 7.0]
    rc, got = inverse(native, w)
    assert rc == 0 and np.array_equal(got.view(np.uint32), base.view(np.uint32))


def test_inverse_argument_errors(native):
    L = native.lib()
    good = np.eye(4, dtype=F)
    singular = good.copy()
    singular[2, :3] = singular[0, :3]  # two equal rows
    zero = np.zeros((4, 4), F)
    for bad, at in ((np.nan, (1, 1)), (np.inf, (0, 2)), (-np.inf, (2, 0))):
        m = good.copy()
        m[at] = bad
        rc, out = inverse(native, m)
        assert rc == 1 and (out == -3.0).all(), bad
    for m in (singular, zero):
        rc, out = inverse(native, m)
        assert rc == 1 and (out == -3.0).all()
        assert b"inverse" in L.spt_last_error(None)
    out = np.zeros(9, F)
    assert L.spt_temporal_inverse(None, out.ctypes.data_as(P)) == 1
    assert L.spt_temporal_inverse(good.ctypes.data_as(P), None) == 1


def test_python_interface_has_the_accumulation(native):
    import simplepathtracer_amd as spt
    for name in ("temporal", "temporal_async"):
        assert callable(getattr(spt.Context, name)), name
    assert callable(spt.temporal_inverse) and callable(spt.TemporalAccumulator)
    for name in ("frame", "reset"):
        assert callable(getattr(spt.TemporalAccumulator, name)), name
