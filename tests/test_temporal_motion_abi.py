"""CPU tests of the motion variant's entry points (spt_temporal_motion_async,
spt_temporal_motion): declared in include/spt_hip.h, exported by the library, bound by _native
with the declared argument types; a null context is an argument error before any device is
touched; the ABI version stays 11 (the entry points are additions); sphere_motion's table and
the Python interface's new keyword arguments.  (What the call computes:
tests/test_temporal_motion_helper.py and tests/test_gpu_temporal_motion.py.)"""
import ctypes
import inspect
import re

import numpy as np
import pytest

NAMES = ("spt_temporal_motion_async", "spt_temporal_motion")
F = np.float32
P = ctypes.c_void_p


def test_motion_entry_points_are_declared_and_exported(native):
    declared = native.declared_symbols()
    L = native.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.spt_abi_version() == native.ABI_VERSION == 11


def test_header_declares_the_signatures_bound(native):
    """The header's parameter lists, type by type, are the argtypes bound, and they are the
    plain pair's with the table and its count put in before the tolerances."""
    text = open(native.HEADER_PATH).read()
    kinds = {"uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    for name in NAMES:
        m = re.search(r"SPT_API int " + name + r"\(([^;]*)\);", text)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).replace("\n", " ").split(",")]
        want = [P if "*" in p or "[" in p else kinds[p.split()[0]] for p in params]
        fn = getattr(native.lib(), name)
        assert fn.argtypes == want, (name, params)
        assert fn.restype == ctypes.c_int
        plain = getattr(native.lib(), name.replace("_motion", "")).argtypes
        assert want == plain[:15] + [P, ctypes.c_uint32] + plain[15:], name
        assert "motion" in params[15] and params[16] == "uint32_t n_spheres"


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    n = 2
    rgba, mom = np.full((n, 4), 5.0, F), np.full((n, 4), 2.0, F)
    feat, ids = np.full((n, 8), 0.5, F), np.zeros(n, np.uint32)
    view, eye = np.eye(4, dtype=F).reshape(16), np.zeros(4, F)
    motion = np.zeros((1, 8), F)
    out, out_mom = np.full((n, 4), -7.0, F), np.full((n, 4), -8.0, F)
    p = lambda a: a.ctypes.data_as(P)  # noqa: E731
    cur = (p(rgba), p(mom), p(feat), p(ids), p(view), p(eye))
    for call in (lambda: L.spt_temporal_motion(None, 2, 1, *cur, *cur, p(motion), 1, 0.25, 0.1, 64.0, p(out), p(out_mom)),
                 lambda: L.spt_temporal_motion_async(None, 2, 1, *cur, *cur, p(motion), 1, 0.25, 0.1, 64.0, p(out), p(out_mom), None),
                 lambda: L.spt_temporal_motion(None, 0, 0, *([None] * 12), None, 0, 0.25, 0.1, 64.0, None, None)):
        assert call() == 1
        assert b"null context" in L.spt_last_error(None)
    assert (out == -7.0).all() and (out_mom == -8.0).all()


def test_sphere_motion_lays_out_this_frame_then_the_previous(native):
    import simplepathtracer_amd as spt
    assert "sphere_motion" in spt.__all__
    a = spt.init_spheres(1)
    b = spt.Scene(a.centers + F(0.25), a.radii * F(1.5), a.colors, a.materials, a.fuzz)
    t = spt.sphere_motion(b, a)
    assert t.shape == (a.n, 8) and t.dtype == F and t.flags.c_contiguous
    assert np.array_equal(t[:, 0:3], b.centers[:, :3]) and np.array_equal(t[:, 3], b.radii)
    assert np.array_equal(t[:, 4:7], a.centers[:, :3]) and np.array_equal(t[:, 7], a.radii)
    still = spt.sphere_motion(a, a)
    assert np.array_equal(still[:, :4], still[:, 4:])
    fewer = spt.Scene(a.centers[:-1], a.radii[:-1], a.colors[:-1], a.materials[:-1], a.fuzz[:-1])
    with pytest.raises(ValueError):
        spt.sphere_motion(a, fewer)
    with pytest.raises(ValueError):
        spt.sphere_motion(fewer, a)


def test_python_interface_has_the_new_keyword_arguments(native):
    import simplepathtracer_amd as spt
    par = lambda f: inspect.signature(f).parameters  # noqa: E731
    assert par(spt.Context.temporal)["motion"].default is None
    assert par(spt.Context.temporal_async)["d_motion"].default == 0 and par(spt.Context.temporal_async)["n_spheres"].default == 0
    assert par(spt.TemporalAccumulator.frame)["scene"].default is None
    assert par(spt.TemporalAccumulator.__init__)["resident"].default is False
    # the positional order of the existing arguments is what it was
    assert list(par(spt.Context.temporal))[:13] == ["self", "rgba", "mom", "feat", "ids", "view", "eye", "history", "prev_view",
                                                    "prev_eye", "tol_normal", "tol_depth", "max_history"]
    assert list(par(spt.TemporalAccumulator.frame))[:4] == ["self", "view", "eye", "denoise"]
