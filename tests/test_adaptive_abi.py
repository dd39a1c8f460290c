"""CPU tests of the adaptive-sampling entry points (spt_render_adaptive[_dev]): declared in
include/spt_hip.h, exported by the library, bound by _native with the declared argument
types; a null context is an argument error before any device is touched.  The ABI version
stays 11: the entry points are additions.  (What they compute: tests/test_adaptive_helper.py
and tests/test_gpu_adaptive.py.)"""
import ctypes
import re

NAMES = ("spt_render_adaptive", "spt_render_adaptive_dev")


def test_adaptive_entry_points_are_declared_and_exported(native):
    declared = native.declared_symbols()
    L = native.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.spt_abi_version() == native.ABI_VERSION == 11


def test_header_declares_the_signatures_bound(native):
    """The header's parameter lists, type by type, are the argtypes bound."""
    text = open(native.HEADER_PATH).read()
    kinds = {"uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    counts = {}
    for name in NAMES:
        m = re.search(r"SPT_API int " + name + r"\(([^;]*)\);", text)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).replace("\n", " ").split(",")]
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        fn = getattr(native.lib(), name)
        assert fn.argtypes == want, (name, params)
        assert fn.restype == ctypes.c_int
        counts[name] = len(want)
    assert counts == {"spt_render_adaptive": 14, "spt_render_adaptive_dev": 15}


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    out = (ctypes.c_float * 8)(*([-7.0] * 8))
    mom = (ctypes.c_float * 8)(*([2.0] * 8))
    g = (ctypes.c_uint8 * 6)(*([0xAB] * 6))
    info = (ctypes.c_uint64 * 2)(5, 6)
    for call in (lambda: L.spt_render_adaptive(None, 0, 1, 0, 2, 8, 8, 64, 0.08, 1.0, out, g, mom, info),
                 lambda: L.spt_render_adaptive_dev(None, 0, 1, 0, 2, 8, 8, 64, 0.08, 1.0, out, g, mom, info, None),
                 lambda: L.spt_render_adaptive(None, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, None, None, None, None)):
        assert call() == 1
        assert b"null" in L.spt_last_error(None)
    assert list(out) == [-7.0] * 8 and list(g) == [0xAB] * 6 and list(mom) == [2.0] * 8 and list(info) == [5, 6]


def test_python_interface_has_adaptive_sampling(native):
    import inspect

    import simplepathtracer_amd as spt
    for name in ("render_adaptive", "render_adaptive_dev", "render_denoised"):
        assert callable(getattr(spt.Context, name)), name
    for name in ("render_adaptive", "render_adaptive_dev"):
        p = inspect.signature(getattr(spt.Context, name)).parameters
        assert (p["base_spp"].default, p["step_spp"].default, p["max_spp"].default) == (8, 8, 64), name
        assert (p["tol"].default, p["lum_floor"].default) == (0.08, 1.0), name
    p = inspect.signature(spt.Context.render_denoised).parameters
    assert p["variance"].default is False and p["adaptive"].default is None
