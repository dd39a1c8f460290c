"""CPU tests of the sample-moments and variance-guided-denoiser entry points
(spt_render_moments[_async], spt_denoise_var[_async]): declared in include/spt_hip.h, exported
by the library, bound by _native with the declared argument types; a null context is an
argument error before any device is touched.  The ABI version stays 11: the entry points are
additions.  (What they compute: tests/test_moments_helper.py and tests/test_gpu_moments.py.)"""
import ctypes
import re

NAMES = ("spt_render_moments", "spt_render_moments_async", "spt_denoise_var_async", "spt_denoise_var")


def test_moments_entry_points_are_declared_and_exported(native):
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
    assert counts == {"spt_render_moments": 8, "spt_render_moments_async": 12, "spt_denoise_var_async": 17,
                      "spt_denoise_var": 15}


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    rgba = (ctypes.c_float * 8)(*([5.0] * 8))
    feat = (ctypes.c_float * 16)(*([0.5] * 16))
    mom = (ctypes.c_float * 8)(*([2.0] * 8))
    out = (ctypes.c_float * 8)(*([-7.0] * 8))
    var = (ctypes.c_float * 2)(*([-8.0] * 2))
    g = (ctypes.c_uint8 * 6)(*([0xAB] * 6))
    scratch = (ctypes.c_float * 16)(*([-9.0] * 16))
    S = (4.0, 0.1, 0.25, 0.5, 1.0)
    for call in (lambda: L.spt_render_moments(None, 0, 1, 0, 2, out, g, mom),
                 lambda: L.spt_render_moments_async(None, 0, 1, 1, 1, 0, 0, 2, out, g, mom, None),
                 lambda: L.spt_denoise_var(None, 2, 1, rgba, feat, mom, *S, 3, out, g, var),
                 lambda: L.spt_denoise_var_async(None, 2, 1, rgba, feat, mom, *S, 3, out, g, var, scratch, None),
                 lambda: L.spt_denoise_var(None, 0, 0, None, None, None, *S, 3, None, None, None)):
        assert call() == 1
        assert b"null" in L.spt_last_error(None)
    assert list(out) == [-7.0] * 8 and list(g) == [0xAB] * 6 and list(scratch) == [-9.0] * 16
    assert list(var) == [-8.0] * 2 and list(mom) == [2.0] * 8


def test_python_interface_has_the_moments(native):
    import inspect

    import simplepathtracer_amd as spt
    for name in ("render_moments", "render_moments_async", "denoise_variance", "denoise_variance_async", "render_denoised"):
        assert callable(getattr(spt.Context, name)), name
    p = inspect.signature(spt.Context.denoise_variance).parameters
    assert (p["sigma_color"].default, p["var_floor"].default, p["levels"].default) == (4.0, 1.0, 3)
    assert p["variance"].default is False and p["g_data"].default is False
    assert inspect.signature(spt.Context.render_denoised).parameters["variance"].default is False
