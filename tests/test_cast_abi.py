"""CPU tests of the ray-query entry points (spt_cast_rays, spt_cast_rays_async,
spt_primary_hits): declared in include/spt_hip.h, exported by the library, bound by
_native, and a null context is an argument error before any device is touched.  The ABI
version stays 11: the entry points are additions.  (What they compute: tests/test_gpu_cast.py.)"""
import ctypes

NAMES = ("spt_cast_rays_async", "spt_cast_rays", "spt_primary_hits")


def test_cast_entry_points_are_declared_and_exported(native):
    declared = native.declared_symbols()
    L = native.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.spt_abi_version() == native.ABI_VERSION == 11


def test_native_binds_the_cast_signatures(native):
    L = native.lib()
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert L.spt_cast_rays_async.argtypes == [P, P, P, u32, P, P, P]
    assert L.spt_cast_rays.argtypes == [P, P, P, u32, P, P]
    assert L.spt_primary_hits.argtypes == [P, P, u32, P, P, P]
    for name in NAMES:
        assert getattr(L, name).restype == ctypes.c_int


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    buf = (ctypes.c_float * 8)()
    idx = (ctypes.c_uint32 * 3)()
    for call in (lambda: L.spt_cast_rays(None, buf, buf, 1, idx, None),
                 lambda: L.spt_cast_rays_async(None, buf, buf, 1, idx, None, None),
                 lambda: L.spt_primary_hits(None, idx, 1, idx, None, None),
                 lambda: L.spt_cast_rays(None, None, None, 0, None, None)):
        assert call() == 1
        assert b"null" in L.spt_last_error(None)
    assert list(idx) == [0, 0, 0]


def test_python_interface_has_the_ray_queries(native):
    from simplepathtracer_amd.renderer import Context
    for name in ("cast_rays", "cast_rays_async", "primary_hits", "id_buffer"):
        assert callable(getattr(Context, name)), name
