"""CPU tests of the feature-buffer entry points (spt_render_features,
spt_render_features_async): declared in include/spt_hip.h, exported by the library, bound
by _native with the declared argument types, and a null context is an argument error before
any device is touched.  The ABI version stays 11: the entry points are additions.
(What the buffers hold: tests/test_gpu_features.py.)"""
import ctypes

NAMES = ("spt_render_features", "spt_render_features_async")


def test_feature_entry_points_are_declared_and_exported(native):
    declared = native.declared_symbols()
    L = native.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.spt_abi_version() == native.ABI_VERSION == 11


def test_native_binds_the_feature_signatures(native):
    L = native.lib()
    P, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert L.spt_render_features.argtypes == [P, u32, u32, u32, u32, P, P]
    assert L.spt_render_features_async.argtypes == [P, u32, u32, u32, u32, u32, u32, u32, P, P, P]
    for name in NAMES:
        assert getattr(L, name).restype == ctypes.c_int


def test_header_declares_the_signatures_bound(native):
    """The header's parameter lists, type by type, are the argtypes bound."""
    import re
    text = open(native.HEADER_PATH).read()
    kinds = {"uint32_t": ctypes.c_uint32}
    for name in NAMES:
        m = re.search(r"SPT_API int " + name + r"\(([^;]*)\);", text)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).replace("\n", " ").split(",")]
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert getattr(native.lib(), name).argtypes == want, (name, params)


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    feat = (ctypes.c_float * 16)(*([-7.0] * 16))
    ids = (ctypes.c_uint32 * 2)(0xABABABAB, 0xABABABAB)
    for call in (lambda: L.spt_render_features(None, 0, 1, 0, 2, feat, ids),
                 lambda: L.spt_render_features_async(None, 0, 1, 1, 1, 0, 0, 2, feat, ids, None),
                 lambda: L.spt_render_features(None, 0, 0, 0, 0, None, None)):
        assert call() == 1
        assert b"null" in L.spt_last_error(None)
    assert list(feat) == [-7.0] * 16 and list(ids) == [0xABABABAB] * 2


def test_python_interface_has_the_feature_buffers(native):
    import simplepathtracer_amd as spt
    for name in ("render_features", "render_features_async", "feature_buffers"):
        assert callable(getattr(spt.Context, name)), name
    assert callable(spt.Context.id_buffer)
