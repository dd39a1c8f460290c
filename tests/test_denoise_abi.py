"""CPU tests of the denoiser's entry points (spt_denoise_scratch_bytes, spt_denoise_async,
spt_denoise): declared in include/spt_hip.h, exported by the library, bound by _native with
the declared argument types; a null context is an argument error before any device is
touched; the scratch size is the layout the header states, min(levels - 1, 2) float4 planes.
The ABI version stays 11: the entry points are additions.  (What the filter computes:
tests/test_denoise_helper.py and tests/test_gpu_denoise.py.)"""
import ctypes

import pytest

NAMES = ("spt_denoise_scratch_bytes", "spt_denoise_async", "spt_denoise")


def test_denoise_entry_points_are_declared_and_exported(native):
    declared = native.declared_symbols()
    L = native.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.spt_abi_version() == native.ABI_VERSION == 11


def test_native_binds_the_denoise_signatures(native):
    L = native.lib()
    P, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    assert L.spt_denoise_scratch_bytes.argtypes == [u32, u32, u32, P]
    assert L.spt_denoise_async.argtypes == [P, u32, u32, P, P, f32, f32, f32, f32, u32, P, P, P, P]
    assert L.spt_denoise.argtypes == [P, u32, u32, P, P, f32, f32, f32, f32, u32, P, P]
    for name in NAMES:
        assert getattr(L, name).restype == ctypes.c_int


def test_header_declares_the_signatures_bound(native):
    """The header's parameter lists, type by type, are the argtypes bound."""
    import re
    text = open(native.HEADER_PATH).read()
    kinds = {"uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    for name in NAMES:
        m = re.search(r"SPT_API int " + name + r"\(([^;]*)\);", text)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).replace("\n", " ").split(",")]
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
        assert getattr(native.lib(), name).argtypes == want, (name, params)


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    rgba = (ctypes.c_float * 8)(*([5.0] * 8))
    feat = (ctypes.c_float * 16)(*([0.5] * 16))
    out = (ctypes.c_float * 8)(*([-7.0] * 8))
    g = (ctypes.c_uint8 * 6)(*([0xAB] * 6))
    scratch = (ctypes.c_float * 16)(*([-9.0] * 16))
    for call in (lambda: L.spt_denoise(None, 2, 1, rgba, feat, 30.0, 0.1, 0.25, 0.5, 3, out, g),
                 lambda: L.spt_denoise_async(None, 2, 1, rgba, feat, 30.0, 0.1, 0.25, 0.5, 3, out, g, scratch, None),
                 lambda: L.spt_denoise(None, 0, 0, None, None, 30.0, 0.1, 0.25, 0.5, 3, None, None)):
        assert call() == 1
        assert b"null" in L.spt_last_error(None)
    assert list(out) == [-7.0] * 8 and list(g) == [0xAB] * 6 and list(scratch) == [-9.0] * 16


@pytest.mark.parametrize("shape", [(1, 1), (45, 37), (1200, 800)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_scratch_bytes_are_the_ping_pong_planes(native, shape):
    """Level 0 reads the caller's rgba and the last level writes the caller's outputs: one
    level needs no scratch, two need one float4 plane, more need two."""
    L = native.lib()
    W, H = shape
    plane = W * H * 16
    got = {}
    for levels in range(1, 9):
        b = ctypes.c_uint64(0xDEAD)
        assert L.spt_denoise_scratch_bytes(W, H, levels, ctypes.byref(b)) == 0, levels
        got[levels] = b.value
    assert got[1] == 0 and got[2] == plane
    assert all(got[k] == 2 * plane for k in range(3, 9)), got
    assert got[5] == 2 * plane


def test_scratch_bytes_argument_errors(native):
    L = native.lib()
    b = ctypes.c_uint64(0xDEAD)
    for levels in (0, 9):
        assert L.spt_denoise_scratch_bytes(45, 37, levels, ctypes.byref(b)) == 1, levels
        assert b"levels" in L.spt_last_error(None)
    assert L.spt_denoise_scratch_bytes(65536, 32768, 3, ctypes.byref(b)) == 1  # 2^31 pixels
    assert L.spt_denoise_scratch_bytes(45, 37, 3, None) == 1
    assert b.value == 0xDEAD
    # an empty image needs none; the largest image fits the 64-bit count
    assert L.spt_denoise_scratch_bytes(0, 37, 3, ctypes.byref(b)) == 0 and b.value == 0
    assert L.spt_denoise_scratch_bytes(65535, 32768, 8, ctypes.byref(b)) == 0 and b.value == 2 * 65535 * 32768 * 16


def test_python_interface_has_the_denoiser(native):
    import simplepathtracer_amd as spt
    for name in ("denoise", "denoise_async", "render_denoised"):
        assert callable(getattr(spt.Context, name)), name
    assert spt.denoise_scratch_bytes(45, 37, 1) == 0
    assert spt.denoise_scratch_bytes(45, 37, 5) == 2 * 45 * 37 * 16
    with pytest.raises(spt.SptError):
        spt.denoise_scratch_bytes(45, 37, 0)
