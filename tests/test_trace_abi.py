"""CPU tests of the path-query entry points (spt_trace_rays, spt_trace_rays_async,
spt_sample_state): declared in include/spt_hip.h, exported by the library, bound by
_native, and a null context is an argument error before any device is touched.  The ABI
version stays 11: the entry points are additions.  spt_sample_state needs no device: it is
pinned here against the oracle's keyed stream (spo_sample_key, spo_next_u32).
(What the traces compute: tests/test_gpu_trace.py.)"""
import ctypes

import numpy as np

NAMES = ("spt_trace_rays_async", "spt_trace_rays", "spt_sample_state")
# (seed, pixel, sample): small values, the extremes of every field, a frame's last pixel
KEYS = ((0, 0, 0), (1, 0, 0), (1, 5, 3), (77, 799 * 1200 + 1199, 11), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF),
        (1 << 63, 1 << 31, 1 << 31), (0x9E3779B97F4A7C15, 0xFFFFFFFF, 0), (3, 0, 0xFFFFFFFF))


def _state(L, seed, pixel, sample, draws):
    st = ctypes.c_uint64(0)
    assert L.spt_sample_state(seed, pixel, sample, draws, ctypes.byref(st)) == 0
    return st.value


def test_trace_entry_points_are_declared_and_exported(native):
    declared = native.declared_symbols()
    L = native.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.spt_abi_version() == native.ABI_VERSION == 11


def test_native_binds_the_trace_signatures(native):
    L = native.lib()
    P, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    assert L.spt_trace_rays_async.argtypes == [P, P, P, P, u32, u32, P, P, P]
    assert L.spt_trace_rays.argtypes == [P, P, P, P, u32, u32, P, P]
    assert L.spt_sample_state.argtypes == [u64, u32, u32, u32, P]
    for name in NAMES:
        assert getattr(L, name).restype == ctypes.c_int


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    buf = (ctypes.c_float * 8)()
    st = (ctypes.c_uint64 * 1)()
    info = (ctypes.c_uint32 * 2)()
    for call in (lambda: L.spt_trace_rays(None, buf, buf, st, 1, 4, buf, info),
                 lambda: L.spt_trace_rays_async(None, buf, buf, st, 1, 4, buf, info, None),
                 lambda: L.spt_trace_rays(None, None, None, None, 0, 4, None, None)):
        assert call() == 1
        assert b"null" in L.spt_last_error(None)
    assert list(buf) == [0.0] * 8 and list(info) == [0, 0]
    assert L.spt_sample_state(1, 2, 3, 0, None) == 1


def test_sample_state_is_the_oracles_sample_key(native, oracle):
    L, O = native.lib(), oracle.lib()
    for seed, pixel, sample in KEYS:
        assert _state(L, seed, pixel, sample, 0) == O.spo_sample_key(seed, pixel, sample), (seed, pixel, sample)


def test_sample_state_after_k_draws_is_where_the_oracle_stream_stands(native, oracle):
    L, O = native.lib(), oracle.lib()
    for seed, pixel, sample in KEYS:
        st = ctypes.c_uint64(O.spo_sample_key(seed, pixel, sample))
        for k in range(1, 8):
            O.spo_next_u32(ctypes.byref(st))
            assert _state(L, seed, pixel, sample, k) == st.value, (seed, pixel, sample, k)
    # a large draw count wraps like the 64-bit counter
    st = O.spo_sample_key(5, 6, 7)
    assert _state(L, 5, 6, 7, 0xFFFFFFFF) == (st + 0xFFFFFFFF * 0x9E3779B97F4A7C15) % (1 << 64)


def test_python_sample_state_is_vectorised_and_equal(native):
    import simplepathtracer_amd as spt
    L = native.lib()
    for seed, pixel, sample in KEYS:
        for k in (0, 2, 7):
            assert spt.sample_state(seed, pixel, sample, k) == _state(L, seed, pixel, sample, k)
    px = np.arange(6, dtype=np.uint32).reshape(2, 3) * 1000003
    got = spt.sample_state(9, px, 4, 2)
    assert got.dtype == np.uint64 and got.shape == (2, 3)
    assert [int(v) for v in got.ravel()] == [_state(L, 9, int(p), 4, 2) for p in px.ravel()]
    got = spt.sample_state(9, 12, np.arange(5), np.arange(5))
    assert [int(v) for v in got] == [_state(L, 9, 12, s, s) for s in range(5)]


def test_python_interface_has_the_path_queries(native):
    import simplepathtracer_amd as spt
    for name in ("trace_rays", "trace_rays_async"):
        assert callable(getattr(spt.Context, name)), name
    assert callable(spt.sample_state) and "sample_state" in spt.__all__
