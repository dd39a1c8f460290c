"""Normalize on the device with its one-branch range guard (spt_device.h): the short path
runs straight-line for every lane and the full IEEE sequences sit behind one wave-uniform
branch, kept only by the lanes whose components are out of range.  Through the hook
tests/cpp/spt_normalize_hook.hip (libspt_normhook.so, one element per lane, so the test
decides which lanes share a wave) the result must equal the plain form a / sqrtf(lensq(a))
bit for bit in every lane: against the same form compiled for the device (NaN bits
included) and against numpy's float32 (NaN matches NaN).

Inputs: every triple over the edge values of tests/cpp/normalize_guard_check.cpp; 2^20 random
in-range triples (waves in which no lane needs the full sequences); and waves of in-range
lanes in which exactly one lane, at each of the 64 positions, holds an out-of-range triple.
Run on an MI355X with `pytest -m gpu`."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import math_sweep as ms

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simplepathtracer_amd", "lib",
                   "libspt_normhook.so")
LO, HI = 0x2B800000, 0x53800000  # 2^-40, 2^40
EDGE_BITS = (0, 1, 0x007FFFFF, LO - 1, LO, LO + 1, HI - 1, HI, HI + 1, 0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x7F800001,
             0x3F800000)


def edge_values():
    b = np.array(EDGE_BITS, np.uint32)
    return ms.f32(np.concatenate([b, b | ms.SIGN]))


def in_range(rng, n):
    """n triples with every component in [2^-40, 2^40], either sign, any mantissa."""
    exp = rng.integers(-40, 40, size=(n, 3))
    mant = rng.integers(0, 1 << 23, size=(n, 3), dtype=np.uint32)
    sign = rng.integers(0, 2, size=(n, 3), dtype=np.uint32)
    v = ms.f32(ms.pack(exp, mant, sign))
    assert ms.operand_ok(v).all()
    return v


@pytest.fixture(scope="module")
def run():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(LIB):
        raise ImportError(f"{LIB} is missing: build it with `make -C simplepathtracer_amd/csrc`")
    L = ctypes.CDLL(LIB)
    P = ctypes.c_void_p
    L.spt_hook_normalize.argtypes = [P, P, P, ctypes.c_uint32, P, ctypes.c_int]
    L.spt_hook_normalize.restype = ctypes.c_int

    def normalize(v, plain):
        d = [torch.from_numpy(np.ascontiguousarray(v[:, k]).view(np.int32)).cuda() for k in range(3)]
        out = torch.empty(3 * v.shape[0], dtype=torch.int32, device="cuda")
        assert L.spt_hook_normalize(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), v.shape[0], out.data_ptr(),
                                    1 if plain else 0) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32).reshape(-1, 3)

    return normalize


def check(run, v, what):
    got, plain = run(v, False), run(v, True)
    bad = np.nonzero((got != plain).any(1))[0]
    assert not bad.size, (f"{what}: {bad.size} of {v.shape[0]} lanes differ from the device's a / sqrtf(lensq(a)); first at "
                          f"{int(bad[0])} (lane {int(bad[0]) % 64}): {[float(c).hex() for c in v[bad[0]]]} got "
                          f"{[hex(int(c)) for c in got[bad[0]]]} want {[hex(int(c)) for c in plain[bad[0]]]}")
    bad = ms.mismatches(got, ms.expected_normalize(v[:, 0], v[:, 1], v[:, 2]))
    assert not bad.size, f"{what}: {bad.size} results differ from numpy's; first at element {int(bad[0]) // 3}"


def test_edge_triples(run):
    e = edge_values()
    v = np.array(list(itertools.product(e, e, e)), np.float32)
    assert v.shape == (28 ** 3, 3)
    check(run, v, "edge triples")


def test_no_lane_needs_the_full_sequences(run):
    v = in_range(np.random.default_rng(ms.SEED), 1 << 20)
    check(run, v, "in-range triples")


def test_exactly_one_lane_needs_the_full_sequences(run):
    """64 waves per out-of-range triple: the triple in lane w of wave w, in-range lanes around it."""
    rng = np.random.default_rng(ms.SEED + 1)
    e = edge_values()
    outside = np.array([t for t in itertools.product(e[~ms.operand_ok(e)], ms.f32(np.uint32([0x3F800000, HI])),
                                                     ms.f32(np.uint32([LO, 0xBF800000])))], np.float32)
    # the out-of-range component in each of the three positions
    outside = np.concatenate([outside, outside[:, [1, 0, 2]], outside[:, [1, 2, 0]]])
    v = in_range(rng, outside.shape[0] * 64 * 64).reshape(outside.shape[0], 64, 64, 3)
    for w in range(64):
        v[:, w, w] = outside
    v = v.reshape(-1, 3)
    slow = ~ms.operand_ok(v).all(1)
    assert (slow.reshape(-1, 64).sum(1) == 1).all()
    check(run, v, "one out-of-range lane per wave")
