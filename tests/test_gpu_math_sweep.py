"""The device's exact fp32 primitives over their whole domains.

spt_device.h, spt_powf.h and spt_decode.h shorten a few IEEE operations by hand (division
without div_scale / div_fixup, a square root without the scaled path, Normalize built from
both, the uniform draw as one FMA, glibc's powf as the device compiler builds it, the
refraction decision, the fold's halvings as one multiply, the pixel byte).  Every kernel
goes through them, and a frame only ever shows them a few million operands of a narrow
distribution.  Here each one runs alone (tests/cpp/spt_mathsweep.hip, built with the
product's flags) against its literal definition: the unary ones over all 2^32 input
patterns against the host (oracle/spt_oracle.c spo_math_*), compared as one 64-bit digest
per block of 2^20 patterns; division, Normalize and the halvings over the operand sets of
tests/math_sweep.py against numpy.  No comparison has a tolerance.  The negative controls
(the raw v_sqrt_f32, a * v_rcp_f32(b)) must fail the same comparisons: the sets can tell
a result that is one ulp off.

Nothing is sampled: every op's host pass over 2^32 patterns is affordable (HOST_SECONDS
prints what each took).  Run on an MI355X with `pytest -m gpu`.
"""
import ctypes
import os
import time

import numpy as np
import pytest

import math_sweep as ms

pytestmark = pytest.mark.gpu

ALL = 1 << 32
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simplepathtracer_amd", "lib",
                   "libspt_mathsweep.so")
HOST_SECONDS = {}  # op -> seconds of the host's pass over 2^32 patterns


class Sweep:
    """ctypes binding of libspt_mathsweep.so over torch's allocations (null stream)."""

    def __init__(self, torch):
        if not os.path.exists(LIB):
            raise ImportError(f"{LIB} is missing: build it with `make -C simplepathtracer_amd/csrc`")
        self.torch = torch
        L = self.L = ctypes.CDLL(LIB)
        P, I, u32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
        L.spt_sweep_digest.argtypes = [I, u32, u64, P, P]
        L.spt_sweep_dump.argtypes = [I, u32, u64, P]
        L.spt_sweep_div.argtypes = [P, P, u64, P, P, P]
        L.spt_sweep_normalize.argtypes = [P, P, P, u64, P]
        L.spt_sweep_halve.argtypes = [P, P, u64, P]
        for fn in (L.spt_sweep_digest, L.spt_sweep_dump, L.spt_sweep_div, L.spt_sweep_normalize, L.spt_sweep_halve):
            fn.restype = I

    def _up(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()

    def _out(self, n):
        return self.torch.empty(n, dtype=self.torch.int32, device="cuda")

    def _down(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint32)

    def digest(self, op, first=0, count=ALL):
        d = self.torch.empty((count + ms.BLOCK - 1) // ms.BLOCK, dtype=self.torch.int64, device="cuda")
        assert self.L.spt_sweep_digest(ms.OPS[op], first, count, d.data_ptr(), None) == 0, op
        self.torch.cuda.synchronize()
        return d.cpu().numpy().view(np.uint64)

    def dump(self, op, first, count):
        out = self._out(count)
        assert self.L.spt_sweep_dump(ms.OPS[op], first, count, out.data_ptr()) == 0, op
        return self._down(out)

    def div(self, a, b):
        da, db = self._up(a, np.int32), self._up(b, np.int32)
        rn, core, raw = self._out(a.size), self._out(a.size), self._out(a.size)
        assert self.L.spt_sweep_div(da.data_ptr(), db.data_ptr(), a.size, rn.data_ptr(), core.data_ptr(),
                                    raw.data_ptr()) == 0
        return self._down(rn), self._down(core), self._down(raw)

    def normalize(self, x, y, z):
        dx, dy, dz = (self._up(c, np.int32) for c in (x, y, z))
        out = self._out(3 * x.size)
        assert self.L.spt_sweep_normalize(dx.data_ptr(), dy.data_ptr(), dz.data_ptr(), x.size, out.data_ptr()) == 0
        return self._down(out).reshape(-1, 3)

    def halve(self, x, j):
        dx, dj = self._up(x, np.int32), self._up(j, np.int32)
        out = self._out(x.size)
        assert self.L.spt_sweep_halve(dx.data_ptr(), dj.data_ptr(), x.size, out.data_ptr()) == 0
        return self._down(out)


@pytest.fixture(scope="module")
def dev(oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Sweep(torch)


@pytest.fixture(scope="module")
def host(oracle):
    """The host's digests over all 2^32 patterns, computed once per op."""
    memo = {}

    def digests(op):
        if op not in memo:
            t = time.perf_counter()
            memo[op] = oracle.math_digest(ms.OPS[op], 0, ALL)
            HOST_SECONDS[op] = time.perf_counter() - t
            print(f"host pass {op}: {HOST_SECONDS[op]:.2f} s")
        return memo[op]

    return digests


def assert_blocks(dev, oracle, op, got, want, first=0, want_op=None):
    """Digests `got` of device op `op` over [first, first + BLOCK * len(got)) against the
    host's `want` (of host op `want_op`); on a mismatch, dump the first differing block
    from both sides and name the first differing input."""
    bad = np.nonzero(got != want)[0]
    if not bad.size:
        return
    at = (first + int(bad[0]) * ms.BLOCK) & 0xFFFFFFFF
    g = dev.dump(op, at, ms.BLOCK)
    w = oracle.math_block(ms.OPS[want_op or op], at, ms.BLOCK)
    diff = np.nonzero(g != w)[0]
    if not diff.size:
        raise AssertionError(f"{op}: digest of block {at:#010x} differs ({int(got[bad[0]]):#x} vs "
                             f"{int(want[bad[0]]):#x}) but its dump equals the host's: the digest kernel is wrong")
    i = int(diff[0])
    raise AssertionError(f"{op}: {bad.size} of {got.size} blocks differ; first differing input {at + i:#010x}: "
                         f"got {int(g[i]):#010x} want {int(w[i]):#010x} ({diff.size} inputs differ in that block)")


# ---------------------------------------------------------------- unary ops

@pytest.mark.parametrize("op", ms.HOST_OPS)
def test_exhaustive(dev, host, oracle, op):
    """Every op that has a literal host definition, over all 2^32 input patterns: sqrtf,
    glibc's powf(x, 5.f), spo_uniform_u32 on the three ranges, the refraction scalar in
    both directions, the pixel byte and the byte conversion.  NaN results are canonical on
    both sides."""
    if op == "REFR_GA":
        # both outcomes of no_tir occur for glass -> air, from the host's answers: cosines
        # on both sides of the critical angle (c^2 = 5/9)
        r = oracle.math_block(ms.OPS[op], 0x3F380000, ms.BLOCK)
        tir = r == ms.u32(np.float32(-1e30))[0]
        assert tir.any() and not tir.all()
    assert_blocks(dev, oracle, op, dev.digest(op), host(op))


# sqrt_pos_normal's stated domain (spt_device.h): [2^-96, +inf].  2^-96 starts a block and
# the blocks end with FLT_MAX; +inf goes through the dump form.
POS_FIRST, POS_END, INF = 0x0F800000, 0x7F800000, 0x7F800000


def test_sqrt_pos_normal_over_its_domain(dev, host, oracle):
    want = host("SQRT")[POS_FIRST >> 20:POS_END >> 20]
    got = dev.digest("SQRT_POS", POS_FIRST, POS_END - POS_FIRST)
    assert_blocks(dev, oracle, "SQRT_POS", got, want, first=POS_FIRST, want_op="SQRT")
    # the two ends through the dump form
    for first, count in ((POS_FIRST, 4), (INF - 3, 4)):
        assert np.array_equal(dev.dump("SQRT_POS", first, count), oracle.math_block(ms.OPS["SQRT"], first, count)), \
            hex(first)


def test_raw_sqrt_is_told_apart(dev, host):
    """Liveness: v_sqrt_f32 alone (<= 1 ulp) does not pass where sqrt_pos_normal does."""
    got = dev.digest("SQRT_RAW", POS_FIRST, POS_END - POS_FIRST)
    assert (got != host("SQRT")[POS_FIRST >> 20:POS_END >> 20]).any()


def test_sqrt_at_a_quarter(dev):
    """spt_device.h: `sqrtf(L) < 0.5f` <=> `L < 0.25f` (coop_ball_vector), because sqrt is
    monotone, sqrt(0.25) == 0.5 and sqrt(prev(0.25)) < 0.5."""
    quarter, half = 0x3E800000, 0x3F000000
    for op in ("SQRT", "SQRT_POS"):
        below, at = dev.dump(op, quarter - 1, 2)
        assert int(at) == half and int(below) < half, op


# ---------------------------------------------------------------- division

# pairs with both operands inside div_operand_ok, per set
GATED = {"div_grid": 6563844, "div_hard": 655360, "div_full": 102758, "div_primary": 1397412,
         "div_recip_hard": 117030}


def describe(a, b, got, want, i):
    return (f"first at {i}: {float(a[i]).hex()} / {float(b[i]).hex()}: got {int(got[i]):#010x} "
            f"want {int(ms.u32(want)[i]):#010x}")


@pytest.mark.parametrize("name", list(ms.DIV_SETS))
def test_division(dev, name):
    """div_rn equals IEEE division on every pair; the ungated core div_core(a, recip(b))
    equals it wherever both operands pass div_operand_ok, and for divisors up to 2^42 as
    the header states; a * v_rcp_f32(b) does not (liveness, on the sets made to be hard)."""
    a, b = ms.DIV_SETS[name]()
    want = ms.expected_div(a, b)
    rn, core, raw = dev.div(a, b)
    bad = ms.mismatches(rn, want)
    assert not bad.size, f"div_rn on {name}: {bad.size} of {a.size} differ; " + describe(a, b, rn, want, int(bad[0]))
    gated = ms.operand_ok(a) & ms.operand_ok(b)
    assert int(gated.sum()) == GATED[name]
    assert GATED["div_grid"] * 2 > ms.DIV_SIZES["div_grid"] and GATED["div_hard"] == ms.DIV_SIZES["div_hard"]
    bad_core = ms.mismatches(core, want)
    inside = bad_core[gated[bad_core]]
    assert not inside.size, (f"div_core on {name}: {inside.size} of {GATED[name]} gated pairs differ; "
                             + describe(a, b, core, want, int(inside[0])))
    # the divisor range spt_device.h states for the core, |b| up to 2^42: normalize's
    # divisor sqrt(|v|^2) reaches sqrt(3) * 2^40 with no gate of its own
    ab = np.abs(b)
    stated = ms.operand_ok(a) & (ab >= ms.GATE_LO) & (ab <= np.float32(2.0 ** 42))
    beyond = bad_core[stated[bad_core]]
    assert not beyond.size, (f"div_core on {name}: {beyond.size} pairs with |b| in (2^40, 2^42] differ; "
                             + describe(a, b, core, want, int(beyond[0])))
    bad_raw = ms.mismatches(raw, want)
    print(f"{name}: {a.size} pairs, {GATED[name]} inside the gate; outside it the ungated core differs on "
          f"{bad_core.size} of {a.size - GATED[name]}; a * rcp(b) differs on {int(gated[bad_raw].sum())} inside")
    if name in ("div_grid", "div_hard", "div_recip_hard"):
        assert gated[bad_raw].any(), f"{name} cannot tell a * rcp(b) from a / b: strengthen the generator"


# ---------------------------------------------------------------- Normalize, halvings

def test_normalize(dev):
    x, y, z = ms.normalize_grid()
    want = ms.expected_normalize(x, y, z)
    got = dev.normalize(x, y, z)
    bad = ms.mismatches(got, want)
    if bad.size:
        i = int(bad[0]) // 3
        raise AssertionError(f"Normalize: {bad.size} of {3 * x.size} lanes differ; first at {i}: "
                             f"({float(x[i]).hex()}, {float(y[i]).hex()}, {float(z[i]).hex()}): got "
                             f"{[hex(int(v)) for v in got[i]]} want {[hex(int(v)) for v in ms.u32(want[i])]}")


def test_halve_n(dev):
    x, j, want = ms.halve_grid()
    got = dev.halve(x, j)
    bad = ms.mismatches(got, want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"halve_n: {bad.size} of {x.size} differ; first at {i}: {float(x[i]).hex()} halved "
                             f"{int(j[i])} times: got {int(got[i]):#010x} want {int(ms.u32(want)[i]):#010x}")
