"""The exact-primitive sweeps' own tools, checked without a GPU: the operand generators and
references of tests/math_sweep.py, and the host side of the unary sweeps
(oracle/spt_oracle.c spo_math_block / spo_math_digest), which tests/test_gpu_math_sweep.py
holds the device against."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import math_sweep as ms

SPECIAL_DRAWS = [0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF, 0x80000000]  # test_device_numerics_match_host's
# one block of 2^20 input patterns per op, where the op does something: roots and powers
# around 1, draws around the clamp at 2^32, cosines below 1 (glass -> air: across the
# critical angle), colours below 255, and bytes around 255 -> 256
OP_BLOCK = {"SQRT": 0x3F700000, "POW5": 0x3F700000, "UNI_M1_1": 0xFFF00000, "UNI_H": 0xFFF00000,
            "UNI_0_1": 0xFFF00000, "REFR_AG": 0x3F000000, "REFR_GA": 0x3F380000, "GAMMA": 0x43700000,
            "F2U8": 0x43780000}


def same_or_nan(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


# ---------------------------------------------------------------- generators

def test_set_sizes():
    assert ms.edge_mantissas().size == 16 and np.unique(ms.edge_mantissas()).size == 16
    for name, make in ms.DIV_SETS.items():
        a, b = make()
        assert a.size == b.size == ms.DIV_SIZES[name], name
        assert a.dtype == b.dtype == np.float32
    assert ms.DIV_SIZES == {"div_grid": 7398400, "div_hard": 655360, "div_full": 1049537, "div_primary": 1413810,
                            "div_recip_hard": 117030}
    x, y, z = ms.normalize_grid()
    assert x.size == y.size == z.size == ms.NORM_SIZE == 2005584
    x, j, want = ms.halve_grid()
    assert x.size == j.size == want.size == ms.HALVE_SIZE == 2003456
    assert int(j.max()) == 300 and np.unique(ms.u32(x) >> 23 & 0xFF).size == 256


def test_div_grid_holds_the_gate_from_both_sides():
    a, b = ms.div_grid()
    for v in (a, b):
        have = set(np.unique(ms.u32(v)).tolist())
        for mid in (0x2B800000, 0x53800000):  # 2^-40, 2^40
            for bits in (mid - 1, mid, mid + 1):
                assert bits in have and (bits | 0x80000000) in have
    assert bool(ms.operand_ok(np.float32(2.0 ** 40))) and not bool(ms.operand_ok(ms.f32(np.uint32(0x53800001))))
    assert bool(ms.operand_ok(np.float32(2.0 ** -40))) and not bool(ms.operand_ok(ms.f32(np.uint32(0x2B7FFFFF))))
    ok = ms.operand_ok(a) & ms.operand_ok(b)
    assert 2 * int(ok.sum()) > a.size and not ok.all()


def test_div_hard_quotients_sit_next_to_a_midpoint():
    """In exact rational arithmetic, on 2000 of the pairs: the quotient, scaled into
    [2^23, 2^24), lies within HARD_BOUND = 2^-12 ulp of a half-integer (the bound is the
    generator's acceptance rule, math_sweep.div_hard_mantissas), never on one, and every
    operand is inside the division core's gate."""
    a, b = ms.div_hard()
    assert ms.operand_ok(a).all() and ms.operand_ok(b).all()
    assert (b < 0).any() and (b > 0).any()
    pick = np.random.default_rng(5).choice(a.size, 2000, replace=False)
    worst = Fraction(0)
    for i in pick:
        q = abs(Fraction(float(a[i])) / Fraction(float(b[i])))
        while q >= 1 << 24:
            q /= 2
        while q < 1 << 23:
            q *= 2
        off = abs(q - (q.numerator // q.denominator) - Fraction(1, 2))
        assert 0 < off <= ms.HARD_BOUND, (a[i], b[i], off)
        worst = max(worst, off)
    # the generator's own distances say the same, over all of them
    A, B, D = ms.div_hard_mantissas()
    assert (D > 0).all() and (D * ms.HARD_BOUND.denominator <= 2 * B * ms.HARD_BOUND.numerator).all()
    assert worst <= Fraction(int((D * (1 << 40) // (2 * B)).max()) + 1, 1 << 40)


def test_div_recip_hard_is_what_it_says():
    """Exactly, with Python integers: each divisor's reciprocal lies within 2^-11 ulp of a
    midpoint (the hardest one within 2^-24), and each quotient at |2 rem - B| <= 7, which
    is within 7 / 2^24 ulp of one."""
    A, B = (v.tolist() for v in ms.div_recip_hard_mantissas())
    closest = Fraction(1)
    for a, b in zip(A, B):
        assert b % 2 == 1 and (1 << 23) < b < (1 << 24) and (1 << 23) <= a < (1 << 24)
        r = abs(2 * ((1 << 47) % b) - b)
        assert r * (1 << 11) <= 2 * b
        closest = min(closest, Fraction(r, 2 * b))
        n = a << (23 if a >= b else 24)
        assert (1 << 23) <= n // b < (1 << 24) and abs(2 * (n % b) - b) in ms.RECIP_OFFSETS
    assert closest < Fraction(1, 1 << 24)
    a, b = ms.div_recip_hard()
    assert ms.operand_ok(a).all() and ms.operand_ok(b).all() and (b < 0).any()
    # the scan kept the hardest: no odd divisor outside the set has a closer reciprocal
    kept = np.unique(np.array(B, np.int64))
    every = np.arange((1 << 23) + 1, 1 << 24, 2, dtype=np.int64)
    d = np.abs(2 * ((1 << 47) % every) - every)
    assert kept.size == ms.RECIP_DIVISORS and np.sort(d)[ms.RECIP_DIVISORS - 1] == d[np.isin(every, kept)].max()


def test_div_primary_has_what_start_path_forms():
    a, b = ms.div_primary()
    assert (a < 0).any() and (a == 0).any() and (np.abs(a[a != 0]) < 1e-6).any()
    assert {1.0, 1200.0, 1440.0, 3840.0, 4096.0, 65535.0, 65536.0} <= set(np.unique(b).tolist())
    assert ms.operand_ok(b).all() and not ms.operand_ok(a).all()


@pytest.mark.parametrize("name", list(ms.DIV_SETS))
def test_division_reference_is_the_rounded_exact_quotient(name):
    """np.float32 division equals float64 division rounded to float32: the double's 53
    bits are at least 2 * 24 + 2, so the second rounding is innocuous."""
    a, b = ms.DIV_SETS[name]()
    with np.errstate(all="ignore"):
        wide = (a.astype(np.float64) / b.astype(np.float64)).astype(np.float32)
    assert same_or_nan(ms.expected_div(a, b), wide).all()


def test_normalize_and_halve_references():
    x, y, z = ms.normalize_grid()
    want = ms.expected_normalize(x, y, z)
    assert want.shape == (x.size, 3) and want.dtype == np.float32
    i = int(np.nonzero((x == 3) | (x == 2.0 ** 40))[0][0])
    l = np.sqrt(np.float32(np.float32(x[i] * x[i] + y[i] * y[i]) + z[i] * z[i]))
    assert want[i, 0] == x[i] / l
    top = (np.abs(x) == 2.0 ** 40) & (np.abs(y) == 2.0 ** 40) & (np.abs(z) == 2.0 ** 40)
    assert top.sum() >= 8  # |v|^2 = 3 * 2^80
    hx, hj, hw = ms.halve_grid()
    for k in (0, 7, 6656 * 3 + 11, 6656 * 150 + 200 * 13 + 5, hx.size - 1):
        v = np.float32(hx[k])
        with np.errstate(all="ignore"):
            for _ in range(int(hj[k])):
                v = np.float32(v * np.float32(0.5))
        assert same_or_nan(hw[k], v)


# ---------------------------------------------------------------- host ops

@pytest.mark.parametrize("op", ms.HOST_OPS)
def test_host_digest_is_the_sum_over_its_block(oracle, op):
    """spo_math_digest against the numpy restatement of the digest over spo_math_block, on
    one whole block and on a range that ends inside its second block."""
    first = OP_BLOCK[op]
    for count in (ms.BLOCK, ms.BLOCK + 77):
        r = oracle.math_block(ms.OPS[op], first, count)
        assert np.array_equal(oracle.math_digest(ms.OPS[op], first, count), ms.digest_of(first, r)), (op, count)


def test_host_ranges_wrap_with_the_pattern(oracle):
    r = oracle.math_block(ms.OPS["F2U8"], 0xFFFFFFF0, 32)
    assert np.array_equal(r[16:], oracle.math_block(ms.OPS["F2U8"], 0, 16))
    assert np.array_equal(oracle.math_digest(ms.OPS["SQRT"], 0xFFFFFFF0, 32),
                          ms.digest_of(0xFFFFFFF0, oracle.math_block(ms.OPS["SQRT"], 0xFFFFFFF0, 32)))


def test_host_rejects_device_only_ops(oracle):
    out = np.zeros(4, np.uint64)
    for op in ("SQRT_POS", "SQRT_RAW"):
        assert oracle.lib().spo_math_digest(ms.OPS[op], 0, 4, out.ctypes.data_as(ctypes.c_void_p)) == 1
    assert oracle.lib().spo_math_digest(11, 0, 4, out.ctypes.data_as(ctypes.c_void_p)) == 1


@pytest.mark.parametrize("op", ms.HOST_OPS)
def test_digest_moves_with_one_ulp(oracle, op):
    first = OP_BLOCK[op]
    r = oracle.math_block(ms.OPS[op], first, ms.BLOCK)
    base = ms.digest_of(first, r)
    for at in (0, 12345, ms.BLOCK - 1):
        for step in (1, -1):
            s = r.copy()
            s[at] = np.uint32((int(s[at]) + step) & 0xFFFFFFFF)
            assert ms.digest_of(first, s)[0] != base[0], (op, at, step)
    # and with where a result sits: two unequal neighbours exchanged
    at = int(np.nonzero(r[1:] != r[:-1])[0][0])
    s = r.copy()
    s[at], s[at + 1] = r[at + 1], r[at]
    assert ms.digest_of(first, s)[0] != base[0]


def test_uniform_ops_are_the_oracles_uniform(oracle):
    for op, (lo, hi) in ms.UNI_RANGES.items():
        for u in SPECIAL_DRAWS:
            want = np.float32(oracle.lib().spo_uniform_u32(u, lo, hi))
            assert int(oracle.math_block(ms.OPS[op], u, 1)[0]) == int(want.view(np.uint32)), (op, hex(u))
    # the literal definition in numpy (math_sweep.uniform_m1_1, which forms div_primary's
    # numerators) is the same function
    first = OP_BLOCK["UNI_M1_1"]
    u = (first + np.arange(ms.BLOCK, dtype=np.uint64)).astype(np.uint32)
    assert np.array_equal(oracle.math_block(ms.OPS["UNI_M1_1"], first, ms.BLOCK), ms.u32(ms.uniform_m1_1(u)))


def test_host_ops_are_the_literal_definitions(oracle):
    """Each host op on its block against an independent statement of the same definition:
    numpy's correctly rounded float32 sqrt, libm's powf, spo_write_pixel."""
    def inputs(op):
        return ms.f32((OP_BLOCK[op] + np.arange(ms.BLOCK, dtype=np.uint64)).astype(np.uint32))

    def block(op):
        return oracle.math_block(ms.OPS[op], OP_BLOCK[op], ms.BLOCK)

    one = np.float32(1)
    with np.errstate(all="ignore"):
        assert np.array_equal(block("SQRT"), ms.u32(np.sqrt(inputs("SQRT"))))
        for op, r in (("REFR_AG", one / np.float32(1.5)), ("REFR_GA", np.float32(1.5) / one)):
            c = inputs(op)
            ok = r * np.sqrt(one - c * c) < one
            k = r * c - np.sqrt(one - r * r * (one - c * c))
            assert np.array_equal(block(op), ms.u32(np.where(ok, k, np.float32(-1e30)))), op
            if op == "REFR_GA":  # the block spans the critical angle: both outcomes
                assert ok.any() and not ok.all()
        x = inputs("F2U8")
        assert np.array_equal(block("F2U8"), x.astype(np.int64).astype(np.uint8).astype(np.uint32))
    # negative, huge and NaN inputs of the conversion: cvttss2si's INT_MIN, low byte 0
    for bits, want in ((0xBF800000, 0xFF), (0xC3800000, 0), (0x4F000000, 0), (0x7FC00000, 0), (0xFF800000, 0),
                       (0x4EFFFFFF, 0x80)):
        assert int(oracle.math_block(ms.OPS["F2U8"], bits, 1)[0]) == want, hex(bits)
    libm = ctypes.CDLL("libm.so.6")
    libm.powf.restype = ctypes.c_float
    libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
    x, got = inputs("POW5"), block("POW5")
    for i in range(0, ms.BLOCK, 4099):
        assert int(got[i]) == int(np.float32(libm.powf(float(x[i]), 5.0)).view(np.uint32))
    x, got = inputs("GAMMA"), block("GAMMA")
    px = np.zeros(3, np.uint8)
    for i in range(0, ms.BLOCK, 4099):
        c = np.array([x[i], 0, 0, 0], np.float32)
        oracle.lib().spo_write_pixel(c.ctypes.data_as(ctypes.c_void_p), px.ctypes.data_as(ctypes.c_void_p))
        assert int(got[i]) == int(px[0])
    assert int(oracle.math_block(ms.OPS["SQRT"], 0xBF800000, 1)[0]) == 0x7FC00000  # NaN canonical
