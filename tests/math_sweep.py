"""Inputs and expected values of the exact-primitive sweeps (tests/test_gpu_math_sweep.py,
tests/test_math_sweep_helper.py).  numpy only: nothing here calls the device or the
oracle.  Every generator is seeded and deterministic, and cached: callers must not write
into what they get.

Operand sets of the division (`a / b`, spt_device.h div_rn / div_core / recip), of
Normalize and of the fold's halvings (spt_decode.h halve_n), with their references as one
numpy float32 operation per reference operation; the op codes and the digest of the
unary sweeps (tests/cpp/spt_mathsweep.hip, oracle/spt_oracle.c spo_math_*).
"""
import functools
from fractions import Fraction

import numpy as np

SEED = 20260117
BLOCK = 1 << 20  # input patterns per digest

# op codes of spt_sweep_digest / spt_sweep_dump and spo_math_digest / spo_math_block
OPS = {"SQRT": 0, "SQRT_POS": 1, "SQRT_RAW": 2, "POW5": 3, "UNI_M1_1": 4, "UNI_H": 5, "UNI_0_1": 6,
       "REFR_AG": 7, "REFR_GA": 8, "GAMMA": 9, "F2U8": 10}
# the ops that have a literal host definition (the other two are device forms of SQRT)
HOST_OPS = ("SQRT", "POW5", "UNI_M1_1", "UNI_H", "UNI_0_1", "REFR_AG", "REFR_GA", "GAMMA", "F2U8")
UNI_RANGES = {"UNI_M1_1": (-1.0, 1.0), "UNI_H": (-0.5, 0.5), "UNI_0_1": (0.0, 1.0)}

GATE_LO, GATE_HI = np.float32(2.0 ** -40), np.float32(2.0 ** 40)  # div_operand_ok
SIGN = np.uint32(0x80000000)


def f32(bits):
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def pack(exp, mant, sign=0):
    """Bits of (-1)^sign * 2^exp * (1 + mant / 2^23), exp unbiased in -126 ... 127."""
    return ((np.asarray(sign, np.uint32) << np.uint32(31)) | ((np.asarray(exp, np.int64) + 127).astype(np.uint32)
                                                                << np.uint32(23)) | np.asarray(mant, np.uint32))


def operand_ok(x):
    """div_operand_ok (spt_device.h): |x| in [2^-40, 2^40]; false for 0, inf, NaN."""
    ax = np.abs(np.asarray(x, np.float32))
    return (ax >= GATE_LO) & (ax <= GATE_HI)


# ---------------------------------------------------------------- digests

def fmix64(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def digest_of(first, results):
    """The digests of consecutive input patterns first, first + 1, ... with these result
    bits: per block of 2^20, the wrapping sum of fmix64(u << 32 | r)."""
    r = np.asarray(results, np.uint32).astype(np.uint64)
    u = (np.uint64(first) + np.arange(r.size, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        h = fmix64((u << np.uint64(32)) | r)
        return np.array([h[k:k + BLOCK].sum(dtype=np.uint64) for k in range(0, r.size, BLOCK)], np.uint64)


# ---------------------------------------------------------------- mantissas

@functools.lru_cache(None)
def edge_mantissas():
    """16 mantissas: the ends, the middle and its neighbours, 1/3 and 2/3, five random."""
    fixed = [0, 1, 2, 3, 0x3FFFFF, 0x400000, 0x400001, 0x555555, 0x2AAAAA, 0x7FFFFE, 0x7FFFFF]
    rng = np.random.default_rng(SEED)
    extra = []
    while len(extra) < 5:
        m = int(rng.integers(0, 1 << 23))
        if m not in fixed and m not in extra:
            extra.append(m)
    return np.array(fixed + extra, np.uint32)


# ---------------------------------------------------------------- division

@functools.lru_cache(None)
def div_grid():
    """Exponents -42 ... 42 x 16 mantissas for each operand, x the four sign pairs:
    7 398 400 pairs.  Holds +-2^-40 and +-2^40 (mantissa 0), their upper neighbours
    (mantissa 1) and their lower ones (exponent - 1, mantissa 0x7FFFFF) in both operands:
    div_operand_ok's two edges from both sides."""
    e = np.repeat(np.arange(-42, 43), 16)
    v = pack(e, np.tile(edge_mantissas(), 85))  # 1360 magnitudes
    a, b = np.repeat(v, v.size), np.tile(v, v.size)
    a = np.concatenate([a, a | SIGN, a, a | SIGN])
    b = np.concatenate([b, b, b | SIGN, b | SIGN])
    return f32(a), f32(b)


HARD_DIVISORS, HARD_SCAN, HARD_KEEP = 4096, 1 << 16, 16
HARD_EXPONENTS = (0, 20, -20, 39, -39)
HARD_ROWS = 8  # divisors per numpy pass: temporaries that stay in the cache
HARD_BOUND = Fraction(1, 1 << 12)  # ulp, from a rounding midpoint


@functools.lru_cache(None)
def div_hard_mantissas():
    """Hard-to-round quotients, in exact integer arithmetic.  For each of 4096 random
    24-bit divisor significands B, 2^16 consecutive numerator significands A are scanned.
    With A / B scaled into [2^23, 2^24) as N / B (N = A << 23 if A >= B, else A << 24),
    the quotient's distance from the midpoint of two neighbouring floats is
    |rem / B - 1/2| = |2 rem - B| / (2 B) ulp, rem = N mod B.  The 16 numerators with the
    smallest |2 rem - B| are kept.

    The bound.  Over 2^16 numerators the residues of an ordinary divisor are spread
    evenly, so the k-th smallest |rem / B - 1/2| is about k / 2^17: 2^-13 ulp for the
    16th.  A divisor whose 2^24 / B lies next to a fraction of small denominator clusters
    its residues instead (7 in 1000 do, by more than a factor of two); such a draw is
    passed over and the next one taken, so that every kept pair lies within
    HARD_BOUND = 2^-12 ulp of a midpoint.  Returns (A, B, |2 rem - B|), 65 536 each, int64."""
    rng = np.random.default_rng(SEED + 1)
    cand = HARD_DIVISORS + 256
    B = (1 << 23) | rng.integers(0, 1 << 23, cand, dtype=np.int64)
    A0 = (1 << 23) + rng.integers(0, (1 << 23) - HARD_SCAN, cand, dtype=np.int64)
    span = np.arange(HARD_SCAN, dtype=np.int64)
    As, Bs, Ds = [], [], []
    for lo in range(0, cand, HARD_ROWS):
        b = B[lo:lo + HARD_ROWS, None]
        A = A0[lo:lo + HARD_ROWS, None] + span[None, :]
        N = A << np.where(A >= b, 23, 24)  # < 2^48
        d = np.abs(2 * (N % b) - b)
        # the 16 smallest by (distance, numerator): a total order, so no tie is left to
        # the partition's whim
        key = d * HARD_SCAN + span[None, :]
        order = np.argpartition(key, HARD_KEEP, axis=1)[:, :HARD_KEEP]
        order = np.take_along_axis(order, np.argsort(np.take_along_axis(key, order, 1), axis=1), 1)
        dk = np.take_along_axis(d, order, 1)
        keep = dk[:, -1] * HARD_BOUND.denominator <= 2 * b[:, 0] * HARD_BOUND.numerator
        As.append(np.take_along_axis(A, order, 1)[keep])
        Bs.append(b[keep, 0])
        Ds.append(dk[keep])
    A, B, D = np.concatenate(As)[:HARD_DIVISORS], np.concatenate(Bs)[:HARD_DIVISORS], np.concatenate(Ds)[:HARD_DIVISORS]
    assert B.size == HARD_DIVISORS
    return A.ravel(), np.repeat(B, HARD_KEEP), D.ravel()


@functools.lru_cache(None)
def div_hard():
    """div_hard_mantissas() placed at 2^e * A / (+-2^-e * B) for e in 0, +-20, +-39: all
    operands inside div_operand_ok, quotients from 2^-79 to 2^79.  655 360 pairs."""
    A, B, _ = div_hard_mantissas()
    ma, mb = (A & 0x7FFFFF).astype(np.uint32), (B & 0x7FFFFF).astype(np.uint32)
    a, b = [], []
    for e in HARD_EXPONENTS:
        for sb in (0, 1):
            a.append(pack(e, ma))
            b.append(pack(-e, mb, sb))
    return f32(np.concatenate(a)), f32(np.concatenate(b))


RECIP_DIVISORS = 2048
RECIP_OFFSETS = (1, 3, 5, 7)  # |2 rem - B| of the numerators made for each divisor


@functools.lru_cache(None)
def div_recip_hard_mantissas():
    """The pairs on which the second residual step of div_core can matter.  Its first step
    q = fma(a - b q0, rc, q0) already rounds correctly when rc is the correctly rounded
    1 / b; rc = recip(b) can only miss that where 1 / b itself lies next to a rounding
    midpoint, and then only a quotient next to a midpoint of its own can show it.  So:
    all 2^22 odd 24-bit significands B are scanned for |2 rem - B|, rem = 2^47 mod B (the
    reciprocal's distance from a midpoint, as in div_hard_mantissas), and the 2048 with
    the smallest are kept; for each, the numerators A whose quotient lies as close to a
    midpoint as an integer remainder allows, 2 rem - B = +-1, +-3, +-5, +-7, are solved for
    exactly: A = rem * (2^s)^-1 mod B for both scalings s.  Returns (A, B), int64."""
    B = np.arange((1 << 23) + 1, 1 << 24, 2, dtype=np.int64)
    d = np.abs(2 * ((1 << 47) % B) - B)
    key = d * (1 << 24) + B  # a total order
    B = np.sort(B[np.argpartition(key, RECIP_DIVISORS)[:RECIP_DIVISORS]])
    As, Bs = [], []
    for b in B.tolist():
        for s in (23, 24):
            inv = pow(1 << s, -1, b)
            for k in RECIP_OFFSETS:
                for rem in ((b + k) // 2, (b - k) // 2):
                    a = rem * inv % b  # the one numerator below b with this remainder
                    if s == 23:
                        a += b  # scaling 23 is the one of a >= b
                    if (1 << 23) <= a < (1 << 24) and (a >= b) == (s == 23):
                        As.append(a)
                        Bs.append(b)
    return np.array(As, np.int64), np.array(Bs, np.int64)


@functools.lru_cache(None)
def div_recip_hard():
    """div_recip_hard_mantissas() at the placements of div_hard()."""
    A, B = div_recip_hard_mantissas()
    ma, mb = (A & 0x7FFFFF).astype(np.uint32), (B & 0x7FFFFF).astype(np.uint32)
    a, b = [], []
    for e in HARD_EXPONENTS:
        for sb in (0, 1):
            a.append(pack(e, ma))
            b.append(pack(-e, mb, sb))
    return f32(np.concatenate(a)), f32(np.concatenate(b))


def special_values():
    """+-0, +-min and max denormal, +-FLT_MIN, +-1, +-2^+-40 and their neighbours,
    +-2^+-42, +-FLT_MAX, +-inf, NaN: 31 bit patterns."""
    pos = [0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000,
           0x2B7FFFFF, 0x2B800000, 0x2B800001, 0x537FFFFF, 0x53800000, 0x53800001,
           0x2A800000, 0x54800000, 0x7F7FFFFF, 0x7F800000]
    return np.array(pos + [p | 0x80000000 for p in pos] + [0x7FC00000], np.uint32)


FULL_RANDOM = 1 << 20


@functools.lru_cache(None)
def div_full():
    """2^20 pairs of uniformly random bit patterns, then every pair of special_values():
    1 048 576 + 961 pairs."""
    rng = np.random.default_rng(SEED + 2)
    r = rng.integers(0, 1 << 32, (2, FULL_RANDOM), dtype=np.uint64).astype(np.uint32)
    s = special_values()
    return (f32(np.concatenate([r[0], np.repeat(s, s.size)])), f32(np.concatenate([r[1], np.tile(s, s.size)])))


def uniform_m1_1(bits):
    """uniform(-1, 1) of a raw draw, the literal definition (oracle spo_uniform_u32)."""
    u = np.asarray(bits, np.uint32).astype(np.float32) / np.float32(4294967296.0)
    u = np.where(u >= np.float32(1), np.nextafter(np.float32(1), np.float32(0)), u).astype(np.float32)
    return (u * np.float32(2) + np.float32(-1)).astype(np.float32)


PRIMARY_WIDTHS = tuple(range(1, 4097)) + (65535, 65536)  # 1200, 1440 and 3840 are inside
PRIMARY_SPECIAL_DRAWS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
PRIMARY_DRAWS = 64


@functools.lru_cache(None)
def div_primary():
    """What start_path divides (spt_path.h: `un / g_width`): divisors float(W) for W in
    1 ... 4096, 65535 and 65536; numerators float(y) + uniform(-1, 1) for y in 0, 1, 2,
    W - 1, W, with 64 random draws each and the draws 0, 1, 0x7FFFFFFF, 0x80000000 and
    0xFFFFFFFF: negative, zero and tiny numerators against one divisor.
    4098 x 5 x 69 = 1 413 810 pairs."""
    rng = np.random.default_rng(SEED + 3)
    W = np.array(PRIMARY_WIDTHS, np.int64)
    y = np.stack([np.zeros_like(W), np.ones_like(W), np.full_like(W, 2), W - 1, W], 1)  # (W, 5)
    nd = PRIMARY_DRAWS + len(PRIMARY_SPECIAL_DRAWS)
    draws = rng.integers(0, 1 << 32, (W.size, 5, nd), dtype=np.uint64).astype(np.uint32)
    draws[:, :, PRIMARY_DRAWS:] = np.array(PRIMARY_SPECIAL_DRAWS, np.uint32)
    a = (y.astype(np.float32)[:, :, None] + uniform_m1_1(draws)).astype(np.float32)
    b = np.broadcast_to(W.astype(np.float32)[:, None, None], a.shape)
    return np.ascontiguousarray(a.ravel()), np.ascontiguousarray(b.ravel())


DIV_SETS = {"div_grid": div_grid, "div_hard": div_hard, "div_full": div_full, "div_primary": div_primary,
            "div_recip_hard": div_recip_hard}
DIV_SIZES = {"div_grid": 4 * 1360 * 1360, "div_hard": HARD_DIVISORS * HARD_KEEP * len(HARD_EXPONENTS) * 2,
             "div_full": FULL_RANDOM + 31 * 31, "div_primary": len(PRIMARY_WIDTHS) * 5 * 69,
             "div_recip_hard": 11703 * len(HARD_EXPONENTS) * 2}


def expected_div(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float32) / np.asarray(b, np.float32)).astype(np.float32)


# ---------------------------------------------------------------- Normalize

NORM_EXPONENTS = tuple(range(-41, 42, 3))  # 28: -41 below the gate, 40 at its top
NORM_MANTISSAS = (0, 1, 0x555555, 0x7FFFFF)
NORM_ANY = 1 << 19
NORM_SIZE = 112 ** 3 + 3 * 2 * 112 ** 2 + 3 * 2 * 112 + NORM_ANY + 2 * 216


@functools.lru_cache(None)
def normalize_grid():
    """Triples (x, y, z) for Normalize, 2 005 584 of them:
    - 28 exponents (-41 ... 40 in steps of 3) x 4 mantissas per component, all 112^3
      combinations, the sign octant cycling with the index (every exponent triple meets
      all eight): components below, inside, at the top of and above the gate;
    - one zero component (+0 and -0, each position) with all 112^2 of the other two, and
      two zero components with each of the 112 values and its negative;
    - 2^19 triples with one component of any bit pattern (inf, NaN, denormals), the other
      two drawn from the 112 values with random signs;
    - all three components among 2^40 and its two neighbours (|v|^2 = 3 * 2^80), and
      among 2^-40 and its two neighbours, in every sign octant."""
    rng = np.random.default_rng(SEED + 4)
    v = pack(np.repeat(np.array(NORM_EXPONENTS), 4), np.tile(np.array(NORM_MANTISSAS, np.uint32), 28))  # 112
    n = v.size
    parts = []
    # all combinations, octant by index
    i = np.arange(n ** 3)
    oct_ = (i % 8).astype(np.uint32)
    parts.append([v[i // (n * n)] | ((oct_ & 1) << 31), v[(i // n) % n] | (((oct_ >> 1) & 1) << 31),
                  v[i % n] | (((oct_ >> 2) & 1) << 31)])
    # one zero component
    p, q = np.repeat(v, n), np.tile(v, n)
    for zero in (np.uint32(0), SIGN):
        z = np.full(n * n, zero, np.uint32)
        parts += [[z, p, q | SIGN], [p | SIGN, z, q], [p, q, z]]
    # two zero components
    for s in (np.uint32(0), SIGN):
        z, zn = np.zeros(n, np.uint32), np.full(n, SIGN, np.uint32)
        parts += [[v | s, z, zn], [zn, v | s, z], [z, zn, v | s]]
    # one component of any bit pattern
    anyb = rng.integers(0, 1 << 32, NORM_ANY, dtype=np.uint64).astype(np.uint32)
    o1 = v[rng.integers(0, n, NORM_ANY)] | (rng.integers(0, 2, NORM_ANY).astype(np.uint32) << 31)
    o2 = v[rng.integers(0, n, NORM_ANY)] | (rng.integers(0, 2, NORM_ANY).astype(np.uint32) << 31)
    pos = rng.integers(0, 3, NORM_ANY)
    parts.append([np.where(pos == 0, anyb, o1), np.where(pos == 1, anyb, np.where(pos == 0, o1, o2)),
                  np.where(pos == 2, anyb, o2)])
    # the gate's two edges in all three components
    for mid in (0x53800000, 0x2B800000):
        g = np.array([mid - 1, mid, mid + 1], np.uint32)
        i = np.arange(27)
        for o in range(8):
            parts.append([g[i // 9] | np.uint32((o & 1) << 31), g[(i // 3) % 3] | np.uint32(((o >> 1) & 1) << 31),
                          g[i % 3] | np.uint32(((o >> 2) & 1) << 31)])
    x, y, z = (f32(np.concatenate([np.asarray(p[k], np.uint32) for p in parts])) for k in range(3))
    return x, y, z


def expected_normalize(x, y, z):
    """Math.hpp Normalize: L = (x*x + y*y) + z*z, l = sqrt(L), each component / l."""
    x, y, z = (np.asarray(c, np.float32) for c in (x, y, z))
    with np.errstate(all="ignore"):
        L = ((x * x).astype(np.float32) + (y * y).astype(np.float32)).astype(np.float32)
        L = (L + (z * z).astype(np.float32)).astype(np.float32)
        l = np.sqrt(L).astype(np.float32)
        return np.stack([(x / l).astype(np.float32), (y / l).astype(np.float32), (z / l).astype(np.float32)], 1)


# ---------------------------------------------------------------- halvings

HALVE_JS = 301
HALVE_SIZE = 256 * 13 * 2 * HALVE_JS


@functools.lru_cache(None)
def halve_grid():
    """All 256 exponent fields (zero and denormals, inf and NaN among them) x 13 mantissas
    x 2 signs x j in 0 ... 300: 2 003 456 (value, j) pairs, and the expected result of j
    single float32 halvings.  Returns (x, j, want)."""
    m = edge_mantissas()[:13]
    bits = (np.repeat(np.arange(256, dtype=np.uint32), 13) << np.uint32(23)) | np.tile(m, 256)
    v = f32(np.concatenate([bits, bits | SIGN]))  # 6656 values
    want = np.empty((HALVE_JS, v.size), np.float32)
    want[0] = v
    with np.errstate(all="ignore"):
        for j in range(1, HALVE_JS):
            want[j] = want[j - 1] * np.float32(0.5)
    x = np.ascontiguousarray(np.broadcast_to(v, want.shape)).ravel()
    j = np.repeat(np.arange(HALVE_JS, dtype=np.uint32), v.size)
    return x, j, want.ravel()


def mismatches(got_bits, want):
    """Indices where result bits differ from the expected floats; NaN matches NaN."""
    got_bits = np.asarray(got_bits, np.uint32)
    want = np.asarray(want, np.float32)
    bad = (got_bits != want.view(np.uint32)) & ~(np.isnan(got_bits.view(np.float32)) & np.isnan(want))
    return np.nonzero(bad.ravel())[0]
