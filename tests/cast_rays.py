"""The adversarial ray mix and the float32 restatement of a hit record, shared by the ray
query tests on the GPU (tests/test_gpu_cast.py) and the comparison with the reference's own
code on the CPU (tests/test_reference_parity.py).  A plain helper module: numpy only.

make_rays builds, for a scene, rays whose kinds are shuffled together:

    A 25%  origin on a random sphere's surface, direction in its outward or inward hemisphere
    B 20%  from the default eye toward a point within 1.2 r of a random centre
    C 20%  grazing: aimed past a sphere (r^2 > 4e-3) from 3..30 units away so that
           hh = r^2 - d2 is uniform in [0, 2e-3] -- either side of RaySphereIntersection's
           hh > 1e-3
    D 10%  origin inside such a sphere with tc uniform in [0, 2e-3] -- either side of tc > 1e-3
    E 15%  kinds A / B with the direction scaled by 0.5, 2 or 1 +- 3e-6 (the never-cull lanes)
    F  2%  a NaN, +inf, -inf or zero component in o or d
    G  8%  from high above the scene, pointing away (misses)
"""
import numpy as np

EYE = [0, 1, -3, 0]  # the default eye of every test file
N_RAYS = 4099
RAY_SEED = 20240
KINDS = "ABCDEFG"
SHARES = (0.25, 0.20, 0.20, 0.10, 0.15, 0.02, 0.08)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(rng, d):
    """A unit vector perpendicular to each row of d."""
    e = np.cross(d, _unit(rng, len(d)))
    return e / np.linalg.norm(e, axis=1, keepdims=True)


def make_rays(centers, radii, n=N_RAYS, seed=RAY_SEED):
    """(o, d, kind, aim): float32 (n, 4) origins and directions (w = 0), the kind's letter
    per ray, and for kinds C and D the sphere aimed at (else -1).  Built in float64 and
    rounded: the thresholds of C and D are then straddled to within float32 rounding."""
    rng = np.random.default_rng(seed)
    C = np.asarray(centers, np.float64)[:, :3]
    R = np.asarray(radii, np.float64)
    counts = [int(round(s * n)) for s in SHARES]
    counts[0] += n - sum(counts)
    kind = np.array([k for k, c in zip(KINDS, counts) for _ in range(c)])
    rng.shuffle(kind)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    aim = np.full(n, -1, np.int64)
    big = np.nonzero(R * R > 4e-3)[0]
    eye = np.asarray(EYE, np.float64)[:3]

    def kind_a(m):
        j = rng.integers(0, len(R), m)
        nrm = _unit(rng, m)
        dd = _unit(rng, m)
        out = np.sum(dd * nrm, axis=1) > 0
        dd = np.where(out[:, None], dd, -dd)             # outward hemisphere ...
        dd = np.where((rng.random(m) < 0.5)[:, None], dd, -dd)  # ... or the inward one
        return C[j] + R[j, None] * nrm, dd

    def kind_b(m):
        j = rng.integers(0, len(R), m)
        u = _unit(rng, m) * np.cbrt(rng.random(m))[:, None]
        t = C[j] + 1.2 * R[j, None] * u - eye
        return np.broadcast_to(eye, (m, 3)).copy(), t / np.linalg.norm(t, axis=1, keepdims=True)

    def kind_ab(m):
        oa, da = kind_a(m)
        ob, db = kind_b(m)
        pick = (rng.random(m) < 0.5)[:, None]
        return np.where(pick, oa, ob), np.where(pick, da, db)

    for k in KINDS:
        sel = np.nonzero(kind == k)[0]
        m = len(sel)
        if k == "A":
            o[sel], d[sel] = kind_a(m)
        elif k == "B":
            o[sel], d[sel] = kind_b(m)
        elif k == "C":
            j = big[rng.integers(0, len(big), m)]
            dd = _unit(rng, m)
            hh = rng.uniform(0.0, 2e-3, m)
            b = np.sqrt(R[j] * R[j] - hh)
            o[sel] = C[j] + b[:, None] * _perp(rng, dd) - rng.uniform(3.0, 30.0, m)[:, None] * dd
            d[sel], aim[sel] = dd, j
        elif k == "D":
            j = big[rng.integers(0, len(big), m)]
            dd = _unit(rng, m)
            tc = rng.uniform(0.0, 2e-3, m)
            b = rng.uniform(0.0, 0.5, m) * R[j]  # hh = r^2 - b^2 >= 3e-3: tc alone decides
            o[sel] = C[j] + b[:, None] * _perp(rng, dd) - tc[:, None] * dd
            d[sel], aim[sel] = dd, j
        elif k == "E":
            oe, de = kind_ab(m)
            scale = rng.choice([0.5, 2.0, 1.0 + 3e-6, 1.0 - 3e-6], m)
            o[sel], d[sel] = oe, de * scale[:, None]
        elif k == "F":
            of, df = kind_ab(m)
            both = np.concatenate([of, df], axis=1)
            both[np.arange(m), rng.integers(0, 6, m)] = rng.choice([np.nan, np.inf, -np.inf, 0.0], m)
            o[sel], d[sel] = both[:, :3], both[:, 3:]
        else:
            og = np.stack([rng.uniform(-20, 20, m), rng.uniform(40, 80, m), rng.uniform(-20, 20, m)], axis=1)
            dg = _unit(rng, m)
            dg[:, 1] = np.abs(dg[:, 1])
            o[sel], d[sel] = og, dg
    o4, d4 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    with np.errstate(all="ignore"):
        o4[:, :3], d4[:, :3] = o, d
    return o4, d4, kind, aim


def restate_hits(centers, radii, idx, o, d):
    """t, P, n of ClosestContactPoint / ContactNormal for rays (o, d) that hit sphere idx
    (Collision.hpp:19-27, 49-56, 67-71): float32 throughout, one numpy
    operation per reference operation (no operation here can contract), sums in Dot's
    order (x x' + y y') + z z', sqrt and division correctly rounded."""
    f = np.float32
    C, r = np.asarray(centers, f)[idx, :3], np.asarray(radii, f)[idx]
    o, d = np.asarray(o, f)[:, :3], np.asarray(d, f)[:, :3]

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    with np.errstate(all="ignore"):
        rs = C - o
        tc = dot(rs, d)
        d2 = dot(rs, rs) - tc * tc
        t = tc - np.sqrt(r * r - d2)
        P = o + d * t[:, None]
        v = P - C
        n = v / np.sqrt(dot(v, v))[:, None]
    assert t.dtype == P.dtype == n.dtype == f
    return t, P, n
