"""The occlusion query's contract in numpy (include/spt_hip.h "occlusion queries", DESIGN.md
§4.17), its segment form, and the limits the tests deal.  A plain helper module: numpy only.

    occ[i] = idx_i < sphere count  and  ds_i < L_i        (fp32 compare)

with (idx_i, ds_i) what FindClosestIntersectionSphere and the cast report for ray i.
"""
import numpy as np

from cast_rays import EYE  # noqa: F401  (the tests' default eye)

F = np.float32
FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.nextafter(np.float32(0), np.float32(1))  # 2^-149
N_CLASSES = 8
LIMIT_SEED = 77


def contract(idx, ds, L, n_spheres):
    """The answer bytes (bool): a hit whose squared distance is strictly below the limit.
    A NaN limit compares false; so does any limit <= 0, as ds >= 0."""
    idx = np.asarray(idx)
    with np.errstate(invalid="ignore"):
        return (idx < n_spheres) & (np.asarray(ds, F) < np.asarray(L, F))


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def restate_segments(a, b, scale=1.0):
    """(o, d, L) of the segment form: v = b - a per component, o = a, d = Normalize(v) as
    tests/cast_rays.py: restate_hits restates it (v / sqrt(Dot(v, v)), float32, one numpy
    operation per device operation), L = Dot(v, v) * scale.  (n, 4) arrays, w = 0; a == b
    gives L = 0 and a NaN direction, which the contract never looks at."""
    a, b = np.asarray(a, F)[:, :3], np.asarray(b, F)[:, :3]
    with np.errstate(all="ignore"):
        v = b - a
        vv = _dot(v, v)
        d = v / np.sqrt(vv)[:, None]
        L = vv * F(scale)
    assert v.dtype == d.dtype == L.dtype == F
    o4, d4 = np.zeros((len(a), 4), F), np.zeros((len(a), 4), F)
    o4[:, :3], d4[:, :3] = a, d
    return o4, d4, L


def make_limits(ds, hit, seed=LIMIT_SEED):
    """(L, cls): one fp32 limit per ray and the class (1..8) it was dealt from, the classes
    shuffled so that single waves mix them:

        1  +inf                     5  nextafter(ds, 0)
        2  FLT_MAX                  6  ds * U[0, 2)
        3  ds exactly               7  one of 0, -1, -inf, NaN, the smallest denormal
        4  nextafter(ds, +inf)      8  4 ds

    For a miss "ds" is a random positive value."""
    rng = np.random.default_rng(seed)
    n = len(ds)
    hit = np.asarray(hit, bool)
    base = np.where(hit, np.asarray(ds, F), rng.uniform(0.01, 400.0, n).astype(F)).astype(F)
    cls = (np.arange(n) % N_CLASSES) + 1
    rng.shuffle(cls)
    L = np.zeros(n, F)
    with np.errstate(all="ignore"):
        L[cls == 1] = np.inf
        L[cls == 2] = FLT_MAX
        L[cls == 3] = base[cls == 3]
        L[cls == 4] = np.nextafter(base[cls == 4], F(np.inf))
        L[cls == 5] = np.nextafter(base[cls == 5], F(0))
        m = cls == 6
        L[m] = base[m] * rng.uniform(0.0, 2.0, m.sum()).astype(F)
        m = cls == 7
        L[m] = rng.choice(np.array([0.0, -1.0, -np.inf, np.nan, DENORM_MIN], F), m.sum())
        L[cls == 8] = F(4) * base[cls == 8]
    assert L.dtype == F
    return L, cls
