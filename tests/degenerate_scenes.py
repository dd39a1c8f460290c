"""Degenerate scene families for the oracle-parity tests (tests/test_degenerate_oracle.py on
the CPU, tests/test_gpu_degenerate.py on the GPU): inputs spt_set_scene accepts unchecked
and no well-formed scene contains -- signed, zero and denormal radii, nested and
intersecting balls, cameras inside balls, exact distance ties between materials,
magnitudes up to where squares overflow, non-finite geometry, fuzz and colours, unknown
material bytes, sky colours outside 0..255, and a mirror room whose paths reach the
specular-event cap.

Every value is a literal or drawn from np.random.default_rng; the 10-sphere `reference`
scene is read from tests/golden/scenes.npz.  A Variant names the spheres that make it
odd (`odd`, indices into its arrays): the CPU test asserts they are seen.
"""
import os
from dataclasses import dataclass, field

import numpy as np

EYE, LOOK, UP, SKY = [0, 1, -3, 0], [0, 1, 0, 0], [0, 1, 0, 0], [137, 207, 240, 0]
DIFFUSE, MIRROR, GLASS, SKYBOX = 3, 1, 2, 0
GROUND = ([0, -1000.5, 0], 1000.0, [30, 144, 255], DIFFUSE, 0.0)
NAN, INF = float("nan"), float("inf")

# the frame, samples, depth and seed of both test files
W, H, SPP, DEPTH, SEED = 64, 48, 4, 12, 1
FAMILIES = ("signed_radii", "nested", "ties_mixed", "sky_bytes", "magnitudes", "spec_cap", "nonfinite")


@dataclass
class Variant:
    family: str
    name: str
    arrays: tuple          # centers (n, 4), radii, colors (n, 4), materials, fuzz
    eye: list = field(default_factory=lambda: [float(v) for v in EYE])
    look: list = field(default_factory=lambda: [float(v) for v in LOOK])
    sky: list = field(default_factory=lambda: [float(v) for v in SKY])
    odd: tuple = ()        # indices of the spheres that make the scene odd
    frame: tuple = (W, H, SPP, DEPTH, SEED)

    @property
    def id(self):
        return f"{self.family}/{self.name}"


def _arrays(balls):
    """balls: (centre xyz, radius, colour rgb, material, fuzz) each."""
    n = len(balls)
    c, col = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    with np.errstate(all="ignore"):
        for i, b in enumerate(balls):
            c[i, :3] = np.float32(b[0])
            col[i, :3] = np.float32(b[2])
        r = np.array([b[1] for b in balls], np.float32)
        f = np.array([b[4] for b in balls], np.float32)
    m = np.array([b[3] for b in balls], np.uint8)
    assert n <= 64
    return c, r, col, m, f


def _reference():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes.npz"), allow_pickle=False)
    return tuple(np.array(z[f"reference_{k}"]) for k in ("centers", "radii", "colors", "materials", "fuzz"))


def _crowd(count=30, seed=3, far=False):
    """Well-formed filler: build_accel keeps a scene of 32 spheres or fewer in one flat
    list, so every variant is filled past that with small balls resting on the ground
    behind the odd ones (far: 60 units away instead, out of every path's reach).  Their
    radii keep 4 x the median radius above the odd balls' sizes, so those are culled as
    cluster members and not kept in the always-tested list."""
    rng = np.random.default_rng(seed)
    balls = []
    for i in range(count):
        r = float(rng.uniform(0.25, 0.38))
        x, z = float(rng.uniform(-3.5, 3.5)), float(rng.uniform(0.6, 4.5))
        c = [x + 60.0, 60.0 + r, z] if far else [x, r - 0.5, z]
        balls.append((c, r, [float(v) for v in rng.uniform(30, 250, 3)], (DIFFUSE, DIFFUSE, MIRROR, GLASS)[i % 4],
                      float(rng.uniform(0, 0.4))))
    return balls


def _variant(family, name, balls, odd, crowd=True, **kw):
    balls = list(balls) + (_crowd() if crowd else [])
    return Variant(family, name, _arrays(balls), odd=tuple(odd), **kw)


# ---------------------------------------------------------------- signed_radii

def signed_radii():
    out = []
    # the hollow glass bubble: a glass ball and a concentric one of negative radius
    out.append(_variant("signed_radii", "bubble", [
        GROUND,
        ([0, 1, -1], 0.9, [255, 255, 255], GLASS, 0.0),
        ([0, 1, -1], -0.8, [255, 255, 255], GLASS, 0.0),
        ([1.4, 0.3, -0.6], 0.5, [200, 40, 40], DIFFUSE, 0.0),
        ([-1.3, 0.4, -0.8], -0.45, [40, 200, 40], MIRROR, 0.05),
    ], odd=(1, 2, 4)))
    # negative-radius diffuse and mirror balls; radii 0, -0, denormal and either side of
    # r * r = 1e-3 (0.0316^2 = 0.99856e-3, 0.0317^2 = 1.00489e-3) right before the camera
    out.append(_variant("signed_radii", "negative_and_tiny", [
        GROUND,
        ([-0.8, 0.9, -1.2], -0.7, [220, 120, 30], DIFFUSE, 0.0),
        ([0.8, 0.9, -1.2], -0.7, [230, 230, 230], MIRROR, 0.1),
        ([0.0, 1.0, -2.5], 0.0, [255, 0, 0], DIFFUSE, 0.0),
        ([0.1, 1.0, -2.5], -0.0, [255, 0, 0], DIFFUSE, 0.0),
        ([-0.1, 1.0, -2.5], 1e-40, [255, 0, 0], DIFFUSE, 0.0),
        ([0.0, 1.05, -2.9], 0.0316, [255, 0, 0], DIFFUSE, 0.0),
        ([0.0, 0.95, -2.9], 0.0317, [0, 255, 0], DIFFUSE, 0.0),
        ([0.0, 1.0, -2.8], -0.0317, [0, 0, 255], MIRROR, 0.0),
        ([0.0, 0.2, -1.6], -0.35, [255, 255, 255], GLASS, 0.0),
    ], odd=range(1, 10)))
    # a seeded field of balls whose radii take either sign
    rng = np.random.default_rng(11)
    balls = [GROUND]
    for i in range(40):
        neg = i % 2 == 0 and i < 36  # 18 of 41 radii negative: the median radius stays positive
        x, z = rng.uniform(-2.0, 2.0), (rng.uniform(-1.8, -0.6) if neg else rng.uniform(-0.4, 2.0))
        r = rng.uniform(0.15, 0.45) * (-1.0 if neg else 1.0)
        balls.append(([x, abs(r) - 0.5 + rng.uniform(0, 1.6), z], r, list(rng.uniform(20, 255, 3)),
                      (DIFFUSE, MIRROR, GLASS)[i % 3], float(rng.uniform(0, 0.3))))
    out.append(_variant("signed_radii", "field", balls, odd=[i + 1 for i in range(0, 36, 2)], crowd=False))
    return out


# ---------------------------------------------------------------- nested

def nested():
    shells = [([0, 1, -1], 0.9, [255, 255, 255], GLASS, 0.0), ([0, 1, -1], 0.6, [255, 255, 255], GLASS, 0.0)]
    crossing = [([-0.4, 1, -1], 0.8, [255, 255, 255], GLASS, 0.0), ([0.4, 1, -1], 0.8, [255, 255, 255], GLASS, 0.0)]
    poke = [([0, 1, -1], 0.8, [255, 255, 255], GLASS, 0.0), ([0.5, 1.0, -1.2], 0.5, [220, 60, 60], DIFFUSE, 0.0)]
    mirror_in = [([0, 1, -1], 0.9, [255, 255, 255], GLASS, 0.0), ([0, 1, -1], 0.4, [240, 240, 240], MIRROR, 0.05),
                 ([0.9, 0.6, -1.3], 0.45, [240, 240, 240], MIRROR, 0.0)]
    side = [([1.6, 0.2, -0.4], 0.7, [60, 200, 90], DIFFUSE, 0.0), ([-1.5, 0.1, -0.5], 0.6, [230, 230, 230], MIRROR, 0.2)]
    out = [
        _variant("nested", "shells", [GROUND] + shells + side, odd=(1, 2)),
        _variant("nested", "crossing", [GROUND] + crossing + side, odd=(1, 2)),
        _variant("nested", "poke", [GROUND] + poke + side, odd=(1, 2)),
        _variant("nested", "mirror_in_glass", [GROUND] + mirror_in + side, odd=(1, 2, 3)),
        # the eye inside a diffuse ball (the crossing glass pair in view behind it)
        _variant("nested", "eye_in_diffuse", [GROUND] + crossing + [([0, 1, -2.7], 1.0, [200, 200, 60], DIFFUSE, 0.0)] + side,
                 odd=(1, 2, 3)),
        # the eye exactly on a ball's surface: centre (0, 1, -2), radius 1, eye (0, 1, -3)
        _variant("nested", "eye_on_surface", [GROUND] + poke + [([0, 1, -2], 1.0, [60, 200, 200], DIFFUSE, 0.0)] + side,
                 odd=(1, 2, 3)),
        # the eye at a ball's centre, and inside a glass and a mirror ball at once
        _variant("nested", "eye_at_centre", [GROUND] + shells + [([0, 1, -3], 0.5, [200, 60, 200], DIFFUSE, 0.0),
                                                                 ([0.2, 1.1, -3.1], 0.9, [255, 255, 255], GLASS, 0.0),
                                                                 ([-0.1, 0.8, -2.8], 1.2, [240, 240, 240], MIRROR, 0.0)] + side,
                 odd=(1, 2, 3, 4, 5)),
    ]
    return out


# ---------------------------------------------------------------- ties_mixed

def _tie_grid(first_then_second):
    mats = (DIFFUSE, MIRROR, GLASS, SKYBOX)
    cols = {DIFFUSE: [220, 80, 40], MIRROR: [235, 235, 235], GLASS: [255, 255, 255], SKYBOX: [10, 10, 10]}
    firsts, seconds = [], []
    for a, ma in enumerate(mats):
        for b, mb in enumerate(mats):
            centre = [-0.9 + 0.6 * a, 0.1 + 0.6 * b, -1.4]
            firsts.append((centre, 0.29, cols[ma], ma, 0.05 if ma == MIRROR else 0.0))
            seconds.append((centre, 0.29, [255 - v for v in cols[mb]], mb, 0.3 if mb == MIRROR else 0.0))
    if first_then_second:  # every pair's first copy, then every second copy in reverse
        return [GROUND] + firsts + seconds[::-1]
    balls = [GROUND]
    for f, s in zip(firsts, seconds):
        balls += [f, s]
    return balls


def ties_mixed():
    """16 balls, each twice at the same centre and radius, the two copies' materials running
    over every ordered pair of {diffuse, mirror, glass, sky}; the lower index must win."""
    near = [GROUND]
    for k in range(6):  # the copy's radius one ulp larger or smaller instead of equal
        c = [-1.0 + 0.4 * k, 0.6 + 0.25 * (k % 2), -1.5]
        r = np.float32(0.3)
        r2 = np.nextafter(r, np.float32(1 if k % 2 else 0))
        near += [(c, float(r), [200, 50, 50], DIFFUSE, 0.0), (c, float(r2), [50, 50, 200], (MIRROR, GLASS, SKYBOX)[k % 3], 0.0)]
    return [
        _variant("ties_mixed", "pairs_adjacent", _tie_grid(False), odd=range(1, 33)),
        _variant("ties_mixed", "pairs_apart", _tie_grid(True), odd=range(1, 33)),
        _variant("ties_mixed", "one_ulp", near, odd=range(1, 13)),
    ]


# ---------------------------------------------------------------- magnitudes

def _scaled_reference(k, extra=(), eye=EYE, look=LOOK):
    c, r, col, m, f = (np.concatenate([a, b]) for a, b in zip(_reference(), _arrays(_crowd())))
    s = np.float32(2.0) ** np.float32(k)
    with np.errstate(all="ignore"):
        c, r = (c * s).astype(np.float32), (r * s).astype(np.float32)
        e = [float(np.float32(v) * s) for v in eye]
        l = [float(np.float32(v) * s) for v in look]
    if extra:
        xc, xr, xcol, xm, xf = _arrays(list(extra))
        c, r, col = np.concatenate([c, xc]), np.concatenate([r, xr]), np.concatenate([col, xcol])
        m, f = np.concatenate([m, xm]), np.concatenate([f, xf])
    return (c, r, col, m, f), e, l


def magnitudes():
    out = []
    # 2^-20: every scaled sphere has r * r below the 1e-3 threshold (the ground's is 9e-7), so
    # the scaled scene alone is all sky; an unscaled diffuse ball behind it keeps the frame live
    a, e, l = _scaled_reference(-20, extra=[([0, 0, 3], 2.0, [200, 120, 40], DIFFUSE, 0.0)])
    out.append(Variant("magnitudes", "2^-20", a, eye=e, look=l, odd=(len(a[1]) - 1,)))
    for k in (20, 40, 62):
        a, e, l = _scaled_reference(k)
        out.append(Variant("magnitudes", f"2^{k}", a, eye=e, look=l))
    # 2^64: one scene unit is sqrt(FLT_MAX), so |centre - eye|^2 is finite only within one
    # unit of the eye: the camera moves to 0.8 units before the middle row of balls and
    # looks half a unit ahead (a look-at three units away would normalise to zero)
    a, e, l = _scaled_reference(64, eye=[0.1, 1.05, -0.8, 0], look=[0.1, 1.05, -0.3, 0])
    out.append(Variant("magnitudes", "2^64", a, eye=e, look=l))
    a, e, l = _scaled_reference(0, extra=[([0, 3e19, 8], 3e19, [250, 250, 250], MIRROR, 0.0)])
    out.append(Variant("magnitudes", "radius_3e19", a, eye=e, look=l, odd=(len(a[1]) - 1,)))
    a, e, l = _scaled_reference(0, extra=[([1e30, 1.0, 2.0], 1.5, [250, 250, 250], DIFFUSE, 0.0),
                                          ([0.5, 0.5, -1e30], 1e30, [250, 120, 250], DIFFUSE, 0.0)])
    out.append(Variant("magnitudes", "centre_1e30", a, eye=e, look=l, odd=(len(a[1]) - 2, len(a[1]) - 1)))
    return out


# ---------------------------------------------------------------- nonfinite

_BAD_GEOMETRY = [
    ([NAN, 1.0, -1.0], 0.5, [255, 0, 0], DIFFUSE, 0.0),
    ([0.5, INF, -1.0], 0.5, [255, 0, 0], MIRROR, 0.0),
    ([0.5, 1.0, -INF], 0.5, [255, 0, 0], GLASS, 0.0),
    ([0.0, 1.5, -1.0], NAN, [255, 0, 0], DIFFUSE, 0.0),
    ([0.3, 1.2, 2.0], INF, [255, 0, 0], MIRROR, 0.0),
    ([-0.3, 0.8, 1.0], -INF, [255, 0, 0], GLASS, 0.0),
]


def nonfinite():
    """Each variant carries the six balls of non-finite geometry (a NaN, +inf and -inf centre
    component; a NaN, +inf and -inf radius) behind its own odd balls."""
    bad = _BAD_GEOMETRY
    fuzz = [NAN, INF, -0.3, 1.0, 2.0, 1e20]
    mirrors = [([-1.25 + 0.5 * k, 0.55 + 0.5 * (k % 2), -1.6], 0.3, [235, 235, 235], MIRROR, fz) for k, fz in enumerate(fuzz)]
    tints = [[NAN, 200, 40], [200, -60, 40], [-0.0, 120, 255], [1000.0, 30, 30]]
    diffuse = [([-0.9 + 0.6 * k, 0.7 + 0.3 * (k % 2), -1.5], 0.32, t, DIFFUSE, 0.0) for k, t in enumerate(tints)]
    glass_tint = [([0.0, 0.1, -2.0], 0.3, [NAN, -5, 1000.0], GLASS, 0.0), ([0.7, 0.1, -2.0], 0.3, [NAN, -5, 1000.0], MIRROR, 0.0)]
    mats = [([-0.8 + 0.8 * k, 0.9, -1.5], 0.42, [200, 200, 40], mb, 0.1) for k, mb in enumerate((4, 128, 255))]
    side = [([1.5, 0.1, -0.6], 0.6, [60, 200, 90], DIFFUSE, 0.0), ([-1.5, 0.1, -0.6], 0.6, [230, 230, 230], MIRROR, 0.1)]
    nb = len(bad)
    return [
        _variant("nonfinite", "fuzz", [GROUND] + bad + mirrors + side, odd=range(1, 1 + nb + len(mirrors))),
        _variant("nonfinite", "colours", [GROUND] + bad + diffuse + glass_tint + side, odd=range(1, 1 + nb + 6)),
        _variant("nonfinite", "materials", [GROUND] + bad + mats + side, odd=range(1, 1 + nb + 3)),
    ]


# ---------------------------------------------------------------- sky_bytes

def sky_bytes():
    ref = tuple(np.concatenate([a, b]) for a, b in zip(_reference(), _arrays(_crowd())))
    return [Variant("sky_bytes", "over_and_under", ref, sky=[300.0, -5.0, 1e10, 0.0]),
            Variant("sky_bytes", "nan_and_wrap", ref, sky=[NAN, 255.5, 65535.0, 0.0])]


# ---------------------------------------------------------------- spec_cap

# A ray that starts inside a ball never meets it (Collision.hpp:49-56 takes the near root,
# which lies behind such an origin, and :98 rejects it), so one closed mirror ball around
# the eye traps nothing.  The room is six overlapping mirror balls of radius 20 (fuzz 0)
# whose caps face a cube of half-width 2 around (0, 1, 0), with one diffuse ball of radius
# RHO inside: a path bounces from wall to wall until it meets the small ball, about
# (wall area) / (4 pi RHO^2) times.
SPEC_CAP_RHO = 0.085
SPEC_CAP_FRAME = (32, 32, 4, 2, 5)  # width, height, spp, depth, seed


def spec_cap():
    R, a = 20.0, 2.0
    walls = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            c = [0.0, 1.0, 0.0]
            c[axis] += sign * (R + a)
            walls.append((c, R, [255, 255, 255], MIRROR, 0.0))
    balls = walls + [([-0.5, 0.6, 0.9], SPEC_CAP_RHO, [200, 160, 120], DIFFUSE, 0.0)] + _crowd(far=True)
    return [_variant("spec_cap", "mirror_room", balls, odd=range(0, 7), crowd=False, eye=[0.7, 1.3, -1.1, 0.0], look=[0.0, 1.0, 0.5, 0.0],
                     frame=SPEC_CAP_FRAME)]


_BUILDERS = {"signed_radii": signed_radii, "nested": nested, "ties_mixed": ties_mixed, "sky_bytes": sky_bytes,
             "magnitudes": magnitudes, "spec_cap": spec_cap, "nonfinite": nonfinite}


def variants(family=None):
    """Every variant, in the order the GPU run takes them (non-finite inputs last)."""
    fams = FAMILIES if family is None else (family,)
    return [v for f in fams for v in _BUILDERS[f]()]


def by_id(vid):
    fam = vid.split("/")[0]
    return next(v for v in _BUILDERS[fam]() if v.id == vid)


def with_filler(v, filler_arrays):
    """The variant followed by filler spheres (the odd spheres keep the low indices)."""
    return tuple(np.concatenate([np.asarray(a), np.asarray(b)]) for a, b in zip(v.arrays, filler_arrays))


# ---------------------------------------------------------------- the GPU test's plan

AUTO = 0xFFFFFFFF  # CLUSTER_AUTO / TREE_AUTO: resolves to 8-slot leaves under a 4-ary tree (3-ary past 512 spheres)
# every variant renders on these two culling shapes ...
SHAPES_ALL = ((0, 0), (AUTO, AUTO))
# ... and the variants of PICKED (the most live of each family by the CPU test, and for
# `magnitudes` the two whose flat-list nodes reach the never-cull record) on these
SHAPES_PICKED = ((4, 0), (8, 0), (8, 2), (3, 16))
PICKED = {
    "signed_radii": ("signed_radii/negative_and_tiny", "signed_radii/bubble"),
    "nested": ("nested/mirror_in_glass", "nested/eye_in_diffuse"),
    "ties_mixed": ("ties_mixed/pairs_adjacent", "ties_mixed/pairs_apart"),
    "sky_bytes": ("sky_bytes/nan_and_wrap",),
    "magnitudes": ("magnitudes/2^62", "magnitudes/2^64"),
    "nonfinite": ("nonfinite/colours", "nonfinite/fuzz"),
}
# the first of each family's picks also runs without primary lists, on the wavefront
# engine, as a service job and behind filler on the three big-tree walks
FIRST = tuple(PICKED[f][0] for f in FAMILIES if f in PICKED)
# filler spheres (generate_stress) that bring the tree to the node counts of the LDS lane
# walk (64 .. 2431 nodes), the global-memory lane walk (.. 9000) and the wave's octant walk
FILLER = {"lds": 400, "global": 12500, "wave": 46000}
FILLER_SEED = 7
FILLER_REGION = (12, 36, 16, 48)  # yB, yE, xB, xE of the 64 x 48 frame: 32 x 24 pixels, at 2 spp
FILLER_SPP = 2
# the octant walk's 46 000-sphere oracle pass costs seconds per variant: one family
WAVE_WALK = ("signed_radii/negative_and_tiny",)
FILLER_CASES = [(vid, walk) for walk in ("lds", "global") for vid in FIRST] + [(vid, "wave") for vid in WAVE_WALK]

# Primary lists: off where the camera's squares leave the float range (the builder decides),
# and on with every block left to the tree walk at 2^-20 (the scaled spheres surround the
# eye at 1e-6 of the threshold scale); every other variant has blocks with lists
LISTS_OFF = ("magnitudes/2^62", "magnitudes/2^64")
LISTS_ALL_WALK = ("magnitudes/2^-20",)

# Bases 1 - c of Schlick's powf(1 - c, 5) that the oracle reaches on the `nonfinite` and
# `magnitudes` variants (tests/test_degenerate_oracle.py reads them back): the extremes of
# both ends.  No variant reaches a base outside [0, 1] or a non-finite one.
SCHLICK_BASES = ("0x1p-22", "0x1.2p-21", "0x1.14p-17", "0x1.fd38ccp-1")


def shape_for_check(k, b, n):
    """(cluster size, branching) as spt_accel_check takes them, AUTO resolved."""
    if b == AUTO:
        b = 3 if n > 512 else 4
    if k == AUTO:
        k = 8 if b >= 2 else 4
    return k, b
