"""The oracle (oracle/spt_oracle.c) against the reference's own code, bit for bit.

oracle/_ref/ref_harness (`make -C oracle ref`, run by build() where the reference's headers
are present) compiles the reference's unmodified headers behind stand-ins and calls its
functions by name; pyoracle.ref_* run it, one process per call under a 60 s limit.  CPU
tests: no GPU, no kernel.  Where neither the harness nor the reference's headers exist
the tests skip; where the headers exist and the harness does not, they fail.

The one seam is the generator's start.  The reference seeds a thread_local splitmix from
its clock; the harness sets that clock to a 32-bit seed s before it starts a fresh thread,
so the stream starts at s << 31 | s = spo_scene_state(s) (test_seam: if that fails, nothing
below means anything).  Everything else is compared through the oracle's stream entry
points (spo_trace_ray, spo_render_segment_stream, spo_render_segment_task_stream), which
share every line with the keyed functions the GPU tests use.

Outside the comparison, because the reference's own behaviour is undefined or endless:
  * scenes of more than 255 spheres (the uint8_t index of FindClosestIntersectionSphere
    never ends; the harness refuses them);
  * bytes of g_data whose colour is not within the range of the uint8_t cast in WritePixel
    (NaN or outside [0, 256) after the square root): test_segments leaves out those bytes
    only, and compares their float colours;
  * paths with more than SPO_SPECULAR_CAP specular events, where the reference recurses on
    without bound: test_paths leaves them out (family spec_cap only, at most 5% there);
  * RenderSegmentTask on a tile taller than wide, whose colorIndex writes past the end of
    its std::vector (the harness refuses it): the non-square tile is 7 wide and 5 high.
Not reachable: the sky colour (initColor is constexpr in Globals.hpp), so the degenerate
family `sky_bytes` is not compared; the frame of the two RenderSegment* functions (1440 x
1440, 100 spp, 10 bounces, constexpr too); Renderer.hpp's tiling (needs GL).
"""
import os

import numpy as np
import pytest

import degenerate_scenes as D
from cast_rays import N_RAYS, RAY_SEED, make_rays, restate_hits
from test_gpu_parity import bits

EYE, LOOK, UP, SKY = D.EYE, D.LOOK, D.UP, D.SKY
SEAM_SEEDS = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
SEAM_RANGES = ((-1, 1), (0, 1), (-.5, .5), (0, 255), (.5, 6))
GENERATOR_SEEDS = (1, 2, 3, 7, 12345, 0xFFFFFFFF)  # of test_product_scene_generator_matches_oracle
CAMERAS = ((EYE, LOOK), ([3, 2, -5, 0], [0, 0.5, 1, 0]), ([-1, 4, 2, 0], [0, 0, 0, 0]),  # of test_camera_basis_matches_oracle
           ([2, 1, -3, 0], [2, 1, -3, 0]))  # look == eye: NaNs
GOLDEN_SCENES = ("random", "reference", "cornell3")
PATHS = 2000
BOUNCES = (1, 2, 10, 50)
PATH_VARIANTS = [v for v in D.variants() if v.family != "sky_bytes"]  # another initColor: not reachable
PATH_CASES = list(GOLDEN_SCENES) + [v.id for v in PATH_VARIANTS]
# RenderSegment*: (yBegin, yEnd, xBegin, xEnd) of the 1440 x 1440 frame
# the non-square tile (colorIndex aliases its rows), the frame's last rows and columns, and
# a tile on the `reference` scene's column of mirror, glass and mirror balls, where the
# 10-pass cap drops samples (found on the CPU with spo_render_segment_task_stream; the
# first two tiles drop none in either scene, and a search of 6500 tiles over the `random`
# scene's glass and mirror balls found no dropped sample at all)
TILES = ((700, 705, 700, 707), (1437, 1440, 1437, 1440), (556, 559, 724, 727))
SEGMENT_SEEDS = (1, 0x9E3779B9)


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        if os.path.isdir(oracle.REF_INCLUDE):
            pytest.fail(f"the reference's headers are in {oracle.REF_INCLUDE} but {oracle.REF_BIN} is not built")
        pytest.skip("neither the reference's headers nor oracle/_ref/ref_harness are here")
    return oracle


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shapes {g.shape} and {w.shape}"
    bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0] if g.ndim > 1 else np.nonzero(g != w)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(g)} differ; first at {bad[0]}: reference "
                           f"{np.asarray(got)[bad[0]]!r}, oracle {np.asarray(want)[bad[0]]!r}")


def golden_scene(oracle, gs, name):
    return oracle.OracleScene(*(gs[f"{name}_{k}"] for k in ("centers", "radii", "colors", "materials", "fuzz")))


# ---------------------------------------------------------------- (a) the seam

@pytest.mark.parametrize("s", SEAM_SEEDS, ids=[hex(s) for s in SEAM_SEEDS])
def test_seam(ref, s):
    """A fresh reference thread whose clock reads s draws what spo_uniform draws from
    spo_scene_state(s)."""
    for a, b in SEAM_RANGES:
        same_bits(ref.ref_draws(s, a, b, 16), ref.uniform_draws(s, a, b, 16), f"seed {s:#x}, U({a}, {b})")


# ---------------------------------------------------------------- (b) generators

@pytest.mark.parametrize("seed", GENERATOR_SEEDS)
def test_generators(ref, seed):
    for init, want in ((False, ref.generate_spheres(seed)), (True, ref.init_spheres(seed))):
        got = ref.ref_generate(seed, init=init)
        assert got.s.n == want.s.n
        for k in ("centers", "radii", "colors", "materials", "fuzz"):  # fuzz: g_diffuses
            assert np.array_equal(getattr(got, k).view(np.uint8), getattr(want, k).view(np.uint8)), (init, k)


# ---------------------------------------------------------------- (c) camera

@pytest.mark.parametrize("eye,look", CAMERAS)
def test_camera(ref, eye, look):
    got, want = ref.ref_camera(eye, look, UP), ref.camera_basis(eye, look, UP)
    if eye == look:
        assert np.isnan(want).any()
    same_bits(got, want, f"camera {eye} -> {look}")


# ---------------------------------------------------------------- (d) geometry

def test_geometry(ref, golden_scenes):
    """All 4099 rays of the cast test's mix on the golden `random` scene: the sphere found,
    the hit's contact point, factor and normal, and RaySphereIntersection of the sphere
    that kinds C and D aim at."""
    gs = golden_scenes
    sc = golden_scene(ref, gs, "random")
    n_s = sc.s.n
    assert n_s == 149
    o, d, kind, aim = make_rays(sc.centers, sc.radii)
    n = len(o)
    assert n == N_RAYS == 4099
    want_idx = np.array([ref.find_closest(sc, d[i], o[i]) for i in range(n)], np.uint32)
    hit = want_idx < n_s
    aimed = aim >= 0
    passes = np.zeros(n, bool)
    for i in np.nonzero(aimed)[0]:
        passes[i] = ref.probe_sphere(sc, aim[i], d[i], o[i])[0]
    # the mix is live (the assertions of tests/test_gpu_cast.py)
    c, dk = kind == "C", kind == "D"
    figures = dict(hits=hit.mean(), c_pass=passes[c].mean(), c_win=(want_idx[c] == aim[c]).mean(), d_pass=passes[dk].mean())
    assert 0.5 <= figures["hits"] <= 0.9, figures
    assert 1.0 - figures["hits"] >= 0.10, figures
    assert 0.35 <= figures["c_pass"] <= 0.65, figures
    assert figures["c_win"] >= 0.25, figures
    assert 0.35 <= figures["d_pass"] <= 0.65, figures

    idx, rec, rsi = ref.ref_geometry(sc, o, d, aim)
    bad = np.nonzero(idx != want_idx)[0]
    assert bad.size == 0, (f"{bad.size} rays find another sphere; first ray {bad[0]} (kind {kind[bad[0]]}): reference "
                           f"{idx[bad[0]]}, oracle {want_idx[bad[0]]}")
    assert np.array_equal(rsi[aimed], passes[aimed]), "RaySphereIntersection of the aimed sphere"
    assert not rsi[~aimed].any()
    t, P, nrm = restate_hits(sc.centers, sc.radii, want_idx[hit], o[hit], d[hit])
    ds = np.array([ref.probe_sphere(sc, want_idx[i], d[i], o[i])[1] for i in np.nonzero(hit)[0]], np.float32)
    same_bits(rec[hit, 0:3], P, "contact point")
    same_bits(rec[hit, 4], t, "contact factor t")
    same_bits(rec[hit, 5:8], nrm, "contact normal")
    same_bits(rec[hit, 9], ds, "squared distance")
    assert not bits(rec[hit, 3]).any() and not bits(rec[hit, 8]).any(), "w lanes of contact point and normal"
    assert not bits(rec[~hit]).any()


def with_w_lanes(o, d, rng):
    """The rays with a fourth component: _mm_dp_ps sums all four products and Normalize
    divides all four lanes, which rays of w = 0 never show."""
    o, d = o.copy(), d.copy()
    o[:, 3] = rng.uniform(-0.25, 0.25, len(o))
    d[:, 3] = rng.uniform(-0.25, 0.25, len(d))
    return o, d


def test_geometry_w_lanes(ref, golden_scenes):
    """The first 1024 rays of the mix with non-zero w lanes in origin and direction: the
    sphere found, RaySphereIntersection, and the squared distance that is compared."""
    sc = golden_scene(ref, golden_scenes, "random")
    o, d, kind, aim = make_rays(sc.centers, sc.radii)
    o, d = with_w_lanes(o[:1024], d[:1024], np.random.default_rng(77))
    aim = aim[:1024]
    want_idx = np.array([ref.find_closest(sc, d[i], o[i]) for i in range(len(o))], np.uint32)
    flat_idx = np.array([ref.find_closest(sc, d[i] * [1, 1, 1, 0], o[i] * [1, 1, 1, 0]) for i in range(len(o))], np.uint32)
    hit = want_idx < sc.s.n
    assert 0.3 <= hit.mean() <= 0.9 and (want_idx != flat_idx).mean() >= 0.02  # the w lanes decide some rays
    idx, rec, rsi = ref.ref_geometry(sc, o, d, aim)
    assert np.array_equal(idx, want_idx)
    aimed = aim >= 0
    probes = [ref.probe_sphere(sc, aim[i], d[i], o[i]) for i in np.nonzero(aimed)[0]]
    assert np.array_equal(rsi[aimed], np.array([p[0] for p in probes]))
    ds = np.array([ref.probe_sphere(sc, want_idx[i], d[i], o[i])[1] for i in np.nonzero(hit)[0]], np.float32)
    same_bits(rec[hit, 9], ds, "squared distance")
    assert bits(rec[hit, 3]).any() and bits(rec[hit, 8]).any()


# ---------------------------------------------------------------- the fixture of tests/test_gpu_cast.py

def reference_casts():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_casts.npz")
    return dict(np.load(path, allow_pickle=False))


def test_reference_casts_fixture(golden_scenes):
    """tests/golden/reference_casts.npz (make_golden.py --reference-casts, the reference's own
    answers): its rays are make_rays' on the golden `random` scene, and it has hits and misses."""
    f = reference_casts()
    n = len(f["idx"])
    assert 1000 <= n <= N_RAYS
    o, d, _, _ = make_rays(golden_scenes["random_centers"], golden_scenes["random_radii"], n=n, seed=RAY_SEED)
    assert np.array_equal(bits(f["o"]), bits(o)) and np.array_equal(bits(f["d"]), bits(d))
    hit = f["idx"] < len(golden_scenes["random_radii"])
    assert hit.sum() >= n // 2 and (~hit).sum() >= n // 10
    assert f["hit"].shape == (n, 2, 4) and not bits(f["hit"][~hit]).any()
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_casts.npz")) \
        <= os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden.npz"))


def test_reference_casts_fixture_regenerates(ref, golden_scenes):
    """The fixture is what the harness answers today."""
    f = reference_casts()
    sc = golden_scene(ref, golden_scenes, "random")
    idx, rec, _ = ref.ref_geometry(sc, f["o"], f["d"], np.full(len(f["o"]), -1, np.int32))
    assert np.array_equal(idx, f["idx"])
    same_bits(rec[:, [0, 1, 2, 4, 5, 6, 7, 9]], f["hit"].reshape(-1, 8), "hit records")


# ---------------------------------------------------------------- (e) paths

def admits_cast_rays(centers, radii):
    """make_rays needs finite geometry whose squares stay finite in float32, and a sphere
    for its kinds C and D to aim at."""
    c, r = np.asarray(centers, np.float64)[:, :3], np.asarray(radii, np.float64)
    return bool(np.isfinite(c).all() and np.isfinite(r).all() and max(np.abs(c).max(), np.abs(r).max()) < 1e15
                and (r * r > 4e-3).any())


def path_case(oracle, gs, case):
    """(scene, frame, family) of a case: the frame gives the eye, the view and the pixel grid."""
    if case in GOLDEN_SCENES:
        sc = golden_scene(oracle, gs, case)
        return sc, oracle.make_frame(gs["view"], EYE, SKY, 200, 100, 1, 10, 1), None
    v = D.by_id(case)
    assert len(v.arrays[1]) <= 255
    W, H, _, depth, seed = v.frame
    assert list(v.sky) == [float(x) for x in SKY]
    view = oracle.camera_basis(v.eye, v.look, UP)
    return oracle.OracleScene(*v.arrays), oracle.make_frame(view, v.eye, v.sky, W, H, 1, depth, seed), v.family


def path_rays(oracle, sc, fr, seed, count=PATHS):
    """count rays: half the scene's own primary rays (the oracle's, through a grid of its
    frame's pixels), half the cast mix where the scene admits it (else primary rays too)."""
    mix = count // 2 if admits_cast_rays(sc.centers, sc.radii) else 0
    prim = count - mix
    pix = np.linspace(0, fr.width * fr.height - 1, prim).astype(np.int64)
    xy = np.stack([pix % fr.width, pix // fr.width], axis=1)
    d = oracle.primary_rays(fr, xy, seed)
    o = np.tile(np.array(list(fr.eye), np.float32), (prim, 1))
    if mix:
        mo, md, _, _ = make_rays(sc.centers, sc.radii, n=mix, seed=seed)
        o, d = np.concatenate([o, mo]), np.concatenate([d, md])
    return o, d


@pytest.mark.parametrize("case", PATH_CASES)
def test_paths(ref, golden_scenes, case):
    """TraceAndSampleColor(d, o, bounces) against spo_trace_ray, 2000 paths a scene, each on
    its own seed."""
    sc, fr, family = path_case(ref, golden_scenes, case)
    rng = np.random.default_rng(PATH_CASES.index(case) + 100)
    # the mirror room cuts about a quarter of such paths at the specular cap: it starts from
    # three times the rays, and below keeps the first PATHS of them that hold at most 4% cut
    o, d = path_rays(ref, sc, fr, seed=int(rng.integers(1, 1 << 31)), count=PATHS * (3 if family == "spec_cap" else 1))
    order = rng.permutation(len(o))  # primary and mixed rays interleaved
    o, d = o[order], d[order]
    # and a tenth as many again with w lanes, which the tracers carry through Dot and Normalize
    wo, wd = with_w_lanes(o[:len(o) // 10], d[:len(o) // 10], rng)
    o, d = np.concatenate([o, wo]), np.concatenate([d, wd])
    n = len(o)
    seeds = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    seeds[:4] = (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
    assert (seeds >= 1 << 31).sum() > n // 4
    bounces = np.array([BOUNCES[i % len(BOUNCES)] for i in range(n)], np.uint32)
    want, info = ref.trace_rays(sc, fr, d, o, bounces, seeds)
    ev = {k: info[:, 2 + i] for i, k in enumerate(ref.EV)}
    # paths cut at SPO_SPECULAR_CAP are outside the comparison: the reference has no cap and
    # would recurse on.  Only the mirror room may have them, and few
    cut = info[:, 1] != 0
    assert np.array_equal(cut, ev["cut"] != 0)
    if family == "spec_cap":
        chosen = np.nonzero(~cut | (np.cumsum(cut) <= PATHS * 4 // 100))[0][:PATHS]
        o, d, seeds, bounces, want, info, cut = (a[chosen] for a in (o, d, seeds, bounces, want, info, cut))
        n = len(chosen)
        assert cut.any() and (info[~cut, 0] > 512).any()  # the cap is met, and long paths are compared
        assert cut.mean() <= 0.05, f"{cut.sum()} of {n} paths are cut at the cap"
    else:
        assert not cut.any(), f"{cut.sum()} paths of {case} are cut at the cap"
    if family is None:  # a well-formed scene: every kind of event and both endings occur
        seen = {k: int((v > 0).sum()) for k, v in ev.items()}
        for k in ("diffuse", "mirror", "glass_reflect", "refract_twice", "tir", "end_bounces", "end_sky"):
            assert seen[k] >= 1, (k, seen)
    assert n >= PATHS
    keep = ~cut
    got = ref.ref_trace(sc, d[keep], o[keep], bounces[keep], seeds[keep])
    same_bits(got, want[keep], f"{case}: path colours")


# ---------------------------------------------------------------- (f) segments

def g_index(x, y, W=1440, H=1440):
    return W * H * 3 - ((W - x) * 3 + y * W * 3)


@pytest.mark.parametrize("task", [False, True], ids=["RenderSegment", "RenderSegmentTask"])
@pytest.mark.parametrize("name", ["random", "reference"])
def test_segments(ref, golden_scenes, name, task):
    """RenderSegment / RenderSegmentTask of the reference's frame (1440 x 1440, 100 spp, 10
    bounces) on one thread against the oracle's stream functions: every colour handed to
    WritePixel, its index, and the whole of g_data."""
    sc = golden_scene(ref, golden_scenes, name)
    view = golden_scenes["view"]
    fr = ref.make_frame(view, EYE, SKY, ref.REF_WIDTH, ref.REF_HEIGHT, ref.REF_SPP, ref.REF_BOUNCES, 0)
    dropped_total = 0
    for seed in SEGMENT_SEEDS:
        for yB, yE, xB, xE in TILES:
            what = f"{name}, seed {seed:#x}, tile y {yB}..{yE - 1} x {xB}..{xE - 1}"
            rgba, g_want, dropped = ref.render_segment_stream(sc, fr, yB, yE, xB, xE, seed, task=task)
            dropped_total += dropped
            index, color, g = ref.ref_segment(sc, view, EYE, yB, yE, xB, xE, seed, task=task)
            want_index = [g_index(x, y) for y in range(yB, yE) for x in range(xB, xE)]
            assert list(index) == want_index, what
            same_bits(color, rgba, what + ": colours handed to WritePixel")
            # the uint8_t cast of a value that is NaN or outside [0, 256) is undefined in the
            # reference: those bytes (the slots RenderSegmentTask's colorIndex never reaches
            # on the non-square tile, 0 / 0 = NaN) are not compared; all others are,
            # over the whole frame, so that a write outside the tile shows
            with np.errstate(all="ignore"):
                v = np.round(np.sqrt(rgba[:, :3] / np.float32(255)) * np.float32(255))
            defined = (v >= 0) & (v < 256)
            if not task:
                assert defined.all(), what
            else:
                assert defined.all(axis=1).sum() >= len(rgba) * 3 // 4, what
            skip = np.zeros(len(g), bool)
            for p in np.nonzero(~defined.all(axis=1))[0]:
                for ch in np.nonzero(~defined[p])[0]:
                    skip[want_index[p] + ch] = True
            assert np.array_equal(g[~skip], g_want[~skip]), what + ": g_data"
            assert g_want.any()
    if task and name == "reference":  # the 10-pass cap is exercised: these tiles have samples it drops
        assert dropped_total >= 1, f"{name}: no sample is dropped by the pass cap on these tiles"
