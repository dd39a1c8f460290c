"""Temporal accumulation under moving spheres (spt_temporal_motion[_async]) against its
definition, bit for bit (include/spt_hip.h "temporal accumulation under moving spheres",
DESIGN.md §4.15), and the accumulator that drives it (TemporalAccumulator(scene=..., resident=...)).

What the call must return comes from tests/temporal_motion.py (numpy), with Minv from
spt_temporal_inverse.  The frames are tests/test_temporal_motion_helper.py's: scene A (the
golden `random` scene, the history, seed 3) and scene B (its three large spheres and a third of
its small ones moved, the current frame, seed 4), rendered by the oracle.  Every test asserts
on the helper's answer that its case is live before it compares anything; no comparison has a
tolerance.

    1  the A/B pair at 45 x 37 x 7, moving and static camera      the rule finds history the plain call misses
    2  the static camera with prev_eye one ulp off                the per-pixel static rule beside the general path
    3  an unmoved table; n_spheres == 0 with a null table         spt_temporal's own GPU output
    4  1x1, 1x40, 40x1, 33x18 at 2 spp                            ragged tiles
    5  ids rewritten to n and to 0xFFFFFFFF                       no record is read, the plain path
    6  degenerate and awkward records                             pass through, or the plain tests decide
    7  device pointers on two caller streams, a device table      the async form
    8  argument errors                                            the new ones, outputs untouched
    9  A -> B -> A' through TemporalAccumulator(scene=...); resident against non-resident
    10 a render, a motion call, the same render
"""
import ctypes

import numpy as np
import pytest

from temporal import DEFAULTS, expected_temporal, yawed
from temporal_motion import expected_temporal_motion
from test_gpu_cast import COUNTERS
from test_gpu_denoise import same
from test_gpu_features import DEPTH, SEED, make_ctx
from test_gpu_parity import SKY, bits
from test_gpu_temporal import SHAPES, history_of, moved
from test_temporal_helper import camera
from test_temporal_motion_helper import BIG, PAIRS, pair, scene_of, table

pytestmark = pytest.mark.gpu

F = np.float32
W1, H1, S1 = 45, 37, 7
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ctx(spt):
    """A context without scene, camera or params: the accumulation needs none."""
    c = spt.Context(0)
    yield c
    c.close()


def want(spt, cur, prev, motion, **kw):
    """The helper's answer for frame `cur` against the history frame `prev` under `motion`."""
    H, W = cur["ids"].shape
    return expected_temporal_motion(cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"], W, H, motion,
                                    history_of(prev), prev["view"], prev["eye"], spt.temporal_inverse(prev["view"]), **kw)


def want_plain(spt, cur, prev, **kw):
    H, W = cur["ids"].shape
    return expected_temporal(cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"], W, H,
                             history_of(prev), prev["view"], prev["eye"], spt.temporal_inverse(prev["view"]), **kw)


def got(ctx, cur, prev, motion=None, **kw):
    """The device's answer; motion None: the plain call."""
    if motion is not None:
        kw["motion"] = motion
    return ctx.temporal(cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"], history_of(prev),
                        prev["view"], prev["eye"], **kw)


def check(ctx, cur, prev, motion, exp, what, **kw):
    out, out_mom = got(ctx, cur, prev, motion, **kw)
    same(out, exp[0], f"{what}: out_rgba")
    same(out_mom, exp[1], f"{what}: out_mom")
    return out, out_mom


# ---------------------------------------------------------------- 1: the A/B pair

@pytest.mark.parametrize("cams", list(PAIRS), ids=list(PAIRS))
def test_the_pair_of_scenes_with_the_defaults(ctx, spt, oracle, golden_scenes, cams):
    prev, cur = pair(oracle, golden_scenes, W1, H1, S1, PAIRS[cams])
    motion = table(golden_scenes)
    exp, plain = want(spt, cur, prev, motion, **DEFAULTS), want_plain(spt, cur, prev, **DEFAULTS)
    mv = exp[2]["mv"]
    found = int((exp[2]["has"] & mv).sum()), int((plain[2]["has"] & mv).sum())
    print(f"motion {cams} 45x37x7: {int(mv.sum())} mv pixels, history on {found[0]} of them (plain {found[1]})")
    assert mv.sum() >= 300 and found[0] >= 2 * found[1] and (moved(exp, plain) & mv).sum() >= 100
    assert not (moved(exp, plain) & ~mv).any()
    check(ctx, cur, prev, motion, exp, f"{cams} camera", **DEFAULTS)


# ---------------------------------------------------------------- 2: the static rule, per pixel

def test_the_static_rule_per_pixel_and_the_path_one_ulp_beside_it(ctx, spt, oracle, golden_scenes):
    prev, cur = pair(oracle, golden_scenes, W1, H1, S1, PAIRS["static"])
    motion = table(golden_scenes)
    exp = want(spt, cur, prev, motion, **DEFAULTS)
    mv = exp[2]["mv"]
    ys, xs = np.mgrid[0:H1, 0:W1]
    at_home = (exp[2]["fx"] == xs) & (exp[2]["fy"] == ys)
    assert at_home[~mv].all() and (~at_home[mv]).mean() > 0.9 and mv.any() and (~mv).any()
    eye = prev["eye"].copy()
    eye[2] = np.nextafter(eye[2], F(0))
    off = dict(prev, eye=eye)
    exp2 = want(spt, cur, off, motion, **DEFAULTS)
    n = int((moved(exp, exp2) & ~mv).sum())
    print(f"static 45x37x7: prev_eye one ulp off moves {n} pixels whose sphere stood still")
    assert n >= 1 and not np.array_equal(exp2[2]["fx"][~mv], xs.astype(F)[~mv])
    check(ctx, cur, off, motion, exp2, "one ulp off the static rule", **DEFAULTS)


# ---------------------------------------------------------------- 3: equals the plain call

@pytest.mark.parametrize("cams", list(PAIRS), ids=list(PAIRS))
def test_a_table_without_motion_is_the_plain_call(ctx, spt, oracle, golden_scenes, cams):
    prev, cur = pair(oracle, golden_scenes, W1, H1, S1, PAIRS[cams])
    plain = got(ctx, cur, prev, **DEFAULTS)  # spt_temporal's own output on the device
    assert (bits(plain[0]) != bits(cur["rgba"])).any()
    for what, motion in (("unmoved table", table(golden_scenes, "B", "B")), ("n_spheres == 0, null table", np.zeros((0, 8), F))):
        exp = want(spt, cur, prev, motion, **DEFAULTS)
        assert not exp[2]["mv"].any()
        out, out_mom = check(ctx, cur, prev, motion, exp, what, **DEFAULTS)
        same(out, plain[0], f"{what} against spt_temporal: out_rgba")
        same(out_mom, plain[1], f"{what} against spt_temporal: out_mom")


# ---------------------------------------------------------------- 4: shapes

MOTION_SHAPES = [(1, 1), (1, 40), (40, 1), (33, 18)]


@pytest.mark.parametrize("shape", MOTION_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_and_ragged_shapes(ctx, spt, oracle, golden_scenes, shape):
    W, H = shape
    yaw, eye = SHAPES[shape]
    cam2 = (yawed(camera(golden_scenes, 0)[0], yaw), np.asarray(eye, F))
    prev, cur = pair(oracle, golden_scenes, W, H, 2, cams=(0, cam2))
    motion = table(golden_scenes)
    if min(W, H) == 1:  # a frame one pixel wide or high sees none of scene B's moved spheres: every other sphere drifts
        still = (motion[:, :4] == motion[:, 4:]).all(axis=1)
        motion[still, 4:7] -= np.asarray([0.02, 0.0, 0.01], F)
    exp, plain = want(spt, cur, prev, motion, **DEFAULTS), want_plain(spt, cur, prev, **DEFAULTS)
    mv, has = exp[2]["mv"], exp[2]["has"]
    print(f"motion {W}x{H}x2: {int(mv.sum())} mv pixels, {int((mv & has).sum())} of them with history, "
          f"{int((~mv & has).sum())} others with history, {int(moved(exp, plain).sum())} differ from the plain definition")
    # (1 x 1: a moved sphere's pixel that seeks history and finds none; 1 x 40: one such pixel above 39 of sky, which
    # find theirs by the plain path; 40 x 1: every pixel on a moved sphere)
    assert mv.any() and exp[2]["sought"][mv].any()
    if W * H > 1:
        assert has.any()
    if W > 1:
        assert (mv & has).any() and moved(exp, plain).any()
    if W * H > 500:
        assert (mv & has).sum() >= 10 and (~mv & has).any()
    check(ctx, cur, prev, motion, exp, f"{W}x{H}x2", **DEFAULTS)


# ---------------------------------------------------------------- 5: ids outside the table

def test_ids_outside_the_table_read_no_record(ctx, spt, oracle, golden_scenes):
    prev, cur = pair(oracle, golden_scenes, W1, H1, S1, PAIRS["moving"])
    motion = table(golden_scenes)
    n = len(motion)
    base = want(spt, cur, prev, motion, **DEFAULTS)
    # sphere 2's pixels carry the miss sentinel, sphere 1's 0xFFFFFFFF, in both frames (the taps still match)
    relabel = {2: n, 1: 0xFFFFFFFF}
    c, h = dict(cur, ids=cur["ids"].copy()), dict(prev, ids=prev["ids"].copy())
    for f, src in ((c, cur), (h, prev)):
        for k, v in relabel.items():
            f["ids"][src["ids"] == k] = v
    exp, plain = want(spt, c, h, motion, **DEFAULTS), want_plain(spt, c, h, **DEFAULTS)
    out_of_table = (c["ids"] >= n) & (c["feat"][:, :, 0, 3] > 0)
    for v in relabel.values():
        sel = (c["ids"] == v) & (c["feat"][:, :, 0, 3] > 0)
        assert sel.sum() >= 20 and base[2]["mv"][sel & (cur["ids"] != n)].all() and not exp[2]["mv"][sel].any(), v
        assert (exp[2]["has"] & sel).any(), "the plain path still finds history there"
    assert (moved(exp, base) & out_of_table).sum() >= 10 and not moved(exp, plain)[out_of_table].any()
    assert exp[2]["mv"].any(), "the small spheres still move"
    check(ctx, c, h, motion, exp, "ids outside the table", **DEFAULTS)


# ---------------------------------------------------------------- 6: degenerate and awkward records

def records(golden_scenes):
    """{case: (table, spheres changed)}: scene A -> B's table with the records of the three
    large spheres (and for some cases every sphere) replaced."""
    base = table(golden_scenes)
    big = list(BIG)
    out = {}

    def case(name, edit, which=big):
        t = base.copy()
        for k in which:
            edit(t[k])
        out[name] = (t, which)

    def put(lanes, value):
        def edit(rec):
            rec[lanes] = value
        return edit

    case("r = 0", put([3], 0.0))
    case("rp = 0", put([7], 0.0))
    case("r = rp = 0", put([3, 7], 0.0))
    case("NaN centre", put([1], np.nan))
    case("NaN previous centre", put([5], np.nan))
    case("infinite centre", put([0], np.inf))
    case("infinite previous centre", put([6], -np.inf))
    case("NaN radius", put([3], np.nan))
    case("infinite radius", put([3], np.inf))
    case("infinite previous radius", put([7], np.inf))
    case("every record NaN", put(slice(None), np.nan), list(range(len(base))))

    def negate(rec):
        rec[3], rec[7] = -rec[3], -rec[7]
    case("both radii negative", negate)
    case("radii of opposite sign", lambda rec: rec.__setitem__(7, -rec[7]))

    def radius_only(rec):
        rec[4:7] = rec[0:3]
        rec[7] = rec[3] * F(0.8)
    case("a radius-only change", radius_only)
    case("behind the previous camera", lambda rec: rec.__setitem__(6, F(-20.0)))
    case("off the previous image", lambda rec: rec.__setitem__(4, rec[0] + F(80.0)))
    return out


RECORD_CASES = ["r = 0", "rp = 0", "r = rp = 0", "NaN centre", "NaN previous centre", "infinite centre",
                "infinite previous centre", "NaN radius", "infinite radius", "infinite previous radius", "every record NaN",
                "both radii negative", "radii of opposite sign", "a radius-only change", "behind the previous camera",
                "off the previous image"]
# what the helper says becomes of the pixels of the spheres changed: they all pass through
# ("none", every case not listed), some still find history ("some"), the taps' own tests decide
# ("any": s == 0 carries every point to the previous centre, s < 0 to the sphere's far side), or the answer is the A -> B
# table's ("same": rp / r is what it was)
RECORD_HISTORY = {"both radii negative": "same", "a radius-only change": "some", "rp = 0": "any", "infinite radius": "any",
                  "radii of opposite sign": "any"}


@pytest.mark.parametrize("name", RECORD_CASES)
def test_degenerate_and_awkward_records(ctx, spt, oracle, golden_scenes, name):
    prev, cur = pair(oracle, golden_scenes, W1, H1, S1, PAIRS["moving"])
    motion, which = records(golden_scenes)[name]
    base = want(spt, cur, prev, table(golden_scenes), **DEFAULTS)
    exp = want(spt, cur, prev, motion, **DEFAULTS)
    sel = np.isin(cur["ids"], which) & (cur["feat"][:, :, 0, 3] > 0)
    mv, has, sought = exp[2]["mv"], exp[2]["has"], exp[2]["sought"]
    print(f"records, {name}: {int(sel.sum())} pixels of the spheres changed, {int((sel & sought).sum())} seek history, "
          f"{int((sel & has).sum())} find it; {int(moved(exp, base).sum())} pixels differ from the A -> B table's answer")
    assert sel.sum() >= 100 and mv[sel].all(), "the records changed are read as moved"
    kind = RECORD_HISTORY.get(name, "none")
    assert (not moved(exp, base).any() and (sel & has).sum() >= 100) if kind == "same" else moved(exp, base).sum() >= 10
    assert not moved(exp, base)[~sel].any()
    if kind == "none":
        assert not (sel & has).any()
        assert np.array_equal(bits(exp[0][sel]), bits(cur["rgba"][sel])) and np.array_equal(bits(exp[1][sel]), bits(cur["mom"][sel]))
    elif kind == "some":
        assert (sel & has).sum() >= 10
    assert np.isfinite(exp[0]).all() and np.isfinite(exp[1]).all(), "nothing spreads"
    check(ctx, cur, prev, motion, exp, name, **DEFAULTS)


# ---------------------------------------------------------------- 7: device pointers, two streams

def test_device_pointers_on_two_streams_with_a_device_table(ctx, spt, oracle, golden_scenes):
    import torch
    dev = torch.device("cuda", 0)
    calls = []
    for cams, kw, motion in (("moving", dict(DEFAULTS), table(golden_scenes)),
                             ("static", dict(tol_normal=float("inf"), tol_depth=0.05, max_history=3.0),
                              records(golden_scenes)["a radius-only change"][0])):
        prev, cur = pair(oracle, golden_scenes, W1, H1, S1, PAIRS[cams])
        t = {k: torch.from_numpy(np.ascontiguousarray(cur[k])).to(dev) for k in ("rgba", "mom", "feat")}
        t["ids"] = torch.from_numpy(cur["ids"].astype(np.int32)).to(dev)
        th = {k: torch.from_numpy(np.ascontiguousarray(prev[k])).to(dev) for k in ("rgba", "mom", "feat")}
        th["ids"] = torch.from_numpy(prev["ids"].astype(np.int32)).to(dev)
        calls.append(dict(cur=cur, prev=prev, kw=kw, t=t, th=th, motion=motion, table=torch.from_numpy(motion).to(dev),
                          stream=torch.cuda.Stream(device=dev),
                          out=torch.full((H1, W1, 4), -1.0, dtype=torch.float32, device=dev),
                          mom=torch.full((H1, W1, 4), -2.0, dtype=torch.float32, device=dev)))
    for k in calls:
        k["stream"].wait_stream(torch.cuda.current_stream(dev))
    for k in calls:  # both enqueued before either is waited for
        t, th = k["t"], k["th"]
        ctx.temporal_async(W1, H1, t["rgba"].data_ptr(), t["mom"].data_ptr(), t["feat"].data_ptr(), t["ids"].data_ptr(),
                           k["cur"]["view"], k["cur"]["eye"],
                           (th["rgba"].data_ptr(), th["mom"].data_ptr(), th["feat"].data_ptr(), th["ids"].data_ptr()),
                           k["prev"]["view"], k["prev"]["eye"], d_out_rgba=k["out"].data_ptr(), d_out_mom=k["mom"].data_ptr(),
                           stream=k["stream"].cuda_stream, d_motion=k["table"].data_ptr(), n_spheres=len(k["motion"]), **k["kw"])
    for k in calls:
        k["stream"].synchronize()
    for k in calls:
        exp = want(spt, k["cur"], k["prev"], k["motion"], **k["kw"])
        assert (exp[2]["mv"] & exp[2]["has"]).sum() >= 50
        assert (moved(exp, want_plain(spt, k["cur"], k["prev"], **k["kw"])) & exp[2]["mv"]).sum() >= 50
        same(k["out"].cpu().numpy(), exp[0], "async: out_rgba")
        same(k["mom"].cpu().numpy(), exp[1], "async: out_mom")
        assert np.array_equal(bits(k["table"].cpu().numpy()), bits(k["motion"])), "the table is an input"


# ---------------------------------------------------------------- 8: argument errors

def test_the_new_argument_errors(ctx, spt, oracle, golden_scenes):
    L = spt._native.lib()
    h = ctx.handle
    W, H = 33, 18
    npix = W * H
    prev, cur = pair(oracle, golden_scenes, W, H, 2)
    motion = table(golden_scenes)
    n = len(motion)
    keep = [np.ascontiguousarray(a) for a in (cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"],
                                              prev["rgba"], prev["mom"], prev["feat"], prev["ids"], prev["view"], prev["eye"])]
    # one buffer, so that an output can end in the table's first bytes or begin in its last
    buf = np.zeros(npix * 4 + n * 8 + npix * 4, F)
    buf[npix * 4:npix * 4 + n * 8] = motion.reshape(-1)
    tab = buf[npix * 4:npix * 4 + n * 8]
    out, out_mom = np.full((H, W, 4), -3.0, F), np.full((H, W, 4), -4.0, F)
    ptrs = [a.ctypes.data_as(P) for a in keep]
    op, mp, tp = out.ctypes.data_as(P), out_mom.ctypes.data_as(P), tab.ctypes.data_as(P)

    def call(fn, o=op, m=mp, t=tp, count=n, **repl):
        a = [repl.get(k, p) for k, p in zip(("rgba", "mom", "feat", "ids"), ptrs[:4])] + ptrs[4:]
        if fn == "async":
            return L.spt_temporal_motion_async(h, W, H, *a, t, count, 0.25, 0.1, 64.0, o, m, None)
        return L.spt_temporal_motion(h, W, H, *a, t, count, 0.25, 0.1, 64.0, o, m)

    for fn in ("blocking", "async"):
        assert call(fn, t=None) == 1 and b"motion" in L.spt_last_error(h)
        assert call(fn, t=None, count=1) == 1 and b"motion" in L.spt_last_error(h)
        assert call(fn, o=tp) == 1 and b"out_rgba overlaps motion" in L.spt_last_error(h)
        assert call(fn, m=tp) == 1 and b"out_mom overlaps motion" in L.spt_last_error(h)
        assert call(fn, o=P(tab.ctypes.data + n * 32 - 4)) == 1 and b"out_rgba overlaps motion" in L.spt_last_error(h)
        assert call(fn, m=P(tab.ctypes.data - npix * 16 + 4)) == 1 and b"out_mom overlaps motion" in L.spt_last_error(h)
        # the existing pair's errors are kept
        assert call(fn, rgba=None) == 1 and b"null" in L.spt_last_error(h)
        assert call(fn, o=None) == 1 and b"null" in L.spt_last_error(h)
        assert call(fn, o=ptrs[0]) == 1 and b"out_rgba overlaps rgba" in L.spt_last_error(h)
    assert (out == -3.0).all() and (out_mom == -4.0).all()
    # an output that ends where the table begins is no overlap; n_spheres == 0 reads no table, wherever it points
    exp = want(spt, cur, prev, motion, **DEFAULTS)
    assert exp[2]["mv"].any() and (exp[2]["mv"] & exp[2]["has"]).any()
    assert call("blocking", m=P(tab.ctypes.data - npix * 16)) == 0, L.spt_last_error(h)
    same(out, exp[0], "33x18 after the errors: out_rgba")
    same(buf[:npix * 4].reshape(H, W, 4), exp[1], "33x18 after the errors: out_mom, ending at the table")
    assert np.array_equal(bits(tab), bits(motion.reshape(-1)))
    assert call("blocking", t=op, count=0) == 0, L.spt_last_error(h)
    same(out, want_plain(spt, cur, prev, **DEFAULTS)[0], "n_spheres == 0 with a table pointer that is not read")


# ---------------------------------------------------------------- 9: the accumulator

def gpu_frame(c, spt, golden_scenes, which, cam, W, H, spp, seed):
    view, eye = camera(golden_scenes, cam)
    c.set_scene(spt.Scene(*scene_of(golden_scenes, which)))
    c.set_camera(view, eye, SKY)
    c.set_params(W, H, spp, DEPTH, seed)
    rgba, mom = c.render_moments(0, H, 0, W)
    feat, ids = c.render_features(0, H, 0, W, ids=True)
    return dict(rgba=rgba.reshape(H, W, 4), mom=mom.reshape(H, W, 4), feat=feat.reshape(H, W, 2, 4), ids=ids.reshape(H, W),
                view=view, eye=eye)


CHAIN = (("A", 0), ("B", 1), ("A", 2))  # (scene, camera) of frames 0, 1, 2: A -> B -> A'


def test_three_frames_through_the_accumulator_and_resident_against_not(spt, golden_scenes):
    W, H, spp = 96, 64, 3
    c = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        scenes = {k: spt.Scene(*scene_of(golden_scenes, k)) for k in "AB"}
        frames = [gpu_frame(c, spt, golden_scenes, which, cam, W, H, spp, SEED + k) for k, (which, cam) in enumerate(CHAIN)]
        # the chain by hand, each step against the helper
        by_hand, hist = [frames[0]["rgba"]], frames[0]
        for k in (1, 2):
            motion = spt.sphere_motion(scenes[CHAIN[k][0]], scenes[CHAIN[k - 1][0]])
            exp = want(spt, frames[k], hist, motion, tol_normal=0.25, tol_depth=0.1, max_history=16.0)
            assert (exp[2]["mv"] & exp[2]["has"]).sum() >= 300, k
            assert (moved(exp, want_plain(spt, frames[k], hist, tol_normal=0.25, tol_depth=0.1, max_history=16.0)) & exp[2]["mv"]).sum() >= 300
            out, out_mom = check(c, frames[k], hist, motion, exp, f"frame {k} by hand", max_history=16.0)
            by_hand.append(out)
            hist = dict(frames[k], rgba=out, mom=out_mom)
        accs = {res: spt.TemporalAccumulator(c, W, H, spp, DEPTH, seed=SEED, sky=SKY, max_history=16.0, resident=res)
                for res in (False, True)}
        for res, acc in accs.items():
            for k, (which, cam) in enumerate(CHAIN):
                img = acc.frame(*camera(golden_scenes, cam), scene=scenes[which])
                assert img.shape == (H, W, 4) and img.dtype == np.float32
                same(img, by_hand[k], f"accumulator (resident={res}) frame {k}")
            assert acc.frame_index == 3
        # a filtered frame, then one without scene= (the spheres stand still): resident equals not, on bits
        den = [acc.frame(*camera(golden_scenes, 1), denoise={}, scene=scenes["B"]) for acc in accs.values()]
        assert np.isfinite(den[0]).all() and (bits(den[0]) != bits(by_hand[1])).any()
        same(den[1], den[0], "resident against non-resident, denoise={}")
        plain = [acc.frame(*camera(golden_scenes, 0)) for acc in accs.values()]
        same(plain[1], plain[0], "resident against non-resident, no scene=")
        # reset(): no history, and no previous scene to follow
        for res, acc in accs.items():
            acc.reset()
            c.set_scene(scenes["B"])
            first = acc.frame(*camera(golden_scenes, 0), scene=scenes["A"])
            same(first, frames[0]["rgba"], f"after reset (resident={res}) the first frame passes through")
        # a scene with another sphere count
        a = scenes["A"]
        fewer = spt.Scene(a.centers[:-1], a.radii[:-1], a.colors[:-1], a.materials[:-1], a.fuzz[:-1])
        for acc in accs.values():
            with pytest.raises(ValueError):
                acc.frame(*camera(golden_scenes, 1), scene=fewer)
            assert acc.frame_index == 1
    finally:
        c.close()


# ---------------------------------------------------------------- 10: non-interference

def test_a_motion_call_leaves_renders_and_stats_alone(spt, oracle, golden_scenes):
    W, H, spp = 64, 40, 4
    prev, cur = pair(oracle, golden_scenes, 33, 18, 2)
    motion = table(golden_scenes)
    exp = want(spt, cur, prev, motion, **DEFAULTS)
    c = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        before = c.render_segment(0, H, 0, W)
        c.synchronize()
        st0 = c.stats()
        check(c, cur, prev, motion, exp, "between two renders", **DEFAULTS)
        st1 = c.stats()
        assert {k: st0[k] for k in COUNTERS} == {k: st1[k] for k in COUNTERS}
        after = c.render_segment(0, H, 0, W)
        st2 = c.stats()
        assert np.array_equal(bits(before), bits(after))
        assert st2["samples"] - st1["samples"] == W * H * spp and st2["launches"] > st1["launches"]
    finally:
        c.close()
