"""Temporal accumulation (spt_temporal[_async]) against its definition, bit for bit: the last
frame's colour and moments reprojected into this frame and blended with it (include/spt_hip.h
"temporal accumulation").

What the call must return comes from tests/temporal.py (numpy), with Minv from
spt_temporal_inverse.  The frames are tests/test_temporal_helper.py's: the golden `random`
scene seen by camera 1 (golden_scenes["view"], eye [0, 1, -3]), camera 2 (yawed 2 degrees,
eye [0.15, 1.05, -2.9]) and camera 3 (4 degrees, [0.3, 1.1, -2.8]), frame k of a sequence with
seed 3 + k, depth 8, rendered by the oracle.  Every test asserts on the helper's answer that
its case is live before it compares anything; no comparison has a tolerance.

    1  the oracle pair at 45 x 37 x 7, the defaults                  every rule rejects, sky history
    2  a chain A -> B -> C on the GPU's own outputs, max_history 10  the cap, fractional counts
    3  the same camera twice; prev_eye one ulp off                   the static rule and the path beside it
    4  1x1, 1x40, 40x1, 31x9, 33x18, 300x200 at 2 spp                ragged tiles, many blocks, x0 = y0 = -1
    5  tol_normal, tol_depth +inf, both; all ids equal               every test of a tap
    6  a previous camera facing the other way                        q.z <= 0: the image passes through
    7  non-finite pixels, bad history taps, zero sample counts       pass through, renormalised neighbours
    8  no history                                                    copies
    9  device pointers on two caller streams                         the async form
    10 the GPU's own frames through Context.temporal; TemporalAccumulator
    11 a render, a temporal call, the same render (launched / service)
    12 argument errors; the empty image
"""
import ctypes

import numpy as np
import pytest

from temporal import DEFAULTS, expected_temporal
from test_gpu_cast import COUNTERS
from test_gpu_denoise import changed, same
from test_gpu_features import DEPTH, SEED, make_ctx
from test_gpu_parity import SKY, bits
from test_temporal_helper import camera, oracle_frame, oracle_pair

pytestmark = pytest.mark.gpu

F = np.float32
W1, H1, S1 = 45, 37, 7
INF = float("inf")
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


def history_of(f):
    return (f["rgba"], f["mom"], f["feat"], f["ids"])


def want(spt, cur, prev, **kw):
    """The helper's answer for frame `cur` against the history frame `prev` (None: none)."""
    H, W = cur["ids"].shape
    if prev is None:
        return expected_temporal(cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"], W, H, **kw)
    return expected_temporal(cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"], W, H,
                             history_of(prev), prev["view"], prev["eye"], spt.temporal_inverse(prev["view"]), **kw)


def got(ctx, cur, prev, **kw):
    if prev is None:
        return ctx.temporal(cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"], **kw)
    return ctx.temporal(cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"], history_of(prev),
                        prev["view"], prev["eye"], **kw)


def check(ctx, spt, cur, prev, what, exp=None, nan=False, **kw):
    """The device's answer against the helper's (or `exp`, already computed) on bits; returns the device's."""
    exp = exp or want(spt, cur, prev, **kw)
    out, out_mom = got(ctx, cur, prev, **kw)
    same(out, exp[0], f"{what}: out_rgba", nan=nan)
    same(out_mom, exp[1], f"{what}: out_mom", nan=nan)
    return out, out_mom


def moved(a, b):
    """Pixels at which two (out_rgba, out_mom) answers differ on bits."""
    return (bits(a[0]) != bits(b[0])).any(axis=2) | (bits(a[1]) != bits(b[1])).any(axis=2)


# ---------------------------------------------------------------- 1: the oracle pair

def test_the_oracle_pair_with_the_defaults(ctx, spt, oracle, golden_scenes):
    prev, cur = oracle_pair(oracle, golden_scenes, W1, H1, S1)
    exp = want(spt, cur, prev, **DEFAULTS)
    info = exp[2]
    print(f"temporal 45x37x7: history in {info['history']:.3f}, taken {info['taken']}, rejected alone {info['alone']}")
    assert 0.5 <= info["history"] < 1.0 and all(n >= 1 for n in info["alone"].values()), info["alone"]
    assert (info["has"] & ~(cur["feat"][:, :, 0, 3] > 0)).any(), "sky history"
    assert changed(exp[0], cur["rgba"]).mean() > 0.5
    out, _ = check(ctx, spt, cur, prev, "45x37x7", exp=exp, **DEFAULTS)
    assert np.array_equal(bits(out[..., 3]), bits(cur["rgba"][..., 3])), "w passes through"
    # the defaults are the defaults
    o2, m2 = got(ctx, cur, prev)
    same(o2, exp[0], "keyword defaults")


# ---------------------------------------------------------------- 2: a chain on the GPU's own outputs

def test_a_chain_of_three_frames_with_the_cap_binding(ctx, spt, oracle, golden_scenes):
    a, b, c = (oracle_frame(oracle, golden_scenes, k, W1, H1, S1, SEED + k) for k in range(3))
    kw = dict(tol_normal=0.25, tol_depth=0.1, max_history=10.0)
    out_b, mom_b = check(ctx, spt, b, a, "A -> B", **kw)
    assert (mom_b[..., 3] == 2 * S1).any(), "7 + 7 samples: the cap does not bind on the first step"
    hist = dict(b, rgba=out_b, mom=mom_b)  # the GPU's own output is the history
    exp = want(spt, c, hist, **kw)
    n = exp[1][..., 3]
    capped, frac = int((n == 10.0 + S1).sum()), int((n != np.round(n)).sum())
    print(f"chain: {capped} pixels at the cap, {frac} with a fractional sample count, history in {exp[2]['history']:.3f}")
    assert capped >= 100 and frac >= 10 and exp[2]["history"] > 0.5
    assert moved(exp, want(spt, c, hist, tol_normal=0.25, tol_depth=0.1, max_history=64.0)).mean() > 0.25  # the cap is live
    check(ctx, spt, c, hist, "B -> C", exp=exp, **kw)


# ---------------------------------------------------------------- 3: the static rule

def test_the_static_rule_and_the_path_one_ulp_beside_it(ctx, spt, oracle, golden_scenes):
    prev, cur = oracle_pair(oracle, golden_scenes, W1, H1, S1, cams=(0, 0))
    exp = want(spt, cur, prev, **DEFAULTS)
    ys, xs = np.mgrid[0:H1, 0:W1]
    assert np.array_equal(exp[2]["fx"], xs.astype(F)) and np.array_equal(exp[2]["fy"], ys.astype(F))
    assert exp[2]["history"] > 0.8
    check(ctx, spt, cur, prev, "static", exp=exp, **DEFAULTS)
    eye = prev["eye"].copy()
    eye[2] = np.nextafter(eye[2], F(0))
    off = dict(prev, eye=eye)
    exp2 = want(spt, cur, off, **DEFAULTS)
    n = int(moved(exp, exp2).sum())
    print(f"static 45x37x7: prev_eye one ulp off moves {n} pixels")
    assert n >= 1 and not np.array_equal(exp2[2]["fx"], xs.astype(F))
    check(ctx, spt, cur, off, "one ulp off the static rule", exp=exp2, **DEFAULTS)


# ---------------------------------------------------------------- 4: shapes

# (W, H): the second camera's yaw in degrees and eye, chosen with the helper so that some pixel
# finds history, some finds none, and some finds it from x0 == -1 or y0 == -1, where only the
# inner taps lie inside the image (at 1 x 1 camera 2's pixel seeks history and finds none; a
# frame one pixel wide or high keeps only motions of less than a pixel across it)
SHAPES = {(1, 1): (2.0, [0.15, 1.05, -2.9, 0]), (1, 40): (-1.0, [0.02, 1.01, -2.99, 0]),
          (40, 1): (0.5, [-0.15, 0.95, -2.9, 0]), (31, 9): (2.0, [0.15, 1.05, -2.9, 0]),
          (33, 18): (-2.0, [-0.02, 0.99, -2.99, 0]), (300, 200): (-2.0, [-0.02, 0.99, -2.99, 0])}


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_ragged_and_large_shapes(ctx, spt, oracle, golden_scenes, shape):
    from temporal import yawed
    W, H = shape
    yaw, eye = SHAPES[shape]
    cam2 = (yawed(camera(golden_scenes, 0)[0], yaw), np.asarray(eye, F))
    prev, cur = oracle_pair(oracle, golden_scenes, W, H, 2, cams=(0, cam2))
    exp = want(spt, cur, prev, **DEFAULTS)
    info = exp[2]
    with np.errstate(all="ignore"):
        ex = info["sought"] & (np.floor(info["fx"]) == -1) & info["has"]
        ey = info["sought"] & (np.floor(info["fy"]) == -1) & info["has"]
    print(f"{W}x{H}x2: history in {info['history']:.3f}, {int(info['sought'].sum())} pixels seek it, {int(ex.sum())} find it "
          f"from x0 == -1, {int(ey.sum())} from y0 == -1")
    if W * H > 1:
        assert info["has"].any() and (~info["has"]).any()
        assert ex.any() or ey.any(), "only the inner taps inside"
    else:
        assert info["sought"].all()
    if W * H > 500:
        assert ex.any() and ey.any()
    check(ctx, spt, cur, prev, f"{W}x{H}x2", exp=exp, **DEFAULTS)


# ---------------------------------------------------------------- 5: every test of a tap

@pytest.mark.parametrize("ids_equal", [False, True], ids=["ids", "ids-equal"])
@pytest.mark.parametrize("off", ["normal", "depth", "both"])
def test_each_tolerance_switched_off(ctx, spt, oracle, golden_scenes, off, ids_equal):
    prev, cur = oracle_pair(oracle, golden_scenes, W1, H1, S1)
    if ids_equal:
        zero = np.zeros((H1, W1), np.uint32)
        prev, cur = dict(prev, ids=zero), dict(cur, ids=zero)
    kw = dict(tol_normal=INF if off in ("normal", "both") else 0.25, tol_depth=INF if off in ("depth", "both") else 0.1,
              max_history=64.0)
    exp = want(spt, cur, prev, **kw)
    base = want(spt, cur, prev, **DEFAULTS)
    assert moved(exp, base).sum() >= 1 and exp[2]["taken"] > base[2]["taken"], off  # the test was live
    if ids_equal:
        assert exp[2]["alone"]["ids"] == 0
    if off == "both":
        assert exp[2]["alone"]["normal"] == 0 and exp[2]["alone"]["depth"] == 0
    check(ctx, spt, cur, prev, f"tol {off} = inf", exp=exp, **kw)


# ---------------------------------------------------------------- 6: behind the previous camera

def test_a_previous_camera_facing_the_other_way(ctx, spt, oracle, golden_scenes):
    from temporal import yawed
    prev, cur = oracle_pair(oracle, golden_scenes, W1, H1, S1)
    back = dict(prev, view=yawed(prev["view"], 180.0))
    exp = want(spt, cur, back, tol_normal=INF, tol_depth=INF, max_history=64.0)
    assert not exp[2]["sought"].any() and exp[2]["history"] == 0.0
    out, out_mom = check(ctx, spt, cur, back, "facing away", exp=exp, tol_normal=INF, tol_depth=INF, max_history=64.0)
    assert np.array_equal(bits(out), bits(cur["rgba"])) and np.array_equal(bits(out_mom), bits(cur["mom"]))


# ---------------------------------------------------------------- 7: non-finite values and zero counts

def test_nonfinite_pixels_and_bad_history_taps(ctx, spt, oracle, golden_scenes):
    prev, cur = oracle_pair(oracle, golden_scenes, W1, H1, S1)
    clean = want(spt, cur, prev, **DEFAULTS)
    c = {k: (v.copy() if k in ("rgba", "mom", "feat") else v) for k, v in cur.items()}
    h = {k: (v.copy() if k in ("rgba", "mom", "feat") else v) for k, v in prev.items()}
    has = clean[2]["has"]
    ys, xs = np.nonzero(has[2:-2, 2:-2])
    at = [(int(y) + 2, int(x) + 2) for y, x in zip(ys[::len(ys) // 16], xs[::len(xs) // 16])][:14]
    assert len(at) == 14
    # current pixels (each had history in the clean answer)
    c["rgba"][at[0]][1] = np.nan
    c["rgba"][at[1]][0] = np.inf
    c["mom"][at[2]][0] = np.nan
    c["mom"][at[3]][2] = -np.inf
    c["mom"][at[4]][3] = np.inf
    c["feat"][at[5]][0, 1] = np.nan  # albedo: read by nothing else
    c["feat"][at[6]][1, 3] = np.inf  # depth
    c["mom"][at[7]][3] = 0.0
    c["mom"][at[8]][3] = -2.0
    cur_bad = at[:9]
    # history pixels
    h["rgba"][at[9]][2] = np.nan
    h["mom"][at[10]][1] = np.inf
    h["mom"][at[11]][3] = 0.0
    h["mom"][at[12]][3] = -1.0
    h["mom"][at[13]][3] = np.nan
    exp = want(spt, c, h, **DEFAULTS)
    for p in cur_bad:
        assert np.array_equal(bits(exp[0][p]), bits(c["rgba"][p])) and np.array_equal(bits(exp[1][p]), bits(c["mom"][p])), p
    # the bad history pixels were tapped: some neighbour's answer changes and stays finite
    ok = np.ones((H1, W1), bool)
    for p in cur_bad:
        ok[p] = False
    renorm = moved(exp, clean) & ok
    print(f"non-finite: {int(renorm.sum())} pixels renormalise around the bad history taps")
    assert renorm.sum() >= 3 and (renorm & exp[2]["has"]).sum() >= 3
    assert np.isfinite(exp[0][ok]).all() and np.isfinite(exp[1][ok]).all(), "nothing spreads"
    check(ctx, spt, c, h, "non-finite", exp=exp, nan=True, **DEFAULTS)


# ---------------------------------------------------------------- 8: no history

def test_without_a_history_the_outputs_are_copies(ctx, spt, oracle, golden_scenes):
    _, cur = oracle_pair(oracle, golden_scenes, W1, H1, S1)
    out, out_mom = check(ctx, spt, cur, None, "no history")
    assert np.array_equal(bits(out), bits(cur["rgba"])) and np.array_equal(bits(out_mom), bits(cur["mom"]))


# ---------------------------------------------------------------- 9: device pointers, two streams

def test_device_pointers_on_two_streams(ctx, spt, oracle, golden_scenes):
    import torch
    dev = torch.device("cuda", 0)
    a, b, c = (oracle_frame(oracle, golden_scenes, k, W1, H1, S1, SEED + k) for k in range(3))
    calls = []
    for cur, prev, kw in ((b, a, dict(DEFAULTS)), (c, b, dict(tol_normal=INF, tol_depth=0.05, max_history=3.0))):
        t = {k: torch.from_numpy(np.ascontiguousarray(cur[k])).to(dev) for k in ("rgba", "mom", "feat")}
        t["ids"] = torch.from_numpy(cur["ids"].astype(np.int32)).to(dev)
        th = {k: torch.from_numpy(np.ascontiguousarray(prev[k])).to(dev) for k in ("rgba", "mom", "feat")}
        th["ids"] = torch.from_numpy(prev["ids"].astype(np.int32)).to(dev)
        calls.append(dict(cur=cur, prev=prev, kw=kw, t=t, th=th, stream=torch.cuda.Stream(device=dev),
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
                           stream=k["stream"].cuda_stream, **k["kw"])
    for k in calls:
        k["stream"].synchronize()
    exps = [want(spt, k["cur"], k["prev"], **k["kw"]) for k in calls]
    assert moved(exps[1], want(spt, c, b, **DEFAULTS)).mean() > 0.25
    for k, exp in zip(calls, exps):
        same(k["out"].cpu().numpy(), exp[0], "async: out_rgba")
        same(k["mom"].cpu().numpy(), exp[1], "async: out_mom")
        for name in ("rgba", "mom", "feat"):
            assert np.array_equal(bits(k["t"][name].cpu().numpy()), bits(k["cur"][name])), name
            assert np.array_equal(bits(k["th"][name].cpu().numpy()), bits(k["prev"][name])), name


# ---------------------------------------------------------------- 10: the Python interface end to end

def gpu_frame(c, golden_scenes, cam, W, H, spp, seed):
    view, eye = camera(golden_scenes, cam)
    c.set_camera(view, eye, SKY)
    c.set_params(W, H, spp, DEPTH, seed)
    rgba, mom = c.render_moments(0, H, 0, W)
    feat, ids = c.render_features(0, H, 0, W, ids=True)
    return dict(rgba=rgba.reshape(H, W, 4), mom=mom.reshape(H, W, 4), feat=feat.reshape(H, W, 2, 4), ids=ids.reshape(H, W),
                view=view, eye=eye)


def test_the_gpus_own_frames_and_the_accumulator(spt, golden_scenes):
    W, H, spp = 96, 64, 3
    c = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        frames = [gpu_frame(c, golden_scenes, k, W, H, spp, SEED + k) for k in range(3)]
        exp = want(spt, frames[1], frames[0], **DEFAULTS)
        assert 0.5 <= exp[2]["history"] < 1.0 and all(n >= 1 for n in exp[2]["alone"].values())
        out, out_mom = check(c, spt, frames[1], frames[0], "the GPU's own frames", exp=exp, **DEFAULTS)
        # the same chain by hand and through the accumulator
        hist2 = dict(frames[1], rgba=out, mom=out_mom)
        by_hand = [(frames[0]["rgba"], frames[0]["mom"]), (out, out_mom), got(c, frames[2], hist2, max_history=16.0)]
        exp3 = want(spt, frames[2], hist2, tol_normal=0.25, tol_depth=0.1, max_history=16.0)
        same(by_hand[2][0], exp3[0], "third frame by hand")
        acc = spt.TemporalAccumulator(c, W, H, spp, DEPTH, seed=SEED, sky=SKY, max_history=16.0)
        for k in range(3):
            view, eye = camera(golden_scenes, k)
            img = acc.frame(view, eye)
            assert img.shape == (H, W, 4)
            same(img, by_hand[k][0], f"accumulator frame {k}")
        assert acc.frame_index == 3
        view, eye = camera(golden_scenes, 0)
        den = acc.frame(view, eye, denoise={})
        assert den.shape == (H, W, 4) and den.dtype == np.float32 and np.isfinite(den).all()
        acc.reset()
        same(acc.frame(*camera(golden_scenes, 0)), frames[0]["rgba"], "after reset the first frame passes through")
    finally:
        c.close()


# ---------------------------------------------------------------- 11: non-interference

@pytest.mark.parametrize("service", [False, True], ids=["launched", "service"])
def test_temporal_leaves_renders_and_stats_alone(spt, oracle, golden_scenes, service):
    W, H, spp = 64, 40, 4
    prev, cur = oracle_pair(oracle, golden_scenes, 33, 18, 2)
    exp = want(spt, cur, prev, **DEFAULTS)
    c = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        if service:
            c.service_start()
        before = c.render_segment(0, H, 0, W)
        if service:
            assert c.stats()["svc_running"] == 1
        else:
            c.synchronize()
        st0 = c.stats()
        check(c, spt, cur, prev, "between two renders", exp=exp, **DEFAULTS)
        st1 = c.stats()
        assert st1["svc_running"] == 0  # a resident session is ended by the call
        if not service:  # (a session's device counters arrive when it ends: the call ends it)
            assert {k: st0[k] for k in COUNTERS} == {k: st1[k] for k in COUNTERS}
        after = c.render_segment(0, H, 0, W)
        st2 = c.stats()
        assert np.array_equal(bits(before), bits(after))
        if service:  # the next render starts a new session
            assert st2["svc_running"] == 1 and st2["svc_sessions"] > st1["svc_sessions"]
            c.service_stop()
        else:
            assert st2["samples"] - st1["samples"] == W * H * spp and st2["launches"] > st1["launches"]
        check(c, spt, cur, prev, "after the renders", exp=exp, **DEFAULTS)
    finally:
        c.close()


# ---------------------------------------------------------------- 12: errors

def test_argument_errors_and_the_empty_image(ctx, spt, oracle, golden_scenes):
    L = spt._native.lib()
    h = ctx.handle
    W, H = 33, 18
    n = W * H
    prev, cur = oracle_pair(oracle, golden_scenes, W, H, 2)
    keep = [np.ascontiguousarray(a) for a in (cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"],
                                              prev["rgba"], prev["mom"], prev["feat"], prev["ids"], prev["view"], prev["eye"])]
    out, out_mom = np.full((H, W, 4), -3.0, F), np.full((H, W, 4), -4.0, F)
    ptrs = [a.ctypes.data_as(P) for a in keep]
    op, mp = out.ctypes.data_as(P), out_mom.ctypes.data_as(P)
    names = ("rgba", "mom", "feat", "ids", "view", "eye", "h_rgba", "h_mom", "h_feat", "h_ids", "pview", "peye")

    def call(fn, w=W, hh=H, tn=0.25, td=0.1, mh=64.0, o=op, m=mp, **repl):
        a = [repl.get(k, p) for k, p in zip(names, ptrs)]
        if fn == "async":
            return L.spt_temporal_async(h, w, hh, *a, tn, td, mh, o, m, None)
        return L.spt_temporal(h, w, hh, *a, tn, td, mh, o, m)

    singular = np.zeros(16, F)
    nanview = keep[10].copy()
    nanview[5] = np.nan
    for fn in ("blocking", "async"):
        for k in ("rgba", "mom", "feat", "ids", "view", "eye"):
            assert call(fn, **{k: None}) == 1 and b"null" in L.spt_last_error(h), k
        assert call(fn, o=None) == 1 and b"null" in L.spt_last_error(h)
        assert call(fn, m=None) == 1 and b"null" in L.spt_last_error(h)
        for k in ("h_rgba", "h_mom", "h_feat", "h_ids"):  # some but not all
            assert call(fn, **{k: None}) == 1 and b"history" in L.spt_last_error(h), k
            assert call(fn, **{j: None for j in ("h_rgba", "h_mom", "h_feat", "h_ids") if j != k}) == 1, k
        assert call(fn, pview=None) == 1 and call(fn, peye=None) == 1
        for bad in (float("nan"), -1.0, -INF):
            assert call(fn, tn=bad) == 1 and b"tol_normal" in L.spt_last_error(h), bad
            assert call(fn, td=bad) == 1 and b"tol_depth" in L.spt_last_error(h), bad
        for bad in (float("nan"), 0.0, -0.0, -1.0, -INF):
            assert call(fn, mh=bad) == 1 and b"max_history" in L.spt_last_error(h), bad
        assert call(fn, pview=singular.ctypes.data_as(P)) == 1 and b"prev_view" in L.spt_last_error(h)
        assert call(fn, pview=nanview.ctypes.data_as(P)) == 1 and b"prev_view" in L.spt_last_error(h)
        assert call(fn, w=65536, hh=32768) == 1  # 2^31 pixels
        # an output that overlaps an input, wholly or by its last bytes, or the other output
        for i, k in enumerate(("rgba", "mom", "feat", "ids", None, None, "h_rgba", "h_mom", "h_feat", "h_ids")):
            if k is None:
                continue
            size = keep[i].nbytes
            assert call(fn, o=ptrs[i]) == 1 and b"overlaps" in L.spt_last_error(h), k
            assert call(fn, m=P(keep[i].ctypes.data + size - 4)) == 1 and b"out_mom overlaps" in L.spt_last_error(h), k
        assert call(fn, m=P(out.ctypes.data + n * 16 - 4)) == 1 and b"out_rgba overlaps out_mom" in L.spt_last_error(h)
        # the empty image is SPT_OK and touches nothing
        assert call(fn, w=0) == 0 and call(fn, hh=0) == 0
    assert (out == -3.0).all() and (out_mom == -4.0).all()
    # tolerances of 0 and +inf and an uncapped history are valid, and the same buffers are then filled
    assert call("blocking", tn=0.0, td=0.0, mh=INF) == 0, L.spt_last_error(h)
    exp = want(spt, cur, prev, tol_normal=0.0, tol_depth=0.0, max_history=INF)
    same(out, exp[0], "33x18 after the errors: out_rgba")
    same(out_mom, exp[1], "33x18 after the errors: out_mom")
