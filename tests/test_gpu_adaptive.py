"""Adaptive sampling (spt_render_adaptive[_dev]) against its contract, bit for bit
(include/spt_hip.h "adaptive sampling").

What it must return comes from tests/adaptive.py (numpy) over the oracle's per-sample
colours, and from the property the contract rests on: a pixel that stopped after n samples is
that pixel of a plain render at spp = n.  The "oracle frame" is the golden `random` scene
through golden_scenes["view"] from the eye [0, 1, -3], seed 3, depth 8, at 45 x 37: 6 x 5
tiles, 5 ragged columns on the right and 5 ragged rows at the bottom.  No comparison has a
tolerance.

    1  the oracle frame: rgba, g_data, mom, info                     the numpy contract
    2  the same frame against plain renders at every n               s0 != 0 in batched launches
    3  base 3, step 5, max 11                                        a last pass shorter than step
    4  1x1, 7x5, 8x8, 9x17, 27x35 at tol 0, +inf, 0.1                ragged and single tiles
    5  tol = +inf is render_moments at base; max = base is one pass  degenerate stops
    6  a sub-rectangle off the tile grid                             regions, untouched bytes
    7  flat 4, flat 8, wave-walk tree, global and LDS lane walks     every batched render kernel
    8  NaN colours (degenerate scene)                                NaN passes through, converged
    9  the device form on a stream, a render right behind it
    10 a resident service around a call; a setter right after one
    11 spt_stats: samples and launches
    12 argument and state errors leave the outputs untouched
    13 render_denoised(variance=True, adaptive=...) by hand; render_denoised() unchanged
"""
import ctypes

import numpy as np
import pytest

import degenerate_scenes as D
from adaptive import expected_adaptive, pixel_counts
from denoise import expected_bytes
from test_gpu_cast import STRESS, STRESS_SEED, WALK_NODES, accel_nodes
from test_gpu_denoise import same
from test_gpu_features import DEPTH, SEED, make_ctx
from test_gpu_parity import EYE, LOOK, SKY, UP, bits, oscene_from, scene_from, setup

pytestmark = pytest.mark.gpu

W1, H1 = 45, 37
P1 = dict(base_spp=4, step_spp=4, max_spp=16, tol=0.15, lum_floor=1.0)
P3 = dict(base_spp=3, step_spp=5, max_spp=11, tol=0.1, lum_floor=1.0)
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
def ctx1(spt, golden_scenes):
    """The oracle frame's context.  Its own spp (1) is not what any call below renders."""
    c = make_ctx(spt, golden_scenes, W1, H1, 1)
    yield c
    c.close()


_oracle = {}


def oracle_samples(oracle, golden_scenes):
    """The oracle's per-sample colours of the oracle frame at 16 spp, (H, W, 16, 4)."""
    if not _oracle:
        osc = oscene_from(oracle, golden_scenes, "random")
        fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W1, H1, 16, DEPTH, SEED)
        _oracle["col"] = oracle.trace_region(osc, fr, 0, H1, 0, W1)[0].reshape(H1, W1, 16, 4)
    return _oracle["col"]


def want(oracle, golden_scenes, region, params):
    """expected_adaptive of a region (yB, yE, xB, xE) of the oracle frame."""
    key = (region, tuple(sorted(params.items())))
    if key not in _oracle:
        yB, yE, xB, xE = region
        col = np.ascontiguousarray(oracle_samples(oracle, golden_scenes)[yB:yE, xB:xE]).reshape(-1, 16, 4)
        _oracle[key] = expected_adaptive(col, xE - xB, yE - yB, params["base_spp"], params["step_spp"], params["max_spp"],
                                         params["tol"], params["lum_floor"])
    return _oracle[key]


def same4(got, exp, what, nan=False):
    same(np.ascontiguousarray(got).reshape(-1, 1, 4), np.ascontiguousarray(exp).reshape(-1, 1, 4), what, nan=nan)


def region_bytes(g, W, H, region):
    """The g_data bytes of the region's pixels, (pixels, 3) in local row-major order."""
    yB, yE, xB, xE = region
    return g.reshape(H, W, 3)[H - 1 - np.arange(yB, yE)][:, xB:xE].reshape(-1, 3)


def passes_of(n_max, p):
    return 1 + -(-(n_max - p["base_spp"]) // p["step_spp"])


def check_against_plain(c, W, H, region, p, what, depth=DEPTH, seed=SEED):
    """One adaptive call of the region, checked against the context's own plain renders:
    tiles share one n from the contract's ladder, info adds up, and the pixels with each n are
    render_moments at spp = n in rgba, g_data bytes and mom, on bits.  Returns the n per pixel."""
    yB, yE, xB, xE = region
    w, h = xE - xB, yE - yB
    g = np.full(W * H * 3, 0xAB, np.uint8)
    rgba, mom, info = c.render_adaptive(*region, g_data=g, **p)
    n_pix = mom[:, 3].astype(np.int64)
    assert np.array_equal(mom[:, 3], n_pix.astype(np.float32)) and (rgba[:, 3] == 0).all(), what
    ladder = sorted(set(list(range(p["base_spp"], p["max_spp"], p["step_spp"])) + [p["max_spp"]]))
    assert set(np.unique(n_pix)) <= set(ladder), (what, np.unique(n_pix))
    n_img = n_pix.reshape(h, w)
    for ty in range(0, h, 8):
        for tx in range(0, w, 8):
            assert len(np.unique(n_img[ty:ty + 8, tx:tx + 8])) == 1, f"{what}: tile at ({tx}, {ty}) has several n"
    assert info["samples"] == int(n_pix.sum()) and info["passes"] == passes_of(int(n_pix.max()), p), (what, info)
    outside = np.ones((H, W), bool)
    outside[H - yE:H - yB, xB:xE] = False
    assert (g.reshape(H, W, 3)[outside] == 0xAB).all(), f"{what}: bytes outside the region"
    got8 = region_bytes(g, W, H, region)
    for n in np.unique(n_pix):
        c.set_params(W, H, int(n), depth, seed)
        g2 = np.full(W * H * 3, 0xAB, np.uint8)
        plain, pmom = c.render_moments(*region, g_data=g2)
        at = n_pix == n
        same4(rgba[at], plain[at], f"{what}: rgba of the pixels at n = {n}", nan=True)
        same4(mom[at], pmom[at], f"{what}: mom of the pixels at n = {n}", nan=True)
        assert np.array_equal(got8[at], region_bytes(g2, W, H, region)[at]), f"{what}: bytes of the pixels at n = {n}"
    return n_pix


# ---------------------------------------------------------------- 2: against plain renders (the first to run)

def test_oracle_frame_against_plain_renders(ctx1):
    n_pix = check_against_plain(ctx1, W1, H1, (0, H1, 0, W1), P1, "45x37")
    assert sorted(np.unique(n_pix)) == [4, 8, 12, 16], np.unique(n_pix)


# ---------------------------------------------------------------- 1: the oracle frame

def test_oracle_frame_against_the_contract(ctx1, oracle, golden_scenes):
    region = (0, H1, 0, W1)
    rgba_e, mom_e, n_map, active = want(oracle, golden_scenes, region, P1)
    print(f"adaptive 45x37, {P1}: active tiles per pass {active}, n map\n{n_map}")
    # the CPU restatement's figures: the case cannot degenerate silently
    assert active == [30, 18, 17, 14] and sorted(np.unique(n_map)) == [4, 8, 12, 16]
    assert n_map[1:4, -1].tolist() == [16, 16, 4] and set(n_map[-1].tolist()) == {4, 12}  # the ragged column and row
    g = np.full(W1 * H1 * 3, 0xAB, np.uint8)
    rgba, mom, info = ctx1.render_adaptive(*region, g_data=g, **P1)
    same4(mom, mom_e, "mom against the oracle's samples")
    same4(rgba, rgba_e, "rgba against the oracle's samples")
    assert np.array_equal(g, expected_bytes(oracle, rgba_e.reshape(H1, W1, 4), W1, H1)), "g_data against the oracle"
    assert info == {"samples": int(pixel_counts(n_map, W1, H1).sum()), "passes": len(active)}


# ---------------------------------------------------------------- 3: pass sizes

def test_a_last_pass_shorter_than_the_step(ctx1, oracle, golden_scenes):
    region = (0, H1, 0, W1)
    rgba_e, mom_e, n_map, active = want(oracle, golden_scenes, region, P3)
    assert active == [30, 19, 17] and sorted(np.unique(n_map)) == [3, 8, 11], (active, np.unique(n_map))
    rgba, mom, info = ctx1.render_adaptive(*region, **P3)
    same4(mom, mom_e, "mom at base 3, step 5, max 11")
    same4(rgba, rgba_e, "rgba at base 3, step 5, max 11")
    assert info == {"samples": int(pixel_counts(n_map, W1, H1).sum()), "passes": 3}
    check_against_plain(ctx1, W1, H1, region, P3, "45x37 at 3/5/11")


# ---------------------------------------------------------------- 4: small shapes

@pytest.mark.parametrize("frame", [(1, 1), (7, 5), (8, 8), (9, 17), (27, 35)], ids=lambda f: f"{f[0]}x{f[1]}")
def test_small_and_ragged_frames(spt, golden_scenes, frame):
    W, H = frame
    c = make_ctx(spt, golden_scenes, W, H, 1)
    try:
        seen = set()
        for tol in (0.0, INF, 0.1):
            n_pix = check_against_plain(c, W, H, (0, H, 0, W), dict(P1, tol=tol), f"{W}x{H} at tol {tol}")
            if tol == INF:
                assert (n_pix == 4).all()
            if tol == 0.0:
                assert set(np.unique(n_pix)) <= {4, 16}
            seen |= set(np.unique(n_pix).tolist())
        assert W * H == 1 or len(seen) >= 2, seen
    finally:
        c.close()


# ---------------------------------------------------------------- 5: degenerate stops

def test_degenerate_stops(ctx1):
    region = (0, H1, 0, W1)
    g = np.full(W1 * H1 * 3, 0xAB, np.uint8)
    rgba, mom, info = ctx1.render_adaptive(*region, g_data=g, **dict(P1, tol=INF))
    ctx1.set_params(W1, H1, 4, DEPTH, SEED)
    g2 = np.full(W1 * H1 * 3, 0xAB, np.uint8)
    plain, pmom = ctx1.render_moments(*region, g_data=g2)
    same4(rgba, plain, "tol = +inf: rgba")
    same4(mom, pmom, "tol = +inf: mom")
    assert np.array_equal(g, g2) and info == {"samples": W1 * H1 * 4, "passes": 1}
    assert (pmom[:, 2] > 0).any(), "the frame has noisy pixels to stop"
    # max_spp = base_spp: one pass, whatever the tolerance
    rgba, mom, info = ctx1.render_adaptive(*region, **dict(P1, max_spp=4, tol=0.0))
    same4(rgba, plain, "max = base: rgba")
    same4(mom, pmom, "max = base: mom")
    assert info == {"samples": W1 * H1 * 4, "passes": 1}


# ---------------------------------------------------------------- 6: a sub-rectangle

def test_a_sub_rectangle_off_the_tile_grid(ctx1, oracle, golden_scenes):
    region = (3, 29, 5, 40)
    rgba_e, mom_e, n_map, active = want(oracle, golden_scenes, region, P1)
    assert len(np.unique(n_map)) >= 3 and active[0] == 4 * 5
    rgba, mom, info = ctx1.render_adaptive(*region, **P1)
    same4(mom, mom_e, "mom of region y 3..29, x 5..40")
    same4(rgba, rgba_e, "rgba of region y 3..29, x 5..40")
    assert info["passes"] == len(active)
    check_against_plain(ctx1, W1, H1, region, P1, "region y 3..29, x 5..40")  # the sentinel bytes too


# ---------------------------------------------------------------- 7: traversal shapes

WALKS = {"flat4": (4, 0), "flat8": (8, 0), "wave": (8, 2), "global": None, "lds": None}


@pytest.mark.parametrize("walk", list(WALKS))
def test_every_batched_traversal_shape(spt, golden_scenes, walk):
    W, H = 27, 35
    if WALKS[walk] is not None:
        c = make_ctx(spt, golden_scenes, W, H, 1, shape=WALKS[walk])
    else:
        s = spt.generate_stress(STRESS_SEED, STRESS[walk])
        lo, hi = WALK_NODES[walk]
        assert lo <= accel_nodes(spt, s, D.AUTO, D.AUTO) <= hi
        c = spt.Context(0)
        setup(c, s, W, H, 1, DEPTH, seed=SEED)
    try:
        n_pix = check_against_plain(c, W, H, (0, H, 0, W), P1, walk)
        assert len(np.unique(n_pix)) >= 2, np.unique(n_pix)
    finally:
        c.close()


# ---------------------------------------------------------------- 8: NaN colours

def test_nan_pixels_pass_through_and_count_as_converged(spt, oracle):
    v = D.by_id("nonfinite/colours")
    W, H, _, depth, seed = v.frame
    p = dict(base_spp=2, step_spp=2, max_spp=6, tol=0.05, lum_floor=1.0)
    view = spt.camera_basis(v.eye, v.look, D.UP)
    osc = oracle.OracleScene(*v.arrays)
    fr = oracle.make_frame(view, v.eye, v.sky, W, H, p["max_spp"], depth, seed)
    col = oracle.trace_region(osc, fr, 0, H, 0, W)[0]
    rgba_e, mom_e, n_map, active = expected_adaptive(col, W, H, p["base_spp"], p["step_spp"], p["max_spp"], p["tol"], p["lum_floor"])
    nan = np.isnan(mom_e[:, :3]).any(axis=1)
    n_pix = pixel_counts(n_map, W, H)
    print(f"{v.id}: {int(nan.sum())} of {len(nan)} pixels NaN, active tiles per pass {active}, "
          f"NaN pixels in tiles that stopped early: {int((nan & (n_pix < p['max_spp'])).sum())}")
    assert nan.any() and not nan.all()
    assert (nan & (n_pix < p["max_spp"])).any(), "a NaN pixel sits in a tile that stopped early: it kept no tile alive"
    c = spt.Context(0)
    try:
        c.set_scene(spt.Scene(*v.arrays))
        c.set_camera(view, v.eye, v.sky)
        c.set_params(W, H, 1, depth, seed)
        rgba, mom, info = c.render_adaptive(0, H, 0, W, **p)
        same4(mom, mom_e, v.id + ": mom", nan=True)
        same4(rgba, rgba_e, v.id + ": rgba", nan=True)
        assert info == {"samples": int(n_pix.sum()), "passes": len(active)}
    finally:
        c.close()


# ---------------------------------------------------------------- 9: the device form

def test_device_form_on_a_stream_with_a_render_behind(spt, ctx1, oracle, golden_scenes):
    import torch
    region = (0, H1, 0, W1)
    rgba_e, mom_e, n_map, active = want(oracle, golden_scenes, region, P1)
    ctx1.set_params(W1, H1, 4, DEPTH, SEED)
    plain4 = ctx1.render_segment(*region)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    n = W1 * H1
    t_rgba = torch.full((n, 4), -1.0, dtype=torch.float32, device=dev)
    t_mom = torch.full((n, 4), -2.0, dtype=torch.float32, device=dev)
    t_g = torch.full((n * 3,), 0xAB, dtype=torch.uint8, device=dev)
    t_next = torch.full((n, 4), -3.0, dtype=torch.float32, device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    info = ctx1.render_adaptive_dev(*region, rgba=t_rgba, rgb8=t_g, mom=t_mom, stream=stream.cuda_stream, **P1)
    # at once, on the same stream: the next render rewrites the workspace's sample words
    ctx1.render_rows_async(spt._native.MODE_SEGMENT, 0, H1, 1, 1, 0, 0, W1, t_next.data_ptr(), 0, stream.cuda_stream)
    stream.synchronize()
    ctx1.synchronize()
    same4(t_mom.cpu().numpy(), mom_e, "device form: mom")
    same4(t_rgba.cpu().numpy(), rgba_e, "device form: rgba")
    assert np.array_equal(t_g.cpu().numpy(), expected_bytes(oracle, rgba_e.reshape(H1, W1, 4), W1, H1))
    assert info == {"samples": int(pixel_counts(n_map, W1, H1).sum()), "passes": len(active)}
    same4(t_next.cpu().numpy(), plain4, "the render behind it")
    # mom alone, on the default stream
    t_mom2 = torch.full((n, 4), -2.0, dtype=torch.float32, device=dev)
    ctx1.render_adaptive_dev(*region, mom=t_mom2, **P1)
    torch.cuda.synchronize(dev)
    same4(t_mom2.cpu().numpy(), mom_e, "device form: mom alone")


# ---------------------------------------------------------------- 10: the service, a setter behind a call

def test_between_service_renders_and_with_a_setter_behind(spt, golden_scenes):
    import torch
    W, H = 64, 40
    c = make_ctx(spt, golden_scenes, W, H, 4)
    try:
        region = (0, H, 0, W)
        rgba_e, mom_e, info_e = c.render_adaptive(*region, **P1)
        assert len(np.unique(mom_e[:, 3])) >= 3
        c.service_start()
        before = c.render_segment(*region)
        assert c.stats()["svc_running"] == 1
        rgba, mom, info = c.render_adaptive(*region, **P1)
        after = c.render_segment(*region)
        assert c.stats()["svc_running"] == 1
        c.service_stop()
        same4(before, after, "the service's renders around the call")
        same4(rgba, rgba_e, "between two service renders: rgba")
        same4(mom, mom_e, "between two service renders: mom")
        assert info == info_e
        # a setter right behind the device form waits for the passes in flight
        dev = torch.device("cuda", 0)
        t_rgba = torch.full((W * H, 4), -1.0, dtype=torch.float32, device=dev)
        t_mom = torch.full((W * H, 4), -2.0, dtype=torch.float32, device=dev)
        c.render_adaptive_dev(*region, rgba=t_rgba, mom=t_mom, **P1)
        c.set_camera(spt.camera_basis([2, 1, -3, 0], LOOK, UP), [2, 1, -3, 0], SKY)
        torch.cuda.synchronize(dev)
        same4(t_rgba.cpu().numpy(), rgba_e, "a setter behind the call: rgba")
        same4(t_mom.cpu().numpy(), mom_e, "a setter behind the call: mom")
        moved, _, _ = c.render_adaptive(*region, **P1)
        assert (bits(moved) != bits(rgba_e)).any(), "the new camera is live"
    finally:
        c.close()


# ---------------------------------------------------------------- 11: stats

def test_stats_count_the_passes_as_renders(ctx1):
    ctx1.synchronize()
    st0 = ctx1.stats()
    _, mom, info = ctx1.render_adaptive(0, H1, 0, W1, **P1)
    st1 = ctx1.stats()
    assert info["passes"] == 4
    assert st1["samples"] - st0["samples"] == int(mom[:, 3].sum()) == info["samples"]
    assert st1["launches"] - st0["launches"] == info["passes"]
    assert st1["casts"] > st0["casts"]


# ---------------------------------------------------------------- 12: errors

def test_state_and_argument_errors_leave_the_outputs_untouched(spt, golden_scenes):
    L = spt._native.lib()
    c = spt.Context(0)
    try:
        h = c.handle
        W, H = 32, 16
        n = 8 * 4
        rgba = np.full((n, 4), -3.0, np.float32)
        mom = np.full((n, 4), -4.0, np.float32)
        g = np.full(W * H * 3, 0xAB, np.uint8)
        info = np.array([7, 9], np.uint64)
        rp, mp, gp, ip = (a.ctypes.data_as(P) for a in (rgba, mom, g, info))
        good = dict(base=2, step=2, mx=4, tol=0.1, floor=1.0)

        def blocking(yB, yE, xB, xE, r=rp, b=gp, m=mp, **kw):
            k = dict(good, **kw)
            return L.spt_render_adaptive(h, yB, yE, xB, xE, k["base"], k["step"], k["mx"], k["tol"], k["floor"], r, b, m, ip)

        def device(yB, yE, xB, xE, r=rp, b=gp, m=mp, **kw):
            # (host pointers: every call below fails, or does nothing, before it would touch them)
            k = dict(good, **kw)
            return L.spt_render_adaptive_dev(h, yB, yE, xB, xE, k["base"], k["step"], k["mx"], k["tol"], k["floor"], r, b, m,
                                             ip, None)

        for call in (blocking, device):
            assert call(0, 4, 0, 8) == 2 and b"scene" in L.spt_last_error(h)
        c.set_scene(scene_from(spt, golden_scenes, "random"))
        for call in (blocking, device):
            assert call(0, 4, 0, 8) == 2 and b"camera" in L.spt_last_error(h)
        c.set_camera(golden_scenes["view"], EYE, SKY)
        for call in (blocking, device):
            assert call(0, 4, 0, 8) == 2 and b"params" in L.spt_last_error(h)
        c.set_params(W, H, 1, 4, 1)
        nan = float("nan")
        for call in (blocking, device):
            for bad in ((0, 17, 0, 8), (0, 4, 0, 33), (4, 3, 0, 8), (0, 4, 8, 7), (0, 0xFFFFFFFF, 0, 8)):
                assert call(*bad) == 1, bad
            for kw in (dict(base=0), dict(step=0), dict(mx=1), dict(base=5), dict(tol=-0.5), dict(tol=nan), dict(tol=-INF),
                       dict(floor=-1.0), dict(floor=nan), dict(floor=INF)):
                assert call(0, 4, 0, 8, **kw) == 1, kw
            assert call(0, 4, 0, 8, r=None, b=None, m=None) == 1 and b"null" in L.spt_last_error(h)
        # a pass over one sample batch: 32 pixels x 2 samples x 4 B = 256 B of words
        c.synchronize()
        launches = c.stats()["launches"]
        c.set_workspace(128)
        for call in (blocking, device):
            assert call(0, 4, 0, 8) == 1 and b"workspace" in L.spt_last_error(h)
        # ... and so is a later pass that could be longer than the first
        c.set_workspace(256)
        assert blocking(0, 4, 0, 8, step=3, mx=8) == 1 and b"workspace" in L.spt_last_error(h)
        assert c.stats()["launches"] == launches, "nothing was rendered"
        # an empty rectangle is SPT_OK and touches nothing, whatever the pointers
        for call in (blocking, device):
            for empty in ((3, 3, 0, 8), (0, 4, 5, 5), (16, 16, 32, 32)):
                assert call(*empty) == 0 and call(*empty, r=None, b=None, m=None) == 0, empty
        assert (rgba == -3.0).all() and (mom == -4.0).all() and (g == 0xAB).all() and info.tolist() == [7, 9]
        # and the same buffers are filled by a valid call once the pass fits
        assert blocking(12, 16, 24, 32) == 0, L.spt_last_error(h)
        assert (rgba[:, :3] != -3.0).all() and (mom != -4.0).all() and set(mom[:, 3].tolist()) <= {2.0, 4.0}
        assert (g != 0xAB).any() and info[0] == mom[:, 3].sum() and 1 <= info[1] <= 2
        assert c.stats()["launches"] == launches + int(info[1])
        # mom may be null when another output is given
        assert blocking(12, 16, 24, 32, m=None) == 0 and blocking(12, 16, 24, 32, r=None, b=None) == 0
    finally:
        c.close()


# ---------------------------------------------------------------- 13: the Python interface end to end

def test_render_denoised_with_adaptive_sampling(spt, golden_scenes):
    W, H, spp = 96, 64, 4
    c = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        plain = c.render_denoised()
        var = c.render_denoised(variance=True)
        rgba, mom, info = c.render_adaptive(0, H, 0, W, **P1)
        assert len(np.unique(mom[:, 3])) >= 3
        by_hand = c.denoise_variance(rgba.reshape(H, W, 4), c.feature_buffers(), mom)
        got = c.render_denoised(variance=True, adaptive=P1)
        same(got, by_hand, "render_denoised(variance=True, adaptive=...)")
        assert (bits(got) != bits(var)).any(), "the adaptive frame is another image"
        by_hand2 = c.denoise_variance(rgba.reshape(H, W, 4), c.feature_buffers(), mom, sigma_color=2.0, levels=2)
        same(c.render_denoised(variance=True, adaptive=P1, sigma_color=2.0, levels=2), by_hand2, "with the filter's keywords")
        with pytest.raises(ValueError):
            c.render_denoised(adaptive=P1)
        # without the keyword: exactly as before
        same(c.render_denoised(), plain, "render_denoised()")
        same(c.render_denoised(variance=True), var, "render_denoised(variance=True)")
        same(plain, c.denoise(c.render_frame().reshape(H, W, 4), c.feature_buffers()), "render_denoised() by hand")
        rm, mm = c.render_moments(0, H, 0, W)
        same(var, c.denoise_variance(rm.reshape(H, W, 4), c.feature_buffers(), mm), "render_denoised(variance=True) by hand")
    finally:
        c.close()
