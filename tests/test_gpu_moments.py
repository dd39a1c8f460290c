"""Sample moments (spt_render_moments[_async]) and the variance-guided filter
(spt_denoise_var[_async]) against their definitions, bit for bit (include/spt_hip.h "sample
moments" and "variance-guided denoiser").

What they must return comes from tests/moments.py (numpy).  The "oracle frame" is the golden
`random` scene through golden_scenes["view"] from the eye [0, 1, -3], seed 3, depth 8, at
45 x 37 x 7, with the oracle's per-sample colours (trace_region) and tests/features.py's
feature buffers.  Every test asserts on the helper's answer that its case is live before it
compares anything; no comparison has a tolerance.

    1  the oracle frame: mom, rgba, g_data; spt_stats                 the oracle's samples, the render it is
    2  1x1, 7x5, 8x8, 9x17, 27x35 at 1, 7, 8, 9, 17 spp               ragged tiles, the load run (8) +- 1
    3  a sub-rectangle off the tile grid                              regions
    4  the row map on a non-blocking stream, a render right behind    the async form, the workspace's reuse
    5  NaN colours (degenerate scene)                                 NaN moments by position
    6  a render, moments, the same render with the service resident   non-interference
    7  moments errors: over one batch, null mom, unset params
    8  the filter on the oracle frame, levels 1..5, with out_var      ragged tiles, the tap order
    9  1x1 .. 33x18 at levels 1 and 4; 300 x 200 at 8 levels           short lattices, many blocks
    10 each sigma +inf; var_floor 1e-6 and 1e6                        every term of the weight
    11 NaN, +inf, -inf in mom                                         pass through, never spread
    12 the g_data bytes, with and without the float output
    13 device pointers on two caller streams, a scratch each
    14 filter errors; the empty image
    15 render_denoised(variance=True) by hand; render_denoised() unchanged
"""
import ctypes

import numpy as np
import pytest

import degenerate_scenes as D
from denoise import DEFAULT_SIGMAS, expected_bytes, expected_denoise
from moments import DEFAULT_VAR_FLOOR, DEFAULT_VAR_SIGMAS, expected_denoise_var, expected_moments
from test_denoise_helper import _inputs, oracle_inputs
from test_gpu_denoise import changed, random_inputs, same
from test_gpu_features import DEPTH, SEED, make_ctx
from test_gpu_parity import EYE, SKY, bits

pytestmark = pytest.mark.gpu

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
    """A context without scene, camera or params: the filter needs none."""
    c = spt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx1(spt, golden_scenes):
    """The oracle frame's context."""
    c = make_ctx(spt, golden_scenes, W1, H1, S1)
    yield c
    c.close()


_oracle = {}


def oracle_frame(oracle, golden_scenes):
    """rgba (H, W, 4), feat (H, W, 2, 4), col (pixels, spp, 4), mom (pixels, 4) of the oracle frame."""
    if not _oracle:
        rgba, feat = oracle_inputs(oracle, golden_scenes, W1, H1, S1)
        osc = _inputs[(W1, H1, S1)][2]
        fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W1, H1, S1, DEPTH, SEED)
        col = oracle.trace_region(osc, fr, 0, H1, 0, W1)[0]
        g = np.zeros(W1 * H1 * 3, np.uint8)
        oracle.render_segment(osc, fr, 0, H1, 0, W1, rgb8=g)
        _oracle.update(rgba=rgba.reshape(H1, W1, 4), feat=feat.reshape(H1, W1, 2, 4), col=col, mom=expected_moments(col), g=g)
    return _oracle


def same_mom(got, exp, what, nan=False):
    same(np.ascontiguousarray(got).reshape(-1, 1, 4), np.ascontiguousarray(exp).reshape(-1, 1, 4), what, nan=nan)


# ---------------------------------------------------------------- 1: the oracle frame

def test_moments_of_the_oracle_frame(ctx1, oracle, golden_scenes):
    o = oracle_frame(oracle, golden_scenes)
    mom = o["mom"]
    rev = expected_moments(o["col"], reverse=True)
    zero, order = float((mom[:, 2] == 0).mean()), int((bits(rev[:, 1]) != bits(mom[:, 1])).sum())
    print(f"moments 45x37x7: variance == 0 in {zero:.3f} of the pixels, the sample order matters in {order}")
    assert 0.05 < zero < 0.95 and order >= 1 and np.isfinite(mom).all()
    ctx1.synchronize()
    st0 = ctx1.stats()
    g = np.full(W1 * H1 * 3, 0xAB, np.uint8)
    rgba, got = ctx1.render_moments(0, H1, 0, W1, g_data=g)
    st1 = ctx1.stats()
    same_mom(got, mom, "mom against the oracle's samples")
    assert np.array_equal(bits(rgba[:, :3]), bits(o["rgba"].reshape(-1, 4)[:, :3])), "rgba against the oracle"
    assert np.array_equal(g, o["g"]), "g_data against the oracle"
    # exactly what render_segment writes, w lane too
    g2 = np.full(W1 * H1 * 3, 0xAB, np.uint8)
    assert np.array_equal(bits(rgba), bits(ctx1.render_segment(0, H1, 0, W1, g_data=g2))) and np.array_equal(g, g2)
    # it counts as the render it is
    assert st1["samples"] - st0["samples"] == W1 * H1 * S1 and st1["launches"] == st0["launches"] + 1
    # mom alone
    none, got2 = ctx1.render_moments(0, H1, 0, W1, rgba=False)
    assert none is None
    same_mom(got2, mom, "mom alone")


# ---------------------------------------------------------------- 2: shapes and sample counts

@pytest.mark.parametrize("frame", [(1, 1), (7, 5), (8, 8), (9, 17), (27, 35)], ids=lambda f: f"{f[0]}x{f[1]}")
def test_moments_against_the_gpus_own_samples(spt, golden_scenes, frame):
    W, H = frame
    c = make_ctx(spt, golden_scenes, W, H, 1)
    try:
        live = 0
        for spp in (1, 7, 8, 9, 17):  # the kernel loads 8 words ahead: 8 - 1, 8, 8 + 1, 2 * 8 + 1
            c.set_params(W, H, spp, DEPTH, SEED)
            col = c.render_samples(0, H, 0, W, spp)
            exp = expected_moments(col)
            assert (exp[:, 3] == spp).all()
            if spp == 1:
                assert (exp[:, 2] == 0).all() or W * H == 1
            live += int((exp[:, 2] > 0).sum())
            rgba, mom = c.render_moments(0, H, 0, W)
            same_mom(mom, exp, f"{W}x{H}x{spp}")
            assert np.array_equal(bits(rgba), bits(c.render_segment(0, H, 0, W))), f"{W}x{H}x{spp}: rgba"
        assert live >= 1 or W * H == 1
    finally:
        c.close()


# ---------------------------------------------------------------- 3: a region off the tile grid

def test_moments_of_a_sub_rectangle(ctx1, oracle, golden_scenes):
    o = oracle_frame(oracle, golden_scenes)
    yB, yE, xB, xE = 3, 29, 5, 40
    exp = np.ascontiguousarray(o["mom"].reshape(H1, W1, 4)[yB:yE, xB:xE]).reshape(-1, 4)
    assert (exp[:, 2] > 0).any() and (exp[:, 2] == 0).any()
    g = np.full(W1 * H1 * 3, 0xAB, np.uint8)
    rgba, mom = ctx1.render_moments(yB, yE, xB, xE, g_data=g)
    same_mom(mom, exp, "region y 3..29, x 5..40")
    g2 = np.full(W1 * H1 * 3, 0xAB, np.uint8)
    assert np.array_equal(bits(rgba), bits(ctx1.render_segment(yB, yE, xB, xE, g_data=g2)))
    assert np.array_equal(g, g2) and (g == 0xAB).any() and (g != 0xAB).any()


# ---------------------------------------------------------------- 4: the async form

def test_moments_row_map_on_a_stream_with_a_render_behind(spt, ctx1, oracle, golden_scenes):
    import torch
    o = oracle_frame(oracle, golden_scenes)
    strip, parts, part = 4, 3, 1
    ys = [y for y in range(H1) if (y // strip) % parts == part]
    assert spt.rows_count(0, H1, strip, parts, part) == len(ys) and 0 < len(ys) < H1
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    n = len(ys) * W1
    t_rgba = torch.full((n, 4), -1.0, dtype=torch.float32, device=dev)
    t_mom = torch.full((n, 4), -2.0, dtype=torch.float32, device=dev)
    t_g = torch.full((W1 * H1 * 3,), 0xAB, dtype=torch.uint8, device=dev)
    t_next = torch.full((H1 * W1, 4), -3.0, dtype=torch.float32, device=dev)
    t_mom2 = torch.full((n, 4), -2.0, dtype=torch.float32, device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ctx1.render_moments_async(0, H1, strip, parts, part, 0, W1, t_rgba.data_ptr(), t_g.data_ptr(), t_mom.data_ptr(),
                              stream.cuda_stream)
    # at once, on the same stream: the next render rewrites the sample words
    ctx1.render_rows_async(spt._native.MODE_SEGMENT, 0, H1, 1, 1, 0, 0, W1, t_next.data_ptr(), 0, stream.cuda_stream)
    # and the moments alone behind it
    ctx1.render_moments_async(0, H1, strip, parts, part, 0, W1, 0, 0, t_mom2.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    ctx1.synchronize()
    same_mom(t_mom.cpu().numpy(), o["mom"].reshape(H1, W1, 4)[ys].reshape(-1, 4), "mom of strip 4, part 1 of 3")
    same_mom(t_mom2.cpu().numpy(), t_mom.cpu().numpy(), "mom alone")
    assert np.array_equal(bits(t_rgba.cpu().numpy()[:, :3]), bits(o["rgba"][ys].reshape(-1, 4)[:, :3])), "rgba of the rows"
    assert np.array_equal(bits(t_next.cpu().numpy()[:, :3]), bits(o["rgba"].reshape(-1, 4)[:, :3])), "the render behind it"
    g = t_g.cpu().numpy().reshape(H1, W1 * 3)
    want_g = np.full((H1, W1 * 3), 0xAB, np.uint8)
    for y in ys:
        want_g[H1 - 1 - y] = o["g"].reshape(H1, W1 * 3)[H1 - 1 - y]
    assert np.array_equal(g, want_g), "g_data rows of the part, the rest untouched"


# ---------------------------------------------------------------- 5: NaN colours

def test_nan_colours_give_nan_moments(spt, oracle):
    v = D.by_id("nonfinite/colours")
    W, H, _, depth, seed = v.frame
    yB, yE, xB, xE = 0, H, 0, W
    spp = 3
    view = spt.camera_basis(v.eye, v.look, D.UP)
    osc = oracle.OracleScene(*v.arrays)
    fr = oracle.make_frame(view, v.eye, v.sky, W, H, spp, depth, seed)
    col = oracle.trace_region(osc, fr, yB, yE, xB, xE)[0]
    exp = expected_moments(col)
    nan = np.isnan(exp[:, :3]).any(axis=1)
    print(f"{v.id}: {int(nan.sum())} of {len(exp)} pixels have NaN moments")
    assert nan.any() and not nan.all()
    c = spt.Context(0)
    try:
        c.set_scene(spt.Scene(*v.arrays))
        c.set_camera(view, v.eye, v.sky)
        c.set_params(W, H, spp, depth, seed)
        _, mom = c.render_moments(yB, yE, xB, xE)
        same_mom(mom, exp, v.id, nan=True)
    finally:
        c.close()


# ---------------------------------------------------------------- 6: the service resident

def test_moments_between_two_service_renders(spt, golden_scenes):
    W, H, spp = 64, 40, 4
    c = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        exp = expected_moments(c.render_samples(0, H, 0, W, spp))
        c.service_start()
        before = c.render_segment(0, H, 0, W)
        assert c.stats()["svc_running"] == 1
        rgba, mom = c.render_moments(0, H, 0, W)
        after = c.render_segment(0, H, 0, W)
        assert c.stats()["svc_running"] == 1
        assert np.array_equal(bits(before), bits(after)) and np.array_equal(bits(before), bits(rgba))
        same_mom(mom, exp, "moments between two service renders")
        c.service_stop()
    finally:
        c.close()


# ---------------------------------------------------------------- 7: moments errors

def test_moments_state_and_argument_errors(spt, golden_scenes):
    from test_gpu_parity import scene_from
    L = spt._native.lib()
    c = spt.Context(0)
    try:
        h = c.handle
        W, H, spp = 32, 16, 2
        n = 8 * 4
        rgba = np.full((n, 4), -3.0, np.float32)
        mom = np.full((n, 4), -4.0, np.float32)
        g = np.full(W * H * 3, 0xAB, np.uint8)
        rp, mp, gp = (a.ctypes.data_as(P) for a in (rgba, mom, g))

        def blocking(yB, yE, xB, xE, r=rp, b=gp, m=mp):
            return L.spt_render_moments(h, yB, yE, xB, xE, r, b, m)

        def rows(yB, yE, strip, parts, part, xB, xE, r=rp, b=gp, m=mp):
            return L.spt_render_moments_async(h, yB, yE, strip, parts, part, xB, xE, r, b, m, None)

        assert blocking(0, 4, 0, 8) == 2 and b"scene" in L.spt_last_error(h)
        c.set_scene(scene_from(spt, golden_scenes, "random"))
        assert rows(0, 4, 1, 1, 0, 0, 8) == 2 and b"camera" in L.spt_last_error(h)
        c.set_camera(golden_scenes["view"], EYE, SKY)
        # unset params
        assert blocking(0, 4, 0, 8) == 2 and b"params" in L.spt_last_error(h)
        assert rows(0, 4, 1, 1, 0, 0, 8) == 2 and b"params" in L.spt_last_error(h)
        c.set_params(W, H, spp, 4, 1)
        for bad in ((0, 17, 0, 8), (0, 4, 0, 33), (4, 3, 0, 8), (0, 4, 8, 7), (0, 0xFFFFFFFF, 0, 8)):
            assert blocking(*bad) == 1, bad
            assert rows(bad[0], bad[1], 1, 1, 0, bad[2], bad[3]) == 1, bad
        for strip, parts, part in ((0, 1, 0), (1, 0, 0), (1, 2, 2), (1, 1, 1)):
            assert rows(0, 4, strip, parts, part, 0, 8) == 1, (strip, parts, part)
        # a null mom
        assert blocking(0, 4, 0, 8, m=None) == 1 and b"null" in L.spt_last_error(h)
        assert rows(0, 4, 1, 1, 0, 0, 8, m=None) == 1 and b"null" in L.spt_last_error(h)
        # a region over one sample batch: 32 pixels x 2 spp x 4 B = 256 B of words
        c.synchronize()
        launches = c.stats()["launches"]
        c.set_workspace(128)
        assert blocking(0, 4, 0, 8) == 1 and b"workspace" in L.spt_last_error(h)
        assert rows(0, 4, 1, 1, 0, 0, 8) == 1 and b"workspace" in L.spt_last_error(h)
        assert c.stats()["launches"] == launches, "nothing was rendered"
        # an empty rectangle is SPT_OK and touches nothing, whatever the pointers
        for empty in ((3, 3, 0, 8), (0, 4, 5, 5), (16, 16, 32, 32)):
            assert blocking(*empty) == 0 and blocking(*empty, None, None, None) == 0, empty
            assert rows(empty[0], empty[1], 1, 1, 0, empty[2], empty[3], None, None, None) == 0, empty
        assert (rgba == -3.0).all() and (mom == -4.0).all() and (g == 0xAB).all()
        # and the same buffers are filled by a valid call once the batch fits
        c.set_workspace(256)
        assert blocking(12, 16, 24, 32) == 0, L.spt_last_error(h)
        assert (rgba[:, :3] != -3.0).all() and (mom != -4.0).all() and (mom[:, 3] == spp).all()
        assert (g != 0xAB).any() and c.stats()["launches"] == launches + 1
    finally:
        c.close()


# ---------------------------------------------------------------- the filter's inputs and the helper's side

def random_mom(W, H, seed, spp=4):
    """Variances from 0 (a third of the pixels) to 4000 on the colours' 0..255 scale."""
    r = np.random.default_rng(seed)
    mom = np.zeros((H, W, 4), np.float32)
    mom[:, :, 0] = r.uniform(0, 255, (H, W))
    mom[:, :, 2] = np.where(r.uniform(size=(H, W)) < 1 / 3, 0.0, r.uniform(0, 4000, (H, W)))
    mom[:, :, 1] = mom[:, :, 2] + mom[:, :, 0] * mom[:, :, 0]
    mom[:, :, 3] = spp
    return mom


_cases, _want = {}, {}


def inputs(name, oracle=None, golden_scenes=None):
    """Named inputs, made once: 'frame1' (the oracle frame), 'nonfinite' (it with test 11's
    moments), or 'WxH' (random inputs seeded by the shape): (rgba, feat, mom, W, H)."""
    if name not in _cases:
        if name == "frame1":
            o = oracle_frame(oracle, golden_scenes)
            _cases[name] = (o["rgba"], o["feat"], o["mom"].reshape(H1, W1, 4), W1, H1)
        elif name == "nonfinite":
            rgba, feat, mom, _, _ = inputs("frame1", oracle, golden_scenes)
            mom = mom.copy()
            for (y, x), v in NONFINITE_MOM.items():
                mom[y, x, 2] = v
            _cases[name] = (rgba, feat, mom, W1, H1)
        else:
            W, H = (int(v) for v in name.split("x"))
            _cases[name] = random_inputs(W, H, 1000 * W + H) + (random_mom(W, H, 77 * W + H), W, H)
    return _cases[name]


def want(name, sigmas=DEFAULT_VAR_SIGMAS, var_floor=DEFAULT_VAR_FLOOR, levels=3, reverse=False):
    key = (name, tuple(sigmas), var_floor, levels, reverse)
    if key not in _want:
        rgba, feat, mom, W, H = _cases[name]
        _want[key] = expected_denoise_var(rgba, feat, mom, W, H, sigmas, var_floor, levels, reverse_taps=reverse)
    return _want[key]


def same_var(got, exp, what, nan=False):
    same(got[..., None, None], exp[..., None, None], what, nan=nan)


# ---------------------------------------------------------------- 8: the oracle frame, levels 1..5

@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_filter_on_the_oracle_frame_at_every_level(ctx, oracle, golden_scenes, levels):
    rgba, feat, mom, W, H = inputs("frame1", oracle, golden_scenes)
    exp, exp_var, _ = want("frame1", levels=levels)
    rev, rev_var, _ = want("frame1", levels=levels, reverse=True)
    moved, order = int(changed(exp, rgba).sum()), int(changed(exp, rev).sum())
    order_var = int((bits(exp_var) != bits(rev_var)).sum())
    print(f"denoise_var 45x37x7, {levels} levels: {moved} of {W * H} pixels change, the tap order matters in {order} "
          f"(out_var: {order_var})")
    assert moved >= 0.9 * W * H and order >= 1 and order_var >= 1
    # the variance is live: the plain filter at the same sigmas gives another image
    assert changed(exp, expected_denoise(rgba, feat, W, H, DEFAULT_VAR_SIGMAS, levels)[0]).mean() > 0.25
    out, var = ctx.denoise_variance(rgba, feat, mom, levels=levels, variance=True)
    same(out, exp, f"45x37x7, {levels} levels")
    same_var(var, exp_var, f"45x37x7, {levels} levels: out_var")
    assert np.array_equal(bits(out[..., 3]), bits(rgba[..., 3])), "w passes through"


# ---------------------------------------------------------------- 9: small and ragged shapes, many blocks

@pytest.mark.parametrize("levels", [1, 4])
@pytest.mark.parametrize("shape", ["1x1", "1x40", "40x1", "15x15", "16x16", "17x17", "33x18"])
def test_filter_on_small_and_ragged_shapes(ctx, shape, levels):
    rgba, feat, mom, W, H = inputs(shape)
    exp, exp_var, _ = want(shape, levels=levels)
    assert np.isfinite(exp).all() and np.isfinite(exp_var).all()
    if W * H > 1:
        assert (mom[..., 2] == 0).any() and (mom[..., 2] > 0).any()
        assert changed(exp, rgba).mean() > 0.9
    out, var = ctx.denoise_variance(rgba, feat, mom, levels=levels, variance=True)
    same(out, exp, f"{shape}, {levels} levels")
    same_var(var, exp_var, f"{shape}, {levels} levels: out_var")
    assert np.array_equal(bits(out[..., 3]), bits(rgba[..., 3])), "w passes through (random w lanes)"


def test_filter_on_300x200_at_the_widest_step(ctx):
    rgba, feat, mom, W, H = inputs("300x200")
    exp, exp_var, _ = want("300x200", levels=8)
    assert changed(exp, rgba).all()
    assert changed(exp, want("300x200", levels=7)[0]).mean() > 0.5  # the last level alone (step 128) still moves pixels
    out, var = ctx.denoise_variance(rgba, feat, mom, levels=8, variance=True)
    same(out, exp, "300x200, 8 levels")
    same_var(var, exp_var, "300x200, 8 levels: out_var")


# ---------------------------------------------------------------- 10: every term of the weight

OFF = {"color": (INF, 0.1, 0.25, 0.5), "albedo": (4.0, INF, 0.25, 0.5), "normal": (4.0, 0.1, INF, 0.5),
       "depth": (4.0, 0.1, 0.25, INF), "all": (INF, INF, INF, INF)}


@pytest.mark.parametrize("off", list(OFF))
def test_filter_with_each_sigma_switched_off(ctx, oracle, golden_scenes, off):
    rgba, feat, mom, W, H = inputs("frame1", oracle, golden_scenes)
    exp, exp_var, _ = want("frame1", sigmas=OFF[off])
    assert changed(exp, want("frame1")[0]).mean() > 0.25, off  # the term was live
    c, a, n, z = OFF[off]
    out, var = ctx.denoise_variance(rgba, feat, mom, sigma_color=c, sigma_albedo=a, sigma_normal=n, sigma_depth=z, variance=True)
    same(out, exp, f"sigma {off} = inf")
    same_var(var, exp_var, f"sigma {off} = inf: out_var")


@pytest.mark.parametrize("floor", [1e-6, 1e6])
def test_filter_at_the_ends_of_the_variance_floor(ctx, oracle, golden_scenes, floor):
    rgba, feat, mom, W, H = inputs("frame1", oracle, golden_scenes)
    exp, exp_var, _ = want("frame1", var_floor=floor)
    assert changed(exp, want("frame1")[0]).mean() > 0.25, floor  # the floor was live
    assert np.isfinite(exp).all() and np.isfinite(exp_var).all()
    out, var = ctx.denoise_variance(rgba, feat, mom, var_floor=floor, variance=True)
    same(out, exp, f"var_floor {floor}")
    same_var(var, exp_var, f"var_floor {floor}: out_var")


# ---------------------------------------------------------------- 11: non-finite moments

NONFINITE_MOM = {(10, 20): np.nan, (18, 30): np.inf, (36, 44): -np.inf}  # (y, x); the last is a corner


def test_filter_passes_nonfinite_variances_through(ctx, oracle, golden_scenes):
    rgba, feat, mom, W, H = inputs("nonfinite", oracle, golden_scenes)
    exp, exp_var, skipped = want("nonfinite")
    assert np.isfinite(exp).all()
    assert sorted(zip(*np.nonzero(~np.isfinite(exp_var)))) == sorted(NONFINITE_MOM)
    for at in NONFINITE_MOM:
        assert np.array_equal(bits(exp[at]), bits(rgba[at])), at  # passed through
    assert skipped >= 1 and changed(exp, rgba).sum() >= 0.9 * W * H
    out, var = ctx.denoise_variance(rgba, feat, mom, variance=True)
    same(out, exp, "non-finite moments")
    same_var(var, exp_var, "non-finite moments: out_var", nan=True)


# ---------------------------------------------------------------- 12: the g_data bytes

def test_filter_bytes_with_and_without_the_float_output(spt, ctx, oracle, golden_scenes):
    rgba, feat, mom, W, H = inputs("frame1", oracle, golden_scenes)
    exp, exp_var, _ = want("frame1")
    exp8 = expected_bytes(oracle, exp, W, H)
    assert len(np.unique(exp8)) > 50 and (exp8 != expected_bytes(oracle, rgba, W, H)).mean() > 0.25
    out, g = ctx.denoise_variance(rgba, feat, mom, g_data=True)
    same(out, exp, "float output beside the bytes")
    assert np.array_equal(g, exp8), f"{(g != exp8).sum()} bytes differ"
    out, g, var = ctx.denoise_variance(rgba, feat, mom, g_data=True, variance=True)
    same_var(var, exp_var, "out_var beside both")
    assert np.array_equal(g, exp8)
    # the bytes alone, into the middle of a sentinel-filled buffer
    L = spt._native.lib()
    pad = 64
    buf = np.full(W * H * 3 + 2 * pad, 0xAB, np.uint8)
    rc = L.spt_denoise_var(ctx.handle, W, H, rgba.ctypes.data_as(P), feat.ctypes.data_as(P), mom.ctypes.data_as(P),
                           *DEFAULT_VAR_SIGMAS, DEFAULT_VAR_FLOOR, 3, None, P(buf.ctypes.data + pad), None)
    assert rc == 0, L.spt_last_error(ctx.handle)
    assert np.array_equal(buf[pad:-pad], exp8), "bytes alone"
    assert (buf[:pad] == 0xAB).all() and (buf[-pad:] == 0xAB).all(), "bytes outside the image"


# ---------------------------------------------------------------- 13: device pointers, two streams

def test_filter_device_pointers_on_two_streams(spt, ctx):
    import torch
    rgba, feat, mom, W, H = inputs("300x200")
    dev = torch.device("cuda", 0)
    t_rgba, t_feat, t_mom = (torch.from_numpy(a).to(dev) for a in (rgba, feat, mom))
    calls = []
    for levels in (8, 3):
        nb = spt.denoise_scratch_bytes(W, H, levels)
        calls.append(dict(levels=levels, stream=torch.cuda.Stream(device=dev),
                          out=torch.full((H, W, 4), -1.0, dtype=torch.float32, device=dev),
                          var=torch.full((H, W), -4.0, dtype=torch.float32, device=dev),
                          g=torch.full((W * H * 3,), 0xAB, dtype=torch.uint8, device=dev),
                          scratch=torch.full((nb // 4,), -2.0, dtype=torch.float32, device=dev)))
    for c in calls:
        c["stream"].wait_stream(torch.cuda.current_stream(dev))
    for c in calls:  # both enqueued before either is waited for
        ctx.denoise_variance_async(W, H, t_rgba.data_ptr(), t_feat.data_ptr(), t_mom.data_ptr(), levels=c["levels"],
                                   d_out=c["out"].data_ptr(), d_rgb8=c["g"].data_ptr() if c["levels"] == 3 else 0,
                                   d_out_var=c["var"].data_ptr() if c["levels"] == 8 else 0,
                                   d_scratch=c["scratch"].data_ptr(), stream=c["stream"].cuda_stream)
    for c in calls:
        c["stream"].synchronize()
    for c in calls:
        exp, exp_var, _ = want("300x200", levels=c["levels"])
        same(c["out"].cpu().numpy(), exp, f"async, {c['levels']} levels")
        if c["levels"] == 8:
            same_var(c["var"].cpu().numpy(), exp_var, "async: out_var")
    assert (calls[0]["g"].cpu().numpy() == 0xAB).all() and (calls[1]["var"].cpu().numpy() == -4.0).all()
    assert np.array_equal(calls[1]["g"].cpu().numpy(), ctx.denoise_variance(rgba, feat, mom, g_data=True)[1])
    for t, a in ((t_rgba, rgba), (t_feat, feat), (t_mom, mom)):
        assert np.array_equal(bits(t.cpu().numpy()), bits(a))


# ---------------------------------------------------------------- 14: filter errors

def test_filter_argument_errors(spt, ctx):
    L = spt._native.lib()
    h = ctx.handle
    W, H = 8, 4
    n = W * H
    rgba, feat, mom, _, _ = inputs("8x4")
    out = np.full((H, W, 4), -3.0, np.float32)
    var = np.full((H, W), -4.0, np.float32)
    g = np.full(n * 3, 0xAB, np.uint8)
    scratch = np.full(2 * n * 4, -5.0, np.float32)
    rp, fp, mp, op, vp, gp, sp = (a.ctypes.data_as(P) for a in (rgba, feat, mom, out, var, g, scratch))
    S = DEFAULT_VAR_SIGMAS

    def blocking(w=W, hh=H, r=rp, f=fp, m=mp, s=S, vf=1.0, levels=3, o=op, b=gp, v=vp):
        return L.spt_denoise_var(h, w, hh, r, f, m, *s, vf, levels, o, b, v)

    def rows(w=W, hh=H, r=rp, f=fp, m=mp, s=S, vf=1.0, levels=3, o=op, b=gp, v=vp, scr=sp):
        return L.spt_denoise_var_async(h, w, hh, r, f, m, *s, vf, levels, o, b, v, scr, None)

    for call in (blocking, rows):
        assert call(r=None) == 1 and b"null" in L.spt_last_error(h)
        assert call(f=None) == 1 and b"null" in L.spt_last_error(h)
        assert call(m=None) == 1 and b"null mom" in L.spt_last_error(h)
        assert call(o=None, b=None) == 1 and b"null" in L.spt_last_error(h)
        assert call(o=None, b=None, v=vp) == 1  # out_var alone is no output
        for levels in (0, 9, 0xFFFFFFFF):
            assert call(levels=levels) == 1 and b"levels" in L.spt_last_error(h), levels
        for t in range(4):
            for bad in (float("nan"), 0.0, -0.0, -1.0, -INF):
                s = list(S)
                s[t] = bad
                assert call(s=s) == 1 and b"sigma" in L.spt_last_error(h), (t, bad)
        for bad in (float("nan"), 0.0, -0.0, -1.0, INF, -INF):
            assert call(vf=bad) == 1 and b"var_floor" in L.spt_last_error(h), bad
        assert call(w=65536, hh=32768) == 1  # 2^31 pixels
        # an output that overlaps an input: wholly, or by its last bytes
        assert call(o=rp) == 1 and b"overlaps" in L.spt_last_error(h)
        assert call(o=mp) == 1 and b"overlaps mom" in L.spt_last_error(h)
        assert call(b=P(mom.ctypes.data + n * 16 - 1)) == 1 and b"overlaps mom" in L.spt_last_error(h)
        assert call(b=fp) == 1 and b"overlaps" in L.spt_last_error(h)
        assert call(v=rp) == 1 and b"out_var overlaps rgba" in L.spt_last_error(h)
        assert call(v=P(feat.ctypes.data + n * 32 - 4)) == 1 and b"out_var overlaps feat" in L.spt_last_error(h)
        assert call(v=mp) == 1 and b"out_var overlaps mom" in L.spt_last_error(h)
        assert call(v=P(out.ctypes.data + n * 16 - 4)) == 1 and b"out_var overlaps out_rgba" in L.spt_last_error(h)
        assert call(v=gp) == 1 and b"out_var overlaps out_rgb8" in L.spt_last_error(h)
        # the empty image is SPT_OK and touches nothing, whatever the pointers
        assert call(w=0) == 0 and call(hh=0) == 0 and call(w=0, hh=0, m=None, o=None, b=gp) == 0
    assert rows(scr=None) == 1 and b"scratch" in L.spt_last_error(h)
    assert rows(o=sp) == 1 and b"overlaps" in L.spt_last_error(h)
    assert rows(v=P(scratch.ctypes.data + 2 * n * 16 - 4)) == 1 and b"out_var overlaps scratch" in L.spt_last_error(h)
    assert (out == -3.0).all() and (var == -4.0).all() and (g == 0xAB).all() and (scratch == -5.0).all()
    # and the same buffers are filled by a valid call
    assert blocking() == 0, L.spt_last_error(h)
    exp, exp_var, _ = want("8x4")
    same(out, exp, "8x4 after the errors")
    same_var(var, exp_var, "8x4 after the errors: out_var")
    assert (g != 0xAB).any()


# ---------------------------------------------------------------- 15: the Python interface end to end

def test_render_denoised_with_and_without_the_variance(spt, golden_scenes):
    W, H, spp = 96, 64, 4
    c = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        rgba, mom = c.render_moments(0, H, 0, W)
        fb = c.feature_buffers()
        feat = np.concatenate([fb["albedo"], fb["coverage"][..., None], fb["normal"], fb["depth"][..., None]], axis=2)
        same_mom(mom, expected_moments(c.render_samples(0, H, 0, W, spp)), "the frame's moments")
        assert np.array_equal(bits(rgba), bits(c.render_frame()))
        exp, exp_var, _ = expected_denoise_var(rgba, feat, mom, W, H)
        by_hand = c.denoise_variance(rgba.reshape(H, W, 4), fb, mom)
        same(by_hand, exp, "denoise_variance(render_moments, feature_buffers)")
        same(c.render_denoised(variance=True), by_hand, "render_denoised(variance=True)")
        exp2, _, _ = expected_denoise_var(rgba, feat, mom, W, H, (2.0, INF, 0.25, 0.5), 0.25, 2)
        assert changed(exp2, exp).mean() > 0.25
        same(c.render_denoised(variance=True, sigma_color=2.0, sigma_albedo=INF, var_floor=0.25, levels=2), exp2,
             "render_denoised(variance=True) with keywords")
        # without it: exactly the plain filter, as before
        plain, _ = expected_denoise(rgba, feat, W, H, DEFAULT_SIGMAS, 3)
        assert changed(plain, exp).mean() > 0.25
        same(c.render_denoised(), plain, "render_denoised()")
        same(c.render_denoised(variance=False), c.denoise(rgba.reshape(H, W, 4), fb), "render_denoised(variance=False)")
    finally:
        c.close()
