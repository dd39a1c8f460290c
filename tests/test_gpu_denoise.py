"""The denoiser (spt_denoise, spt_denoise_async) against its definition, bit for bit: the
edge-avoiding a-trous filter guided by the feature buffers (include/spt_hip.h "denoiser",
DESIGN.md §4.11).

What the filter must return comes from tests/denoise.py (numpy; the bytes through the
oracle's spo_write_pixel).  The "oracle frame" is the golden `random` scene through
golden_scenes["view"] from the eye [0, 1, -3], seed 3, depth 8, rendered by the oracle, with
tests/features.py's feature buffers.  Every test asserts on the helper's answer that its
case is live before it compares anything; no comparison has a tolerance.

    1  the oracle frame at 45 x 37 x 7, levels 1..5                ragged tiles, taps mostly outside at step 16
    2  1x1, 1x40, 40x1, 15x15, 16x16, 17x17, 33x18, levels 1 and 4  lattices shorter than / one past a tile, cov == 0
    3  300 x 200 random, levels 8 (step 128) and 3                  many blocks, ragged tiles in every lattice
    4  each sigma +inf, and all four (the plain B3 wavelet)         every term of the weight
    5  non-finite colours and features                              pass through, never spread
    6  the g_data bytes, with and without the float output          spo_write_pixel, the frame's layout
    7  device pointers on two caller streams, a scratch each        the async form
    8  the GPU's own render and feature_buffers(); render_denoised  the Python interface end to end
    9  a render, a denoise, the same render (launched / service)    non-interference
    10 argument errors; the empty image
"""
import ctypes

import numpy as np
import pytest

from denoise import DEFAULT_SIGMAS, expected_bytes, expected_denoise
from test_denoise_helper import oracle_inputs
from test_gpu_cast import COUNTERS
from test_gpu_features import DEPTH, SEED, make_ctx
from test_gpu_parity import bits

pytestmark = pytest.mark.gpu

W1, H1, S1 = 45, 37, 7
INF = float("inf")


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
    """A context without scene, camera or params: the denoiser needs none."""
    c = spt.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- inputs and the helper's side

def random_inputs(W, H, seed):
    """Colours in 0..255 (w too: it passes through), albedo in 0..1, normals of length <= 1,
    cov from {0, 0.5, 1}, dep in 0..20."""
    r = np.random.default_rng(seed)
    rgba = r.uniform(0, 255, (H, W, 4)).astype(np.float32)
    feat = np.zeros((H, W, 2, 4), np.float32)
    feat[:, :, 0, :3] = r.uniform(0, 1, (H, W, 3))
    feat[:, :, 0, 3] = r.choice(np.array([0.0, 0.5, 1.0], np.float32), (H, W))
    v = r.normal(size=(H, W, 3))
    v /= np.maximum(np.linalg.norm(v, axis=2, keepdims=True), 1e-9)
    feat[:, :, 1, :3] = v * r.uniform(0, 0.999, (H, W, 1))
    feat[:, :, 1, 3] = r.uniform(0, 20, (H, W))
    assert (np.linalg.norm(feat[:, :, 1, :3].astype(np.float64), axis=2) <= 1.0).all()
    return rgba, feat


_cases, _want = {}, {}


def inputs(name, oracle=None, golden_scenes=None):
    """Named inputs, made once: 'frame1' (the oracle frame at 45 x 37 x 7), 'nonfinite' (it
    with test 5's pixels), or 'WxH' (random_inputs seeded by the shape)."""
    if name not in _cases:
        if name == "frame1":
            rgba, feat = oracle_inputs(oracle, golden_scenes, W1, H1, S1)
            _cases[name] = (rgba.reshape(H1, W1, 4), feat.reshape(H1, W1, 2, 4), W1, H1)
        elif name == "nonfinite":
            rgba, feat, _, _ = inputs("frame1", oracle, golden_scenes)
            rgba, feat = rgba.copy(), feat.copy()
            for (y, x), v in NONFINITE_COLOURS.items():
                rgba[y, x, :3] = v
            for (y, x), (row, lane) in NONFINITE_FEATURES.items():
                feat[y, x, row, lane] = np.nan
            _cases[name] = (rgba, feat, W1, H1)
        else:
            W, H = (int(v) for v in name.split("x"))
            _cases[name] = random_inputs(W, H, 1000 * W + H) + (W, H)
    return _cases[name]


def want(name, sigmas=DEFAULT_SIGMAS, levels=3, reverse=False):
    key = (name, tuple(sigmas), levels, reverse)
    if key not in _want:
        rgba, feat, W, H = _cases[name]
        _want[key] = expected_denoise(rgba, feat, W, H, sigmas, levels, reverse_taps=reverse)
    return _want[key]


def changed(out, rgba):
    """Pixels whose rgb differs on bits."""
    return (bits(out[..., :3]) != bits(rgba[..., :3])).any(axis=2)


def same(got, exp, what, nan=False):
    """got == exp on bits (with nan=True a NaN matches a NaN at the same place)."""
    assert got.shape == exp.shape and got.dtype == np.float32, (what, got.shape, exp.shape)
    differ = bits(got) != bits(exp)
    if nan:
        gn, en = np.isnan(got), np.isnan(exp)
        assert np.array_equal(gn, en), f"{what}: NaN in other lanes"
        differ &= ~en
    bad = np.argwhere(differ)
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError(f"{what}: {len(np.unique(bad[:, :2], axis=0))} of {got.shape[0] * got.shape[1]} pixels differ; "
                             f"first at (y, x, lane) {at}: got {got[at]!r}, want {exp[at]!r}")


# ---------------------------------------------------------------- 1: the oracle frame, levels 1..5

@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_oracle_frame_at_every_level(ctx, oracle, golden_scenes, levels):
    rgba, feat, W, H = inputs("frame1", oracle, golden_scenes)
    exp, _ = want("frame1", levels=levels)
    rev, _ = want("frame1", levels=levels, reverse=True)
    moved, order = int(changed(exp, rgba).sum()), int(changed(exp, rev).sum())
    print(f"denoise 45x37x7, {levels} levels: {moved} of {W * H} pixels change, the tap order matters in {order}")
    # The helper's figures: 1646, 1664, 1665, 1665, 1665 pixels change and the order matters in
    # 1637, 1646, 1644, 1650, 1649.  From 3 levels on every pixel changes.  At 1 and 2 levels a
    # few ground pixels stay: 18 of the 19 at 1 level have 25 taps of one and the same colour,
    # a fixed point of any normalised filter (the 19th's mean rounds back to its value).
    assert moved == W * H if levels >= 3 else moved >= 0.98 * W * H, moved
    assert order >= 1, order
    same(ctx.denoise(rgba, feat, levels=levels), exp, f"45x37x7, {levels} levels")


# ---------------------------------------------------------------- 2: small and ragged shapes

@pytest.mark.parametrize("levels", [1, 4])
@pytest.mark.parametrize("shape", ["1x1", "1x40", "40x1", "15x15", "16x16", "17x17", "33x18"])
def test_small_and_ragged_shapes(ctx, shape, levels):
    rgba, feat, W, H = inputs(shape)
    exp, _ = want(shape, levels=levels)
    assert np.isfinite(exp).all()
    if W * H > 1:
        # cov == 0 pixels (z = 0) among cov > 0 ones, and the filter moves pixels
        cov = feat[:, :, 0, 3]
        assert (cov == 0).any() and (cov > 0).any()
        assert changed(exp, rgba).mean() > 0.9
    same(ctx.denoise(rgba, feat, levels=levels), exp, f"{shape}, {levels} levels")


# ---------------------------------------------------------------- 3: many blocks, the widest step

@pytest.mark.parametrize("levels", [8, 3])
def test_300x200_at_the_widest_step_and_at_three_levels(ctx, levels):
    rgba, feat, W, H = inputs("300x200")
    exp, _ = want("300x200", levels=levels)
    assert changed(exp, rgba).all()
    if levels == 8:  # the last level alone (step 128) still moves pixels
        assert changed(exp, want("300x200", levels=7)[0]).mean() > 0.5
    else:
        assert changed(exp, want("300x200", levels=levels, reverse=True)[0]).sum() >= 1
    same(ctx.denoise(rgba, feat, levels=levels), exp, f"300x200, {levels} levels")


# ---------------------------------------------------------------- 4: every term of the weight

OFF = {"color": (INF, 0.1, 0.25, 0.5), "albedo": (30.0, INF, 0.25, 0.5), "normal": (30.0, 0.1, INF, 0.5),
       "depth": (30.0, 0.1, 0.25, INF), "all": (INF, INF, INF, INF)}


@pytest.mark.parametrize("off", list(OFF))
def test_each_sigma_switched_off(ctx, oracle, golden_scenes, off):
    rgba, feat, W, H = inputs("frame1", oracle, golden_scenes)
    exp, _ = want("frame1", sigmas=OFF[off])
    # the term was live: without it the answer is another
    assert changed(exp, want("frame1")[0]).mean() > 0.25, off
    if off == "all":
        # the plain B3 wavelet: an interior pixel of a constant image keeps its value
        flat, _ = expected_denoise(np.full((9, 9, 4), 8.0, np.float32), np.zeros((9, 9, 2, 4), np.float32), 9, 9, OFF[off], 1)
        assert flat[4, 4, 0] == 8.0
    c, a, n, z = OFF[off]
    got = ctx.denoise(rgba, feat, sigma_color=c, sigma_albedo=a, sigma_normal=n, sigma_depth=z)
    same(got, exp, f"sigma {off} = inf")


# ---------------------------------------------------------------- 5: non-finite pixels

NONFINITE_COLOURS = {(10, 20): np.nan, (18, 30): np.inf, (36, 44): -np.inf}  # (y, x); the last is a corner
NONFINITE_FEATURES = {(5, 5): (0, 1), (25, 12): (1, 0), (30, 40): (1, 3)}  # alb.g, nrm.x, dep


def test_nonfinite_pixels_pass_through(ctx, oracle, golden_scenes):
    rgba, feat, W, H = inputs("nonfinite", oracle, golden_scenes)
    exp, skipped = want("nonfinite")
    bad = ~np.isfinite(exp[..., :3]).all(axis=2)
    assert sorted(zip(*np.nonzero(bad))) == sorted(NONFINITE_COLOURS)
    for at in list(NONFINITE_COLOURS) + list(NONFINITE_FEATURES):
        assert np.array_equal(bits(exp[at]), bits(rgba[at])), at  # passed through
    assert skipped >= 1
    assert changed(exp, rgba).sum() == W * H - 6
    same(ctx.denoise(rgba, feat), exp, "non-finite pixels", nan=True)


# ---------------------------------------------------------------- 6: the g_data bytes

def test_gdata_bytes_with_and_without_the_float_output(spt, ctx, oracle, golden_scenes):
    rgba, feat, W, H = inputs("frame1", oracle, golden_scenes)
    exp, _ = want("frame1")
    exp8 = expected_bytes(oracle, exp, W, H)
    assert len(np.unique(exp8)) > 50 and (exp8 != expected_bytes(oracle, rgba, W, H)).mean() > 0.25
    out, g = ctx.denoise(rgba, feat, g_data=True)
    same(out, exp, "float output beside the bytes")
    assert np.array_equal(g, exp8), f"{(g != exp8).sum()} bytes differ"
    # the bytes alone, into the middle of a sentinel-filled buffer
    L = spt._native.lib()
    P = ctypes.c_void_p
    pad = 64
    buf = np.full(W * H * 3 + 2 * pad, 0xAB, np.uint8)
    rc = L.spt_denoise(ctx.handle, W, H, rgba.ctypes.data_as(P), feat.ctypes.data_as(P), *DEFAULT_SIGMAS, 3, None,
                       P(buf.ctypes.data + pad))
    assert rc == 0, L.spt_last_error(ctx.handle)
    assert np.array_equal(buf[pad:-pad], exp8), "bytes alone"
    assert (buf[:pad] == 0xAB).all() and (buf[-pad:] == 0xAB).all(), "bytes outside the image"


# ---------------------------------------------------------------- 7: device pointers, two streams

def test_device_pointers_on_two_streams(spt, ctx):
    import torch
    rgba, feat, W, H = inputs("300x200")
    dev = torch.device("cuda", 0)
    t_rgba, t_feat = torch.from_numpy(rgba).to(dev), torch.from_numpy(feat).to(dev)
    calls = []
    for levels in (8, 3):
        nb = spt.denoise_scratch_bytes(W, H, levels)
        assert nb == 2 * W * H * 16
        calls.append(dict(levels=levels, stream=torch.cuda.Stream(device=dev),
                          out=torch.full((H, W, 4), -1.0, dtype=torch.float32, device=dev),
                          g=torch.full((W * H * 3,), 0xAB, dtype=torch.uint8, device=dev),
                          scratch=torch.full((nb // 4,), -2.0, dtype=torch.float32, device=dev)))
    for c in calls:
        c["stream"].wait_stream(torch.cuda.current_stream(dev))
    # both enqueued before either is waited for
    for c in calls:
        ctx.denoise_async(W, H, t_rgba.data_ptr(), t_feat.data_ptr(), levels=c["levels"], d_out=c["out"].data_ptr(),
                          d_rgb8=c["g"].data_ptr() if c["levels"] == 3 else 0, d_scratch=c["scratch"].data_ptr(),
                          stream=c["stream"].cuda_stream)
    for c in calls:
        c["stream"].synchronize()
    for c in calls:
        exp, _ = want("300x200", levels=c["levels"])
        same(c["out"].cpu().numpy(), exp, f"async, {c['levels']} levels")
    assert (calls[0]["g"].cpu().numpy() == 0xAB).all(), "no bytes were asked for"
    g = calls[1]["g"].cpu().numpy()
    assert (g != 0xAB).mean() > 0.9
    # the bytes are the blocking form's (test 6 pins those against the oracle)
    assert np.array_equal(g, ctx.denoise(rgba, feat, g_data=True)[1])
    assert np.array_equal(bits(t_rgba.cpu().numpy()), bits(rgba)) and np.array_equal(bits(t_feat.cpu().numpy()), bits(feat))


# ---------------------------------------------------------------- 8: the GPU's own frame

def test_own_render_and_feature_buffers(spt, golden_scenes):
    W, H, spp = 96, 64, 4
    c = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        rgba = c.render_frame().reshape(H, W, 4)
        fb = c.feature_buffers()
        feat = np.concatenate([fb["albedo"], fb["coverage"][..., None], fb["normal"], fb["depth"][..., None]], axis=2)
        exp, _ = expected_denoise(rgba, feat, W, H, DEFAULT_SIGMAS, 3)
        assert changed(exp, rgba).mean() > 0.9
        same(c.denoise(rgba, fb), exp, "denoise(render_frame, feature_buffers)")
        same(c.denoise(rgba.reshape(-1, 4), c.render_features(0, H, 0, W)).reshape(H, W, 4), exp, "the frame's flat forms")
        same(c.render_denoised(), exp, "render_denoised")
        exp2, _ = expected_denoise(rgba, feat, W, H, (30.0, INF, 0.25, 0.5), 2)
        same(c.render_denoised(sigma_albedo=INF, levels=2), exp2, "render_denoised with keywords")
    finally:
        c.close()


# ---------------------------------------------------------------- 9: non-interference

@pytest.mark.parametrize("service", [False, True], ids=["launched", "service"])
def test_denoise_leaves_renders_and_stats_alone(spt, golden_scenes, service):
    W, H, spp = 64, 40, 4
    rgba, feat, _, _ = inputs("33x18")
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
        got = c.denoise(rgba, feat, levels=4)
        st1 = c.stats()
        assert st1["svc_running"] == 0  # a resident session is ended by the call
        if not service:  # (a session's device counters arrive when it ends: the call ends it)
            assert {k: st0[k] for k in COUNTERS} == {k: st1[k] for k in COUNTERS}
        after = c.render_segment(0, H, 0, W)
        st2 = c.stats()
        assert np.array_equal(bits(before), bits(after))
        if service:  # the next render starts a new session
            assert st2["svc_running"] == 1 and st2["svc_sessions"] > st1["svc_sessions"]
        else:  # the counters move by the renders only
            assert st2["samples"] - st1["samples"] == W * H * spp and st2["launches"] > st1["launches"]
        same(got, want("33x18", levels=4)[0], "denoise between two renders")
        same(c.denoise(rgba, feat, levels=4), got, "denoise after the renders")
        if service:
            c.service_stop()
    finally:
        c.close()


# ---------------------------------------------------------------- 10: errors

def test_denoise_argument_errors(spt, ctx):
    L = spt._native.lib()
    P = ctypes.c_void_p
    h = ctx.handle
    W, H = 8, 4
    n = W * H
    rgba, feat, _, _ = inputs("8x4")
    out = np.full((H, W, 4), -3.0, np.float32)
    g = np.full(n * 3, 0xAB, np.uint8)
    scratch = np.full(2 * n * 4, -5.0, np.float32)
    rp, fp, op, gp, sp = (a.ctypes.data_as(P) for a in (rgba, feat, out, g, scratch))
    S = DEFAULT_SIGMAS

    def blocking(w=W, hh=H, r=rp, f=fp, s=S, levels=3, o=op, b=gp):
        return L.spt_denoise(h, w, hh, r, f, *s, levels, o, b)

    def rows(w=W, hh=H, r=rp, f=fp, s=S, levels=3, o=op, b=gp, scr=sp):
        return L.spt_denoise_async(h, w, hh, r, f, *s, levels, o, b, scr, None)

    assert L.spt_denoise(None, W, H, rp, fp, *S, 3, op, gp) == 1 and b"null" in L.spt_last_error(None)
    assert L.spt_denoise_async(None, W, H, rp, fp, *S, 3, op, gp, sp, None) == 1 and b"null" in L.spt_last_error(None)
    for call in (blocking, rows):
        assert call(r=None) == 1 and b"null" in L.spt_last_error(h)
        assert call(f=None) == 1 and b"null" in L.spt_last_error(h)
        assert call(o=None, b=None) == 1 and b"null" in L.spt_last_error(h)
        for levels in (0, 9, 0xFFFFFFFF):
            assert call(levels=levels) == 1 and b"levels" in L.spt_last_error(h), levels
        for t in range(4):
            for v in (float("nan"), 0.0, -0.0, -1.0, -INF):
                s = list(S)
                s[t] = v
                assert call(s=s) == 1 and b"sigma" in L.spt_last_error(h), (t, v)
        assert call(w=65536, hh=32768) == 1  # 2^31 pixels
        assert call(w=0xFFFFFFFF, hh=0xFFFFFFFF) == 1
        # an output that overlaps an input: wholly, or by its last bytes
        assert call(o=rp) == 1 and b"overlaps" in L.spt_last_error(h)
        assert call(o=P(feat.ctypes.data + n * 32 - 4)) == 1 and b"overlaps" in L.spt_last_error(h)
        assert call(b=P(rgba.ctypes.data + 16)) == 1 and b"overlaps" in L.spt_last_error(h)
        assert call(b=fp) == 1 and b"overlaps" in L.spt_last_error(h)
        # the empty image is SPT_OK and touches nothing, whatever the pointers
        assert call(w=0) == 0 and call(hh=0) == 0 and call(w=0, hh=0, o=None, b=gp) == 0
    # the async form's scratch: null where some is needed, or under an output
    assert rows(scr=None) == 1 and b"scratch" in L.spt_last_error(h)
    assert rows(scr=None, levels=2) == 1
    assert rows(o=sp) == 1 and b"overlaps" in L.spt_last_error(h)
    assert rows(b=P(scratch.ctypes.data + 2 * n * 16 - 1)) == 1 and b"overlaps" in L.spt_last_error(h)
    assert (out == -3.0).all() and (g == 0xAB).all() and (scratch == -5.0).all()
    # and the same buffers are filled by a valid call
    assert blocking() == 0, L.spt_last_error(h)
    exp, _ = want("8x4")
    same(out, exp, "8x4 after the errors")
    assert (g != 0xAB).any()
    # one level needs no scratch
    import torch
    dev = torch.device("cuda", 0)
    t_rgba, t_feat = torch.from_numpy(rgba).to(dev), torch.from_numpy(feat).to(dev)
    t_out = torch.full((H, W, 4), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.denoise_async(W, H, t_rgba.data_ptr(), t_feat.data_ptr(), levels=1, d_out=t_out.data_ptr(), d_scratch=0)
    ctx.synchronize()
    torch.cuda.synchronize(dev)
    same(t_out.cpu().numpy(), want("8x4", levels=1)[0], "one level without scratch")
