"""The fold through the scene's colour table (spt_codes.h, spt_decode.h) against its
definition: a pixel is the in-order float32 sum of its samples' colours, times 1 / spp
(RenderSegment) or 1 / the samples that finished (RenderSegmentTask), and its g_data bytes
are gamma_byte of that.  The per-sample colours come from spt_render_samples, whose kernel
keeps the arithmetic decode (decode_sample); the sums are formed here, one float32 add per
sample, on the device's own adder (torch), so NaN and inf compare by bit pattern too.
The table serves the launched renders (spt_render_rows_async and what shares its path), so
the frames here are rendered through the device-pointer entry point; the batched host calls
keep the arithmetic decode and must give the same bits.

Shapes: 9 x 9 regions (ragged 8 x 8 tiles on both edges); spp 1, 8, 9, 17 (no full run of
8 words, one run, a run and a remainder, two runs and a remainder); bounces 1, 3, 50 (a
one-row table, a short one, config 2's).  Run on an MI355X with `pytest -m gpu`.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EYE, LOOK, UP, SKY = [0, 1, -3, 0], [0, 1, 0, 0], [0, 1, 0, 0], [137, 207, 240, 0]
CAP_BYTES = 32 << 20  # kCtabMaxBytes
FW, FH = 40, 30       # frame of the small cases
REGION = (11, 20, 15, 24)  # yB, yE, xB, xE: 9 x 9


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert not len(bad), (f"{what}: {len(bad)} of {g.size} lanes differ; first at {tuple(bad[0])}: "
                          f"got {g[tuple(bad[0])]:#010x} want {w[tuple(bad[0])]:#010x}")


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
    c = spt.Context(0)
    yield c
    c.close()


def scene_from(spt, gs, name):
    return spt.Scene(*(gs[f"{name}_{k}"] for k in ("centers", "radii", "colors", "materials", "fuzz")))


def setup(ctx, spt, scene, w, h, spp, b, seed=1):
    ctx.set_scene(scene)
    ctx.set_camera(spt.camera_basis(EYE, LOOK, UP), EYE, SKY)
    ctx.set_params(w, h, spp, b, seed)


def gamma_bytes(rgb):
    """gamma_byte (spt_device.h) of float32 colours: f2u8(roundf(sqrtf(c / 255.f) * 255.f)),
    f2u8 = 0 outside the int32 range (NaN included), else the int32's low byte."""
    with np.errstate(all="ignore"):
        c = np.asarray(rgb, np.float32)
        v = (np.sqrt(c / np.float32(255)) * np.float32(255)).astype(np.float32)
        r = np.trunc(v.astype(np.float64) + np.copysign(0.5, v.astype(np.float64)))  # roundf: halves away from 0
        ok = (r > -2147483648.0) & (r < 2147483648.0)
        return np.where(ok, np.where(ok, r, 0).astype(np.int64) & 0xFF, 0).astype(np.uint8)


def fold_of_samples(samp, task):
    """The definition: samp[p, s] = {r, g, b, counted} in sample order -> float32 pixels."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(samp)).cuda()
    acc = torch.zeros((t.shape[0], 3), dtype=torch.float32, device="cuda")
    cnt = np.zeros(t.shape[0], np.float32)
    for s in range(t.shape[1]):
        if task:
            m = t[:, s, 3] != 0
            acc = torch.where(m[:, None], acc + t[:, s, :3], acc)
            cnt += m.cpu().numpy().astype(np.float32)
        else:
            acc = acc + t[:, s, :3]
            cnt += np.float32(1)
    with np.errstate(all="ignore"):
        scale = np.float32(1) / (cnt if task else np.full_like(cnt, np.float32(t.shape[1])))  # 1.f / 0 = inf
    return (acc * torch.from_numpy(scale).cuda()[:, None]).cpu().numpy()


def render_dev(ctx, region, task, fw=FW, fh=FH):
    """The region through spt_render_rows_async: region-local float4 pixels and the frame's
    g_data bytes (0xAB where the call wrote nothing)."""
    import torch
    yB, yE, xB, xE = region
    d = torch.zeros(((yE - yB) * (xE - xB), 4), dtype=torch.float32, device="cuda")
    g = torch.full((fw * fh * 3,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_rows_async(1 if task else 0, yB, yE, 1, 1, 0, xB, xE, d.data_ptr(), g.data_ptr())
    ctx.synchronize()
    return d.cpu().numpy(), g.cpu().numpy()


def check_region(ctx, region, spp, task, what, fw=FW, fh=FH):
    """Render the region (float4 and g_data) and its samples; compare with the definition.
    Returns the float pixels."""
    yB, yE, xB, xE = region
    got, g = render_dev(ctx, region, task, fw, fh)
    samp = ctx.render_samples(yB, yE, xB, xE, spp, task=task)
    want = fold_of_samples(samp, task)
    assert_bits(got[:, :3], want, what)
    gw = np.full(fw * fh * 3, 0xAB, np.uint8).reshape(fh, fw, 3)
    gw[fh - yE:fh - yB, xB:xE] = gamma_bytes(want).reshape(yE - yB, xE - xB, 3)[::-1]
    assert np.array_equal(g, gw.ravel()), f"{what}: g_data bytes"
    return got


def halvings_to_zero(colors):
    """code_jz (spt_scenestate.cpp): halvings after which every finite albedo, times 0.5f, is 0."""
    jz = 0
    for a in np.asarray(colors, np.float32)[:, :3].ravel():
        if not np.isfinite(a):
            continue
        x, j = np.float32(a) * np.float32(0.5), 0
        while x != 0 and j < 280:
            x, j = x * np.float32(0.5), j + 1
        jz = max(jz, j)
    return jz


# ---------------------------------------------------------------- the table fold is the sum

@pytest.mark.parametrize("task", [False, True])
@pytest.mark.parametrize("spp", [1, 8, 9, 17])
@pytest.mark.parametrize("bounces", [1, 3, 50])
def test_table_fold_is_the_in_order_sum(spt, ctx, golden_scenes, bounces, spp, task):
    setup(ctx, spt, scene_from(spt, golden_scenes, "random"), FW, FH, spp, bounces, seed=7)
    got = check_region(ctx, REGION, spp, task, f"bounces {bounces}, spp {spp}, task {task}")
    n = ctx.stats()["fold_table_entries"]
    assert n > 0, "the random scene's table fits: the fold went through it"
    assert (got[:, :3] > 0).any()
    # the table has one row of entries per j <= jmax = min(bounces - 1, jz)
    jz = halvings_to_zero(golden_scenes["random_colors"])
    ctx.set_params(FW, FH, spp, 1, 7)
    if min(bounces - 1, jz) != 0:  # jmax moved: stale until the next launched render
        assert ctx.stats()["fold_table_entries"] == 0
    render_dev(ctx, (11, 12, 15, 16), task)
    row = ctx.stats()["fold_table_entries"]
    assert row >= len(golden_scenes["random_radii"]) and n == (min(bounces - 1, jz) + 1) * row


def _mirror_glass_lattice():
    """6x6x6 lattice of fuzzy mirror and glass spheres over a diffuse ground: some paths
    need more than RenderSegmentTask's 10 passes and are dropped (key 0)."""
    pts = [[(i - 2.5), 0.2 + j, 1.5 + k, 0] for i in range(6) for j in range(6) for k in range(6)]
    c = np.float32([[0, -1000.5, 0, 0]] + pts)
    n = len(c)
    r = np.float32([1000] + [0.47] * (n - 1))
    col = np.float32([[30, 144, 255, 0]] + [[200, 100, 50, 0]] * (n - 1))
    m = np.uint8([3] + [1] * (n - 1))
    m[2::2] = 2
    fz = np.float32([0] + [0.02] * (n - 1))
    return c, r, col, m, fz


def test_task_mode_with_dropped_paths_and_an_aliased_tile(spt, ctx, oracle):
    arrays = _mirror_glass_lattice()
    spp, b, seed = 17, 8, 9
    setup(ctx, spt, spt.Scene(*arrays), 64, 64, spp, b, seed=seed)
    # square 9 x 9 tile: pixel p is colors[p]; dropped paths do not count
    ctx.reset_stats()
    check_region(ctx, (20, 29, 30, 39), spp, True, "task mode, lattice", 64, 64)
    assert ctx.stats()["fold_table_entries"] > 0
    # 5 x 3 tile: colorIndex dx + dy * 3 aliases (up to two sources per index, added within
    # a sample in the reference's order, indices without a source NaN): the CPU restatement
    # of RenderSegmentTask is the definition of that order
    gw = np.full(64 * 64 * 3, 0xAB, np.uint8)
    got, g = render_dev(ctx, (24, 27, 30, 35), True, 64, 64)
    assert ctx.stats()["dropped"] > 0
    osc = oracle.OracleScene(*arrays)
    fr = oracle.make_frame(spt.camera_basis(EYE, LOOK, UP), EYE, SKY, 64, 64, spp, b, seed)
    want, _ = oracle.render_segment(osc, fr, 24, 27, 30, 35, task=True, rgb8=gw)
    nan = np.isnan(got[:, :3]) & np.isnan(want[:, :3])
    assert nan.any() and not nan.all()
    assert_bits(np.where(nan, 0, got[:, :3]), np.where(nan, 0, want[:, :3]), "task mode, 5 x 3 tile")
    assert np.array_equal(g, gw), "5 x 3 tile: g_data bytes"


def _edge_albedo_scene(spt):
    """A dozen diffuse spheres in front of the camera over a diffuse ground; albedos 0, a
    denormal, the largest finite float, +inf and NaN among them (NaN and inf in the middle)."""
    xs, ys = [-0.9, -0.3, 0.3, 0.9], [0.4, 1.0, 1.6]
    c = np.float32([[0, -1000.5, 0, 0]] + [[x, y, 0, 0] for y in ys for x in xs])
    r = np.float32([1000] + [0.28] * 12)
    big, den = np.finfo(np.float32).max, np.float32(1e-44)
    col = np.float32([[90, 160, 40, 0],
                      [0, 0, 0, 0], [den, 3e-42, 7e-40, 0], [big, 1, big, 0], [1e-30, 200, 1e-38, 0],
                      [255, 0, den, 0], [np.nan, 50, np.nan, 0], [7, np.inf, 0.5, 0], [big, big, big, 0],
                      [den, den, den, 0], [np.inf, np.inf, np.inf, 0], [1, np.nan, 2, 0], [120, 60, 30, 0]])
    return spt.Scene(c, r, col, np.full(13, 3, np.uint8), np.zeros(13, np.float32))


@pytest.mark.parametrize("bounces", [3, 50])
def test_table_edges_zero_denormal_huge_inf_nan(spt, ctx, bounces):
    spp = 9
    setup(ctx, spt, _edge_albedo_scene(spt), 18, 18, spp, bounces, seed=3)
    got = check_region(ctx, (4, 13, 4, 13), spp, False, f"edge albedos, bounces {bounces}", 18, 18)
    assert ctx.stats()["fold_table_entries"] > 0
    assert np.isnan(got[:, :3]).any() and np.isinf(got[:, :3]).any()


# ---------------------------------------------------------------- rebuilds and the fallback

def test_table_follows_set_params_and_set_scene(spt, ctx, golden_scenes):
    def fresh(scene, b):
        c = spt.Context(0)
        try:
            setup(c, spt, scene, FW, FH, 9, b, seed=5)
            return render_dev(c, REGION, False)[0], c.stats()["fold_table_entries"]
        finally:
            c.close()

    rnd, ref = scene_from(spt, golden_scenes, "random"), scene_from(spt, golden_scenes, "reference")
    setup(ctx, spt, rnd, FW, FH, 9, 2, seed=5)
    render_dev(ctx, REGION, False)
    n2 = ctx.stats()["fold_table_entries"]
    ctx.set_params(FW, FH, 9, 50, 5)  # jmax moves: more rows
    a = render_dev(ctx, REGION, False)[0]
    assert_bits(ctx.render_segment(*REGION), a, "a batched host call (arithmetic decode) vs the table fold")
    na = ctx.stats()["fold_table_entries"]
    want, nw = fresh(rnd, 50)
    assert na == nw > n2
    assert_bits(a, want, "after set_params with another depth")
    ctx.set_scene(ref)  # another slot count
    b = render_dev(ctx, REGION, False)[0]
    nb = ctx.stats()["fold_table_entries"]
    want, nw = fresh(ref, 50)
    assert nb == nw != na
    assert_bits(b, want, "after set_scene with another scene")
    check_region(ctx, REGION, 9, False, "after set_scene: the sum")


def test_table_above_the_cap_falls_back_to_the_arithmetic_decode(spt, golden_scenes):
    """8 000 tiny spheres behind the scene, one with an albedo near FLT_MAX: jz = 277, and at
    depth 300 the table would need (jmax + 1) * slots * 16 B > 32 MiB.  No table: spt_stats
    says so, and the pixels are still the in-order sums."""
    gs = golden_scenes
    n_far, bounces, spp = 8000, 300, 9
    far = np.zeros((n_far, 4), np.float32)
    far[:, 0] = (np.arange(n_far, dtype=np.float32) - n_far / 2) * np.float32(0.01)
    far[:, 1] = np.float32(40.0)
    far[:, 2] = np.float32(200.0)
    fcol = np.full((n_far, 4), 9, np.float32)
    fcol[0, :3] = np.float32(3e38)
    c = np.concatenate([gs["random_centers"], far]).astype(np.float32)
    r = np.concatenate([gs["random_radii"], np.full(n_far, 1e-3, np.float32)]).astype(np.float32)
    col = np.concatenate([gs["random_colors"], fcol]).astype(np.float32)
    m = np.concatenate([gs["random_materials"], np.full(n_far, 3, np.uint8)]).astype(np.uint8)
    f = np.concatenate([gs["random_fuzz"], np.zeros(n_far, np.float32)]).astype(np.float32)
    jmax = min(bounces - 1, halvings_to_zero(col))
    stride = len(r)  # code_stride = the slot count >= the sphere count
    assert (jmax + 1) * stride * 16 > CAP_BYTES
    cx = spt.Context(0)
    try:
        setup(cx, spt, spt.Scene(c, r, col, m, f), FW, FH, spp, bounces, seed=7)
        got = check_region(cx, REGION, spp, False, "above the cap")
        assert cx.stats()["fold_table_entries"] == 0
        assert (got[:, :3] > 0).any()
        cx.set_params(FW, FH, spp, 50, 7)  # 50 rows of ~8 200 slots fit again
        check_region(cx, REGION, spp, False, "back under the cap")
        assert cx.stats()["fold_table_entries"] >= 50 * stride
    finally:
        cx.close()


@pytest.mark.parametrize("task", [False, True])
def test_batched_frames_fold_through_the_table_in_order(spt, ctx, golden_scenes, task):
    spp = 9
    setup(ctx, spt, scene_from(spt, golden_scenes, "random"), FW, FH, spp, 50, seed=4)
    region = (6, 22, 10, 26)  # 16 x 16
    try:
        a = render_dev(ctx, region, task)[0]
        ctx.set_workspace(16 * 16 * (8 if task else 4) * 5)  # 5 samples per batch: 5 + 4
        ctx.reset_stats()
        b = render_dev(ctx, region, task)[0]
        st = ctx.stats()
        assert st["launches"] == 2 and st["fold_table_entries"] > 0
    finally:
        ctx.set_workspace(4 << 30)
    assert_bits(b, a, "two sample batches vs one")


def test_path_queries_decode_through_the_table_or_past_it(spt, ctx, golden_scenes):
    """spt_trace_rays on a context whose launched render has built the table (depth 3): at
    depths 1 and 3 its decode pass reads the table, at depth 10 the codes pass the table and
    it decodes arithmetically; a context that never rendered has no table.  Same bits."""
    rnd = scene_from(spt, golden_scenes, "random")
    setup(ctx, spt, rnd, FW, FH, 4, 3, seed=2)
    render_dev(ctx, REGION, False)
    assert ctx.stats()["fold_table_entries"] > 0
    rng = np.random.default_rng(11)
    n = 257  # more than one block of the decode pass, not a multiple of a wave
    o = np.tile(np.float32(EYE), (n, 1))
    d = np.zeros((n, 4), np.float32)
    d[:, :3] = rng.normal(size=(n, 3)).astype(np.float32) * np.float32([1.0, 0.6, 0.3]) + np.float32([0, -0.1, 1])
    d[:, :3] /= np.linalg.norm(d[:, :3], axis=1, keepdims=True).astype(np.float32)
    fresh = spt.Context(0)
    try:
        fresh.set_scene(rnd)
        fresh.set_camera(spt.camera_basis(EYE, LOOK, UP), EYE, SKY)
        assert fresh.stats()["fold_table_entries"] == 0
        for b in (1, 3, 10):
            got, want = ctx.trace_rays(o, d, b, seed=5), fresh.trace_rays(o, d, b, seed=5)
            assert_bits(got, want, f"trace_rays at depth {b}")
            assert (got[:, :3] > 0).any()
    finally:
        fresh.close()
