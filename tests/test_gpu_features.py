"""Feature buffers (spt_render_features, spt_render_features_async) against the oracle, bit
for bit: per pixel the first-hit albedo, coverage, normal and depth averaged over the
frame's own jittered primary rays, and sample 0's sphere.

What the buffers must hold comes from tests/features.py (numpy + pyoracle, no device).
Unless stated the scene is the golden `random` (149 spheres) seen through
golden_scenes["view"] from the eye [0, 1, -3], seed 3, depth 8.  Every test asserts on the
oracle's answers that its case is live (hits and sky, partly covered pixels, every
material, sums that depend on the sample order) before it compares anything.

    1  45 x 37 at 7 spp, whole frame, on the six culling shapes      ragged tiles, sum order
    2  37 x 45 x 7, 64 x 40 x 5, 24 x 16 x 1 (ids == id_buffer())   other aspects and spp
    3  an unaligned sub-rectangle; the row map on a caller's stream  regions, interleaved rows
    4  candidate lists on and off (SPT_PRIM_LISTS=0)                 both casts
    5  unknown material bytes                                       albedo's rule vs geometry
    6  400 / 12 500 / 46 000-sphere stress scenes                    LDS, global, wave walks
    7  1024 x 1024 at 1 spp against 16 bands of 64 rows              more tiles than waves
       1024 x 1024 at 2100 spp against its two halves               more than 2^31 samples a call
    8  non-finite geometry                                          NaN by position
    9  a render, features, the same render (launched / service)     non-interference
       set_camera right behind an async call on a caller's stream   setters wait for the lists' readers
    10 state and argument errors
"""
import ctypes

import numpy as np
import pytest

import degenerate_scenes as D
from features import expected_features
from test_gpu_cast import COUNTERS, RANDOM_SHAPES, STRESS, STRESS_SEED, WALK_NODES, _case_id, accel_nodes
from test_gpu_parity import EYE, LOOK, UP, SKY, bits, scene_from, setup

pytestmark = pytest.mark.gpu

SEED, DEPTH = 3, 8
W1, H1, S1 = 45, 37, 7  # test 1's frame: 6 x 5 tiles, ragged right (5 columns) and bottom (5 rows)


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


# ---------------------------------------------------------------- the oracle's side

_want = {}


def want_random(oracle, spt, golden_scenes, W, H, spp, region=None, materials=None):
    """The helper's answer for the golden scene's frame (optionally with other material
    bytes), computed once and shared."""
    region = region or (0, H, 0, W)
    key = (W, H, spp, region, None if materials is None else bytes(materials))
    if key not in _want:
        s = scene_from(spt, golden_scenes, "random")
        if materials is not None:
            s = spt.Scene(s.centers, s.radii, s.colors, materials, s.fuzz)
        osc = oracle.OracleScene(s.centers, s.radii, s.colors, s.materials, s.fuzz)
        fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W, H, spp, DEPTH, SEED)
        w = expected_features(oracle, osc, fr, s, region)
        w["scene"] = s
        _want[key] = w
    return _want[key]


def liveness(w, n):
    """Figures of a helper answer: hit share, partly covered pixels, all-sky pixels, the
    materials hit, distinct ids, pixels whose depth sum depends on the sample order."""
    hit = w["idx"] < n
    cov = w["feat"][:, 0, 3]
    dep = w["vals"][:, :, 7]
    fwd, rev = np.zeros(len(dep), np.float32), np.zeros(len(dep), np.float32)
    for s in range(dep.shape[1]):
        fwd = fwd + dep[:, s]
        rev = rev + dep[:, dep.shape[1] - 1 - s]
    return dict(hits=float(hit.mean()), partial=int(((cov > 0) & (cov < 1)).sum()), sky=int((~hit).all(axis=1).sum()),
                materials=sorted(set(w["mat"][hit].tolist())), ids=len(np.unique(w["ids"])),
                order=int((bits(fwd) != bits(rev)).sum()))


def want_frame1(oracle, spt, golden_scenes):
    w = want_random(oracle, spt, golden_scenes, W1, H1, S1)
    if "live" not in w:
        fig = liveness(w, w["scene"].n)
        print(f"features 45x37x7: {fig}")
        # the oracle's figures: 0.82, 130, 240, [1, 2, 3], 57 ids, 260
        assert 0.5 <= fig["hits"] <= 0.95, fig
        assert fig["partial"] >= 50 and fig["sky"] >= 100, fig
        assert fig["materials"] == [1, 2, 3], fig
        assert fig["order"] >= 1, fig
        w["live"] = fig
    return w


def check(feat, ids, w, what, nan=False):
    """feat on bits (NaN matching NaN by position with nan=True) and ids."""
    if ids is not None:
        bad = np.nonzero(ids != w["ids"])[0]
        assert bad.size == 0, f"{what}: {bad.size} ids differ; first pixel {bad[0]}: got {ids[bad[0]]}, want {w['ids'][bad[0]]}"
    if feat is None:
        return
    assert feat.shape == w["feat"].shape and feat.dtype == np.float32, what
    g, e = bits(feat).reshape(-1, 8), bits(w["feat"]).reshape(-1, 8)
    differ = g != e
    if nan:
        gn, en = np.isnan(feat).reshape(-1, 8), np.isnan(w["feat"]).reshape(-1, 8)
        assert np.array_equal(gn, en), f"{what}: NaN in other lanes"
        assert np.array_equal(feat, w["feat"], equal_nan=True), what
        differ &= ~en
    bad = np.nonzero(differ.any(axis=1))[0]
    if bad.size:
        names = ("alb.r", "alb.g", "alb.b", "cov", "nrm.x", "nrm.y", "nrm.z", "dep")
        p = bad[0]
        col = int(np.nonzero(differ[p])[0][0])
        raise AssertionError(f"{what}: {bad.size} of {len(g)} pixels differ; first pixel {p} {names[col]}: "
                             f"got {feat.reshape(-1, 8)[p, col]!r}, want {w['feat'].reshape(-1, 8)[p, col]!r}")


def make_ctx(spt, golden_scenes, W, H, spp, shape=(D.AUTO, D.AUTO), scene=None):
    ctx = spt.Context(0)
    ctx.set_cluster_size(shape[0])
    ctx.set_cluster_tree(shape[1])
    setup(ctx, scene or scene_from(spt, golden_scenes, "random"), W, H, spp, DEPTH, seed=SEED, view=golden_scenes["view"])
    return ctx


# ---------------------------------------------------------------- 1, 2: whole frames

@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=[_case_id(("random", s)) for s in RANDOM_SHAPES])
def test_ragged_frame_on_every_culling_shape(spt, oracle, golden_scenes, shape):
    w = want_frame1(oracle, spt, golden_scenes)
    ctx = make_ctx(spt, golden_scenes, W1, H1, S1, shape)
    try:
        feat, ids = ctx.render_features(0, H1, 0, W1, ids=True)
        check(feat, ids, w, f"45x37x7 on {shape}")
        assert np.array_equal(bits(ctx.render_features(0, H1, 0, W1)), bits(feat)), "feat alone"
        fb = ctx.feature_buffers()
        assert fb["albedo"].shape == (H1, W1, 3) and fb["normal"].shape == (H1, W1, 3)
        assert fb["coverage"].shape == fb["depth"].shape == fb["ids"].shape == (H1, W1)
        assert fb["ids"].dtype == np.uint32 and np.array_equal(fb["ids"].ravel(), ids)
        f4 = feat.reshape(H1, W1, 2, 4)
        for name, got in (("albedo", f4[:, :, 0, :3]), ("coverage", f4[:, :, 0, 3]), ("normal", f4[:, :, 1, :3]),
                          ("depth", f4[:, :, 1, 3])):
            assert np.array_equal(bits(fb[name]), bits(got)), name
    finally:
        ctx.close()


@pytest.mark.parametrize("frame", [(37, 45, 7), (64, 40, 5), (24, 16, 1)], ids=lambda f: "x".join(map(str, f)))
def test_other_aspects_and_sample_counts(spt, oracle, golden_scenes, frame):
    W, H, spp = frame
    w = want_random(oracle, spt, golden_scenes, W, H, spp)
    fig = liveness(w, w["scene"].n)
    print(f"features {W}x{H}x{spp}: {fig}")
    # the oracle's figures: hit share 0.54 / 0.91, 101 / 89 partly covered pixels
    assert 0.2 <= fig["hits"] < 1.0 and fig["ids"] >= 3, fig
    if spp > 1:
        assert fig["partial"] >= 20, fig
    ctx = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        feat, ids = ctx.render_features(0, H, 0, W, ids=True)
        check(feat, ids, w, f"{W}x{H}x{spp}")
        if spp == 1:
            # the buffers are the single sample's values (as values: +0 + -0 is +0), the ids id_buffer's
            assert np.array_equal(feat, w["vals"][:, 0].reshape(-1, 2, 4))
            assert np.array_equal(ctx.id_buffer().ravel(), ids)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3: regions and the row map

def test_sub_rectangle_and_row_map(spt, oracle, golden_scenes):
    import torch
    w = want_frame1(oracle, spt, golden_scenes)
    want_f, want_i = w["feat"].reshape(H1, W1, 2, 4), w["ids"].reshape(H1, W1)
    ctx = make_ctx(spt, golden_scenes, W1, H1, S1)
    try:
        yB, yE, xB, xE = 3, 29, 5, 38
        feat, ids = ctx.render_features(yB, yE, xB, xE, ids=True)
        cut = dict(feat=np.ascontiguousarray(want_f[yB:yE, xB:xE]).reshape(-1, 2, 4),
                   ids=np.ascontiguousarray(want_i[yB:yE, xB:xE]).ravel())
        check(feat, ids, cut, "region y 3..29, x 5..38")
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(device=dev)
        for strip, parts in ((4, 2), (1, 3)):
            got_f = np.full((H1, W1, 2, 4), -1.0, np.float32)
            got_i = np.full((H1, W1), 0xABABABAB, np.uint32)
            for part in range(parts):
                ys = [y for y in range(H1) if (y // strip) % parts == part]
                assert spt.rows_count(0, H1, strip, parts, part) == len(ys)
                tf = torch.full((len(ys) * W1, 2, 4), -1.0, dtype=torch.float32, device=dev)
                ti = torch.full((len(ys) * W1,), 0x2B2B2B2B, dtype=torch.int32, device=dev)
                tf2, ti2 = tf.clone(), ti.clone()
                stream.wait_stream(torch.cuda.current_stream(dev))
                ctx.render_features_async(0, H1, strip, parts, part, 0, W1, tf.data_ptr(), ti.data_ptr(), stream.cuda_stream)
                # one output alone
                ctx.render_features_async(0, H1, strip, parts, part, 0, W1, tf2.data_ptr(), 0, stream.cuda_stream)
                ctx.render_features_async(0, H1, strip, parts, part, 0, W1, 0, ti2.data_ptr(), stream.cuda_stream)
                stream.synchronize()
                got_f[ys] = tf.cpu().numpy().reshape(len(ys), W1, 2, 4)
                got_i[ys] = ti.cpu().numpy().view(np.uint32).reshape(len(ys), W1)
                assert np.array_equal(bits(tf2.cpu().numpy()), bits(tf.cpu().numpy())), "d_feat only"
                assert np.array_equal(ti2.cpu().numpy(), ti.cpu().numpy()), "d_ids only"
            check(got_f.reshape(-1, 2, 4), got_i.ravel(), w, f"strip {strip}, {parts} parts")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4: candidate lists on and off

@pytest.mark.parametrize("lists", [True, False], ids=["lists", "nolists"])
def test_candidate_lists_on_and_off(spt, oracle, golden_scenes, monkeypatch, lists):
    w = want_frame1(oracle, spt, golden_scenes)
    if not lists:
        monkeypatch.setenv("SPT_PRIM_LISTS", "0")
    ctx = make_ctx(spt, golden_scenes, W1, H1, S1)
    try:
        blocks = ctx.stats()["prim_list_blocks"]
        assert (blocks > 0) == lists, blocks
        feat, ids = ctx.render_features(0, H1, 0, W1, ids=True)
        check(feat, ids, w, f"lists {lists}")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5: albedo's material rule

def test_unknown_material_bytes_are_sky_for_albedo_only(spt, oracle, golden_scenes):
    w1 = want_frame1(oracle, spt, golden_scenes)
    mats = w1["scene"].materials.copy()
    third = np.arange(0, len(mats), 3)
    mats[third] = np.where(np.arange(len(third)) % 2 == 0, 0, 200).astype(np.uint8)
    w = want_random(oracle, spt, golden_scenes, W1, H1, S1, materials=mats)
    # geometry, and so every winner, is unchanged
    assert np.array_equal(w["idx"], w1["idx"])
    assert np.array_equal(bits(w["feat"][:, 1]), bits(w1["feat"][:, 1]))
    assert np.array_equal(bits(w["feat"][:, 0, 3]), bits(w1["feat"][:, 0, 3]))
    moved = int((bits(w["feat"][:, 0, :3]) != bits(w1["feat"][:, 0, :3])).any(axis=1).sum())
    assert moved >= 20, moved
    ctx = make_ctx(spt, golden_scenes, W1, H1, S1, scene=w["scene"])
    try:
        feat, ids = ctx.render_features(0, H1, 0, W1, ids=True)
        check(feat, ids, w, "unknown material bytes")
        assert np.array_equal(ids, w1["ids"])
        assert np.array_equal(bits(feat[:, 1]), bits(w1["feat"][:, 1])), "normal / depth"
        assert np.array_equal(bits(feat[:, 0, 3]), bits(w1["feat"][:, 0, 3])), "coverage"
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6: the other walks

@pytest.mark.parametrize("walk", list(STRESS), ids=list(STRESS))
def test_the_other_walks(spt, oracle, walk):
    """generate_stress(2, n) through the default camera from the default eye: the oracle's
    answers meet the liveness conditions there, so the eye did not move."""
    W, H, spp, region = 64, 48, 2, (12, 36, 16, 48)
    s = spt.generate_stress(STRESS_SEED, STRESS[walk])
    lo, hi = WALK_NODES[walk]
    nodes = accel_nodes(spt, s, D.AUTO, D.AUTO)
    assert lo <= nodes <= hi, f"{walk}: {nodes} tree nodes leave the walk's range [{lo}, {hi}]"
    view = spt.camera_basis(EYE, LOOK, UP)
    osc = oracle.OracleScene(s.centers, s.radii, s.colors, s.materials, s.fuzz)
    fr = oracle.make_frame(view, EYE, SKY, W, H, spp, DEPTH, SEED)
    w = expected_features(oracle, osc, fr, s, region)
    fig = liveness(w, s.n)
    print(f"features {walk}: {fig}")
    assert 0.2 <= fig["hits"] < 1.0 and fig["ids"] >= 3, fig
    ctx = spt.Context(0)
    try:
        setup(ctx, s, W, H, spp, DEPTH, seed=SEED)
        feat, ids = ctx.render_features(*region, ids=True)
        check(feat, ids, w, walk)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7: more tiles than resident waves

def test_more_tiles_than_resident_waves(spt, oracle, golden_scenes):
    W = H = 1024
    ctx = make_ctx(spt, golden_scenes, W, H, 1)
    try:
        feat, ids = ctx.render_features(0, H, 0, W, ids=True)
        for b in range(16):
            bf, bi = ctx.render_features(64 * b, 64 * b + 64, 0, W, ids=True)
            sl = slice(64 * b * W, (64 * b + 64) * W)
            assert np.array_equal(bits(bf), bits(feat[sl])), f"band {b}: feat"
            assert np.array_equal(bi, ids[sl]), f"band {b}: ids"
        w = want_random(oracle, spt, golden_scenes, W, H, 1, region=(0, 64, 0, W))
        check(feat[:64 * W], ids[:64 * W], w, "rows 0..63 of 1024x1024")
        # (those rows see the ground alone; the whole frame sees spheres and the sky)
        assert len(np.unique(ids)) >= 3 and (ids == w["scene"].n).any()
    finally:
        ctx.close()


def test_more_than_2_31_samples_are_cut_into_launches(spt, golden_scenes):
    """1024 x 1024 at 2100 spp is 2.2e9 samples, past the 2^31 items one launch indexes: the
    frame in one call (two launches inside, of 998 and 26 rows) equals its two halves
    (1.1e9 samples each, one launch each).  No oracle pass: test 7 pins the values."""
    W = H = 1024
    spp = 2100
    assert W * H * spp > (1 << 31) > W * (H // 2) * spp
    ctx = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        feat, ids = ctx.render_features(0, H, 0, W, ids=True)
        for yB in (0, H // 2):
            hf, hi = ctx.render_features(yB, yB + H // 2, 0, W, ids=True)
            sl = slice(yB * W, (yB + H // 2) * W)
            assert np.array_equal(bits(hf), bits(feat[sl])), f"rows from {yB}: feat"
            assert np.array_equal(hi, ids[sl]), f"rows from {yB}: ids"
        cov = feat[:, 0, 3]
        assert ((cov > 0) & (cov < 1)).sum() > 1000 and len(np.unique(ids)) >= 3
    finally:
        ctx.close()


# ---------------------------------------------------------------- 8: non-finite geometry

def test_nonfinite_geometry(spt, oracle):
    v = D.variants("nonfinite")[0]
    W, H, _, depth, seed = v.frame
    spp = 2
    s = spt.Scene(*v.arrays)
    view = spt.camera_basis(v.eye, v.look, D.UP)
    osc = oracle.OracleScene(*v.arrays)
    fr = oracle.make_frame(view, v.eye, v.sky, W, H, spp, depth, seed)
    w = expected_features(oracle, osc, fr, s, (0, H, 0, W))
    fig = liveness(w, s.n)
    assert 0.0 < fig["hits"] < 1.0 and fig["ids"] >= 3, fig
    ctx = spt.Context(0)
    try:
        ctx.set_scene(s)
        ctx.set_camera(view, v.eye, v.sky)
        ctx.set_params(W, H, spp, depth, seed)
        feat, ids = ctx.render_features(0, H, 0, W, ids=True)
        check(feat, ids, w, v.id, nan=True)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 9: non-interference

@pytest.mark.parametrize("service", [False, True], ids=["launched", "service"])
def test_features_leave_renders_and_stats_alone(spt, oracle, golden_scenes, service):
    W, H, spp = 64, 40, 4
    ctx = make_ctx(spt, golden_scenes, W, H, spp)
    try:
        if service:
            ctx.service_start()
        before = ctx.render_segment(0, H, 0, W)
        if service:
            assert ctx.stats()["svc_running"] == 1
        else:
            ctx.synchronize()
        st0 = ctx.stats()
        feat, ids = ctx.render_features(0, H, 0, W, ids=True)
        st1 = ctx.stats()
        assert st1["svc_running"] == 0  # a resident session is ended by the call
        if not service:  # (a session's device counters arrive when it ends: the call ends it)
            assert {k: st0[k] for k in COUNTERS} == {k: st1[k] for k in COUNTERS}
        after = ctx.render_segment(0, H, 0, W)
        st2 = ctx.stats()
        assert np.array_equal(bits(before), bits(after))
        if service:  # the next render starts a new session
            assert st2["svc_running"] == 1 and st2["svc_sessions"] > st1["svc_sessions"]
        else:  # the counters move by the renders only
            assert st2["samples"] - st1["samples"] == W * H * spp and st2["launches"] > st1["launches"]
        f2, i2 = ctx.render_features(0, H, 0, W, ids=True)
        assert np.array_equal(bits(f2), bits(feat)) and np.array_equal(i2, ids)
        assert np.array_equal(ids, ctx.id_buffer().ravel())
        if service:
            ctx.service_stop()
    finally:
        ctx.close()


def test_setters_wait_for_features_in_flight(spt, golden_scenes):
    """The feature kernels read the primary-ray candidate lists from the caller's stream; a
    setter that rewrites the lists in place (set_camera: same frame, same capacity) must wait
    for them as it waits for renders.  1024 x 1024 at 2100 spp keeps the kernels running for
    tens of milliseconds on a non-blocking stream while set_camera moves the eye: the buffers
    must hold what the old camera sees, and the next call what the new one sees."""
    import torch
    W = H = 1024
    ctx = make_ctx(spt, golden_scenes, W, H, 2100)
    try:
        assert ctx.stats()["prim_list_blocks"] > 0
        want_f, want_i = ctx.render_features(0, H, 0, W, ids=True)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(device=dev)
        tf = torch.full((W * H, 2, 4), -1.0, dtype=torch.float32, device=dev)
        ti = torch.full((W * H,), 0x2B2B2B2B, dtype=torch.int32, device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        ctx.render_features_async(0, H, 1, 1, 0, 0, W, tf.data_ptr(), ti.data_ptr(), stream.cuda_stream)
        eye2 = [0.6, 1.3, -3.0, 0.0]
        ctx.set_camera(spt.camera_basis(eye2, LOOK, UP), eye2, SKY)  # rebuilds and re-uploads the lists
        assert stream.query(), "set_camera returned while the features kernels were in flight"
        stream.synchronize()
        assert np.array_equal(bits(tf.cpu().numpy()), bits(want_f)), "feat of the old camera"
        assert np.array_equal(ti.cpu().numpy().view(np.uint32), want_i), "ids of the old camera"
        moved_f, moved_i = ctx.render_features(0, H, 0, W, ids=True)
        assert (moved_i != want_i).mean() > 0.01
        fresh = make_ctx(spt, golden_scenes, W, H, 2100)
        try:
            fresh.set_camera(spt.camera_basis(eye2, LOOK, UP), eye2, SKY)
            ff, fi = fresh.render_features(0, H, 0, W, ids=True)
        finally:
            fresh.close()
        assert np.array_equal(bits(moved_f), bits(ff)) and np.array_equal(moved_i, fi), "the new camera"
    finally:
        ctx.close()


# ---------------------------------------------------------------- 10: errors

def test_feature_argument_and_state_errors(spt, golden_scenes):
    L = spt._native.lib()
    P = ctypes.c_void_p
    ctx = spt.Context(0)
    try:
        h = ctx.handle
        feat = np.full((8 * 4, 2, 4), -3.0, np.float32)
        ids = np.full(8 * 4, 0xABABABAB, np.uint32)
        fp, ip = feat.ctypes.data_as(P), ids.ctypes.data_as(P)

        def blocking(yB, yE, xB, xE, f=fp, i=ip):
            return L.spt_render_features(h, yB, yE, xB, xE, f, i)

        def rows(yB, yE, strip, parts, part, xB, xE, f=fp, i=ip):
            return L.spt_render_features_async(h, yB, yE, strip, parts, part, xB, xE, f, i, None)

        # SPT_ERR_STATE: no scene, no camera, no params -- one message each
        assert blocking(0, 4, 0, 8) == 2 and b"scene" in L.spt_last_error(h)
        assert rows(0, 4, 1, 1, 0, 0, 8) == 2 and b"scene" in L.spt_last_error(h)
        ctx.set_scene(scene_from(spt, golden_scenes, "random"))
        assert blocking(0, 4, 0, 8) == 2 and b"camera" in L.spt_last_error(h)
        assert rows(0, 4, 1, 1, 0, 0, 8) == 2 and b"camera" in L.spt_last_error(h)
        ctx.set_camera(golden_scenes["view"], EYE, SKY)
        assert blocking(0, 4, 0, 8) == 2 and b"params" in L.spt_last_error(h)
        assert rows(0, 4, 1, 1, 0, 0, 8) == 2 and b"params" in L.spt_last_error(h)
        ctx.set_params(32, 16, 2, 4, 1)
        # SPT_ERR_ARG, before anything is launched
        for bad in ((0, 17, 0, 8), (0, 4, 0, 33), (4, 3, 0, 8), (0, 4, 8, 7), (0, 0xFFFFFFFF, 0, 8)):
            assert blocking(*bad) == 1, bad
            assert rows(bad[0], bad[1], 1, 1, 0, bad[2], bad[3]) == 1, bad
        for strip, parts, part in ((0, 1, 0), (1, 0, 0), (1, 2, 2), (1, 1, 1)):
            assert rows(0, 4, strip, parts, part, 0, 8) == 1, (strip, parts, part)
        assert blocking(0, 4, 0, 8, None, None) == 1 and b"null" in L.spt_last_error(h)
        assert rows(0, 4, 1, 1, 0, 0, 8, None, None) == 1
        # an empty rectangle is SPT_OK and touches nothing, whatever the pointers
        for empty in ((3, 3, 0, 8), (0, 4, 5, 5), (16, 16, 32, 32)):
            assert blocking(*empty) == 0, empty
            assert blocking(*empty, None, None) == 0, empty
            assert rows(empty[0], empty[1], 1, 1, 0, empty[2], empty[3], None, None) == 0, empty
        assert (feat == -3.0).all() and (ids == 0xABABABAB).all()
        # and the same buffers are filled by a valid call: the last rows and columns
        assert blocking(12, 16, 24, 32) == 0
        assert (feat != -3.0).all() and (ids != 0xABABABAB).all()
        assert ctx.render_features(3, 3, 0, 8).shape == (0, 2, 4)
    finally:
        ctx.close()
