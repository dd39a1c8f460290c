"""Occlusion queries (spt_occluded_rays, spt_occluded_rays_async; Context.occluded, visible,
occluded_async) against their contract, ray by ray, on every traversal the casts have.

    occ[i] = idx_i < sphere count  and  ds_i < L_i        (tests/occlusion.py: contract)

The cases, scenes, shapes and the 4099 adversarial rays are those of tests/test_gpu_cast.py
(whose oracle answers are shared, computed once per scene); the stress scenes' node counts
are asserted with spt_accel_check so that each still takes the walk it is here for.  Every
ray is dealt one of make_limits' eight classes of limit -- at, one ulp either side of, far
below and far above its own closest hit's ds, infinite, and the limits that answer 0
whatever the scene -- shuffled so that single waves mix them.  The device's bytes must equal
the contract computed two ways: from the oracle (find_closest + probe_sphere) and from the
same context's own cast_rays(hits=True).

Segments: b = o + d s with s around the closest hit's t (0.5 t, t, 1.5 t; a random length on
misses; some a == b), at scale 1.0 and 0.999, against the restated contract
(tests/occlusion.py: restate_segments) -- again from the oracle and from the context's own
casts of the restated rays.
"""
import ctypes

import numpy as np
import pytest

import degenerate_scenes as D
from cast_rays import make_rays
from occlusion import contract, make_limits, restate_segments
from test_gpu_cast import (CASES, COUNTERS, WALK_NODES, _camera_ctx, _case_id, _oracle_frame, accel_nodes, oracle_side,
                           spt)  # noqa: F401  (spt: the module's fixture)
from test_gpu_parity import bits, scene_from

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
SEGMENTS = 1
POISON = 0xAB


def raw_occluded(spt, ctx, a, b, limits, flags=0, scale=1.0):
    """spt_occluded_rays into a poisoned buffer: the bytes as the library wrote them."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    occ = np.full(len(a), POISON, np.uint8)
    lp = None if limits is None else np.ascontiguousarray(limits, np.float32).ctypes.data_as(P)
    rc = spt._native.lib().spt_occluded_rays(ctx.handle, a.ctypes.data_as(P), b.ctypes.data_as(P), lp, len(a), flags,
                                             scale, occ.ctypes.data_as(P))
    assert rc == 0, spt._native.lib().spt_last_error(ctx.handle)
    return occ


def check_bytes(got, want, what, kind=None):
    got = np.asarray(got)
    assert np.isin(got, (0, 1)).all(), f"{what}: a byte is neither 0 nor 1: {np.unique(got)}"
    bad = np.nonzero(got.astype(bool) != want)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want)} answers differ; first ray {bad[0]}"
                           + (f" (kind {kind[bad[0]]})" if kind is not None else "")
                           + f": got {got[bad[0]]}, want {int(want[bad[0]])}")


# ---------------------------------------------------------------- the oracle's side of segments

_seg_cache = {}


def segment_side(oracle, w, name):
    """The scene's segments (a, b), the restated rays and the oracle's (idx, ds) on them,
    once per scene."""
    if name in _seg_cache:
        return _seg_cache[name]
    s, osc, o, d, hit = w["scene"], w["osc"], w["o"], w["d"], w["hit"]
    n = len(o)
    rng = np.random.default_rng(31)
    t = w["want"][:, 0, 3]
    factor = np.float32([0.5, 1.0, 1.5])[rng.integers(0, 3, n)]
    with np.errstate(all="ignore"):
        length = np.where(hit, t * factor, rng.uniform(0.5, 60.0, n).astype(np.float32)).astype(np.float32)
        b = (o + d * length[:, None]).astype(np.float32)  # (n, 4), w = 0
    same = rng.random(n) < 0.02  # a == b
    b[same] = o[same]
    so, sd, L1 = restate_segments(o, b, 1.0)
    idx = np.array([oracle.find_closest(osc, sd[i], so[i]) for i in range(n)], np.uint32)
    ds = np.zeros(n, np.float32)
    for i in np.nonzero(idx < s.n)[0]:
        ds[i] = oracle.probe_sphere(osc, idx[i], sd[i], so[i])[1]
    want = contract(idx, ds, L1, s.n)
    # live: both answers, and rays on either side at each factor's class
    share = want.mean()
    print(f"segments {name}: occluded {share:.3f}, a == b {same.sum()}")
    assert 0.10 <= share <= 0.90, share  # (hits 0.7 x a third each at 0.5 t, t, 1.5 t: about 0.35)
    assert not want[same].any() and same.sum() >= 20
    _seg_cache[name] = dict(a=o, b=b, o=so, d=sd, idx=idx, ds=ds, same=same)
    return _seg_cache[name]


# ---------------------------------------------------------------- the query on every walk

@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_occluded_rays_match_the_contract(spt, oracle, golden_scenes, case):
    import torch
    name, (k, b) = case
    w = oracle_side(oracle, spt, golden_scenes, name)
    s, o, d, kind = w["scene"], w["o"], w["d"], w["kind"]
    n = len(o)
    if name in WALK_NODES:
        lo, hi = WALK_NODES[name]
        nodes = accel_nodes(spt, s, k, b)
        assert lo <= nodes <= hi, f"{name}: {nodes} tree nodes leave the walk's range [{lo}, {hi}]"
    ds = w["want"][:, 1, 3]
    L, cls = make_limits(ds, w["hit"])
    want = contract(w["idx"], ds, L, s.n)
    assert 0.25 <= want.mean() <= 0.75, want.mean()
    ctx = spt.Context(0)
    try:
        ctx.set_cluster_size(k)
        ctx.set_cluster_tree(b)
        ctx.set_scene(s)  # a scene is all the query needs
        # the context's own casts define the same answers
        idx2, hit2 = ctx.cast_rays(o, d, hits=True)
        own = contract(idx2, hit2[:, 1, 3], L, s.n)
        assert np.array_equal(own, want), "the cast's own (idx, ds) give another contract than the oracle's"
        got = raw_occluded(spt, ctx, o, d, L)
        check_bytes(got, want, "4099 mixed rays, mixed limits", kind)
        assert np.array_equal(ctx.occluded(o[:, :3], d[:, :3], L), want), "(n, 3) arrays through Context.occluded"
        # batch sizes around a wave, and the same rays sorted by kind (coherent waves)
        for m in (1, 63, 64, 65):
            check_bytes(raw_occluded(spt, ctx, o[:m], d[:m], L[:m]), want[:m], f"{m} rays", kind)
        order = np.argsort(kind, kind="stable")
        check_bytes(raw_occluded(spt, ctx, o[order], d[order], L[order]), want[order], "rays sorted by kind", kind[order])
        # unbounded, and one limit for all
        check_bytes(raw_occluded(spt, ctx, o, d, None), w["hit"], "no limits: idx < n", kind)
        assert np.array_equal(ctx.occluded(o, d), w["hit"])
        one = np.float32(np.median(ds[w["hit"]]))
        scalar = contract(w["idx"], ds, np.full(n, one, np.float32), s.n)
        assert scalar.any() and (w["hit"] & ~scalar).any()
        assert np.array_equal(ctx.occluded(o, d, one), scalar), "a scalar limit"
        # device pointers on a stream of the caller's, into a poisoned buffer
        dev = torch.device("cuda", 0)
        to, td, tl = (torch.from_numpy(x).to(dev) for x in (o, d, L))
        tocc = torch.full((n + 64,), POISON, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        ctx.occluded_async(to.data_ptr(), td.data_ptr(), tl.data_ptr(), n, tocc.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        out = tocc.cpu().numpy()
        check_bytes(out[:n], want, "async", kind)
        assert (out[n:] == POISON).all(), "async wrote past its n bytes"
        # segments, from the oracle and from this context's casts of the restated rays
        g = segment_side(oracle, w, name)
        for scale in (1.0, 0.999):
            so, sd, Ls = restate_segments(g["a"], g["b"], scale)
            seg_want = contract(g["idx"], g["ds"], Ls, s.n)
            si, sh = ctx.cast_rays(so, sd, hits=True)
            assert np.array_equal(contract(si, sh[:, 1, 3], Ls, s.n), seg_want), f"scale {scale}: own casts of the restated rays"
            check_bytes(raw_occluded(spt, ctx, g["a"], g["b"], None, SEGMENTS, scale), seg_want, f"segments, scale {scale}", kind)
            assert np.array_equal(ctx.visible(g["a"][:, :3], g["b"][:, :3], scale), ~seg_want), f"visible, scale {scale}"
        tb = torch.from_numpy(g["b"]).to(dev)
        tocc.fill_(POISON)
        ctx.occluded_async(to.data_ptr(), tb.data_ptr(), 0, n, tocc.data_ptr(), segments=True, scale=0.999,
                           stream=stream.cuda_stream)
        stream.synchronize()
        check_bytes(tocc.cpu().numpy()[:n], seg_want, "async segments", kind)
    finally:
        ctx.close()


# ---------------------------------------------------------------- non-interference

@pytest.mark.parametrize("service", [False, True], ids=["launched", "service"])
def test_occlusion_queries_leave_renders_and_stats_alone(spt, oracle, golden_scenes, service):
    W, H, spp = 64, 40, 4
    ctx, s = _camera_ctx(spt, golden_scenes, W, H, spp)
    try:
        osc, fr = _oracle_frame(oracle, golden_scenes, s, W, H, spp)
        want, _ = oracle.render_segment(osc, fr, 0, H, 0, W)
        o, d, _, _ = make_rays(s.centers, s.radii, n=1000, seed=9)
        lim = np.float32(25.0)
        if service:
            ctx.service_start()
        before = ctx.render_segment(0, H, 0, W)
        if service:
            assert ctx.stats()["svc_running"] == 1
        else:
            ctx.synchronize()
        st0 = ctx.stats()
        occ = ctx.occluded(o, d, lim)
        st1 = ctx.stats()
        assert st1["svc_running"] == 0
        if not service:  # (a session's device counters arrive when it ends: the query ends it)
            assert {k: st0[k] for k in COUNTERS} == {k: st1[k] for k in COUNTERS}
        vis = ctx.visible(o, o + d)
        after = ctx.render_segment(0, H, 0, W)
        assert np.array_equal(bits(before[:, :3]), bits(want[:, :3]))
        assert np.array_equal(bits(after[:, :3]), bits(want[:, :3]))
        assert np.array_equal(ctx.occluded(o, d, lim), occ)
        assert np.array_equal(ctx.visible(o, o + d), vis)
        assert occ.any() and not occ.all()
        if service:
            ctx.service_stop()
    finally:
        ctx.close()


# ---------------------------------------------------------------- argument errors

def test_occlusion_argument_errors(spt, golden_scenes):
    L = spt._native.lib()
    o = np.zeros((4, 4), np.float32)
    d = np.tile(np.float32([0, 0, 1, 0]), (4, 1))
    lim = np.ones(4, np.float32)
    occ = np.full(4, POISON, np.uint8)
    ctx = spt.Context(0)
    try:
        for call in (lambda: ctx.occluded(o, d), lambda: ctx.visible(o, d),
                     lambda: ctx.occluded_async(1, 1, 0, 4, 1)):
            with pytest.raises(spt._native.SptError) as e:
                call()
            assert e.value.code == 2  # SPT_ERR_STATE: no scene
        ctx.set_scene(scene_from(spt, golden_scenes, "random"))
        h = ctx.handle
        op, dp, lp, cp = (x.ctypes.data_as(P) for x in (o, d, lim, occ))
        # n == 0 touches nothing, whatever the pointers and flags
        assert L.spt_occluded_rays(h, None, None, None, 0, 0, 1.0, None) == 0
        assert L.spt_occluded_rays_async(h, None, None, None, 0, 0, 1.0, None, None) == 0
        assert len(ctx.occluded(o[:0], d[:0])) == 0 and len(ctx.visible(o[:0], d[:0])) == 0
        # unknown flag bits; limits together with segments
        for flags in (2, 4, 3, 0x80000000):
            assert L.spt_occluded_rays(h, op, dp, None, 4, flags, 1.0, cp) == 1, flags
            assert L.spt_occluded_rays_async(h, op, dp, None, 4, flags, 1.0, cp, None) == 1, flags
        assert L.spt_occluded_rays(h, op, dp, lp, 4, SEGMENTS, 1.0, cp) == 1
        assert L.spt_occluded_rays_async(h, op, dp, lp, 4, SEGMENTS, 1.0, cp, None) == 1
        # null required pointers
        for args in ((None, dp, lp, cp), (op, None, lp, cp), (op, dp, lp, None), (op, dp, None, None)):
            a_, b_, l_, c_ = args
            assert L.spt_occluded_rays(h, a_, b_, l_, 4, 0, 1.0, c_) == 1
            assert b"null" in L.spt_last_error(h)
            assert L.spt_occluded_rays_async(h, a_, b_, l_, 4, 0, 1.0, c_, None) == 1
            assert b"null" in L.spt_last_error(h)
        assert (occ == POISON).all(), "a refused call wrote an answer"
        with pytest.raises(ValueError):
            ctx.occluded(o, d[:3])
        with pytest.raises(ValueError):
            ctx.occluded(o[:, :2], d[:, :2])
        with pytest.raises(ValueError):
            ctx.occluded(o, d, lim[:3])
        with pytest.raises(ValueError):
            ctx.visible(o, d[:3])
        # and the query still answers: rays along +z from the origin, any limit
        assert ctx.occluded(o, d, lim).shape == (4,)
    finally:
        ctx.close()
