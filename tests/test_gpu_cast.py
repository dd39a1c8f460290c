"""Ray queries (spt_cast_rays, spt_cast_rays_async, spt_primary_hits) against the oracle,
ray by ray, on every traversal the render kernels have.

The culling proofs of DESIGN.md §4.4 (the line test, the expanded boxes, the member
pretest, the never-cull lanes) are otherwise checked only on the rays a camera and the
samplers happen to produce.  Here 4099 rays a scene (prime: a partial last wave and block)
are built to be adversarial, their kinds shuffled together so that single waves mix them:

    A 25%  origin on a random sphere's surface, direction in its outward or inward hemisphere
    B 20%  from the default eye toward a point within 1.2 r of a random centre
    C 20%  grazing: aimed past a sphere (r^2 > 4e-3) from 3..30 units away so that
           hh = r^2 - d2 is uniform in [0, 2e-3] -- either side of RaySphereIntersection's
           hh > 1e-3
    D 10%  origin inside such a sphere with tc uniform in [0, 2e-3] -- either side of tc > 1e-3
    E 15%  kinds A / B with the direction scaled by 0.5, 2 or 1 +- 3e-6 (the never-cull lanes)
    F  2%  a NaN, +inf, -inf or zero component in o or d
    G  8%  from high above the scene, pointing away (misses)

    case        scene, culling shape                          walk (launch_render's rule)
    random-*    golden `random` (149 spheres) on (0,0),       brute force, flat lists of 4 / 8
                (4,0), (8,0), (8,2), (3,16), (AUTO,AUTO)      slots, the wave's tree walk
    lds         generate_stress(2, 400), AUTO                 LDS lane walk (64..2431 nodes)
    global      generate_stress(2, 12500), AUTO               global lane walk (..9000 nodes)
    wave        generate_stress(2, 46000), AUTO               wave walk (> 9000 nodes)

The stress scenes' node counts are asserted with spt_accel_check, so a change of the
builder cannot silently move one to another walk.

Every ray's idx must equal pyoracle.find_closest; for hits ds equals
pyoracle.probe_sphere(...)[1] and t / P / n a float32 restatement of
ClosestContactPoint and ContactNormal bit for bit; misses are eight +0.
The oracle's answers must show the mix is live (hit share, misses, kinds C and D either
side of their thresholds) before any of that counts.
"""
import ctypes
import os

import numpy as np
import pytest

import degenerate_scenes as D
from cast_rays import N_RAYS, RAY_SEED, make_rays, restate_hits
from test_gpu_parity import EYE, LOOK, UP, SKY, bits, scene_from, setup

pytestmark = pytest.mark.gpu

STRESS_SEED = 2
# scene -> (cluster size, branching) it is cast on
RANDOM_SHAPES = ((0, 0), (4, 0), (8, 0), (8, 2), (3, 16), (D.AUTO, D.AUTO))
STRESS = {"lds": D.FILLER["lds"], "global": D.FILLER["global"], "wave": D.FILLER["wave"]}
# node counts of launch_render's rule (spt_internal.h kLdsMinNodes, kLdsNodeRecords, kGlaneMaxNodes)
WALK_NODES = {"lds": (64, 2431), "global": (2432, 9000), "wave": (9001, 1 << 30)}
CASES = [("random", s) for s in RANDOM_SHAPES] + [(w, (D.AUTO, D.AUTO)) for w in STRESS]


def _case_id(c):
    name, (k, b) = c
    f = lambda v: "auto" if v == D.AUTO else str(v)
    return f"{name}-{f(k)}-{f(b)}"


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


# ---------------------------------------------------------------- the oracle's side

_oracle_cache = {}


def scene_arrays(spt, golden_scenes, name):
    if name == "random":
        s = scene_from(spt, golden_scenes, "random")
    else:
        s = spt.generate_stress(STRESS_SEED, STRESS[name])
    return s


def oracle_side(oracle, spt, golden_scenes, name):
    """The scene, its rays and the oracle's answers, computed once per scene and shared by
    every shape and batch size; asserts the mix is live."""
    if name in _oracle_cache:
        return _oracle_cache[name]
    s = scene_arrays(spt, golden_scenes, name)
    osc = oracle.OracleScene(s.centers, s.radii, s.colors, s.materials, s.fuzz)
    o, d, kind, aim = make_rays(s.centers, s.radii)
    n = len(o)
    idx = np.array([oracle.find_closest(osc, d[i], o[i]) for i in range(n)], np.uint32)
    hit = idx < s.n
    ds = np.zeros(n, np.float32)
    for i in np.nonzero(hit)[0]:
        ds[i] = oracle.probe_sphere(osc, idx[i], d[i], o[i])[1]
    passes = np.zeros(n, bool)
    for i in np.nonzero(aim >= 0)[0]:
        passes[i] = oracle.probe_sphere(osc, aim[i], d[i], o[i])[0]
    t, P, nrm = restate_hits(s.centers, s.radii, idx[hit], o[hit], d[hit])
    want = np.zeros((n, 2, 4), np.float32)
    want[hit, 0, :3], want[hit, 0, 3] = P, t
    want[hit, 1, :3], want[hit, 1, 3] = nrm, ds[hit]
    # the mix is live: measured on the CPU 0.69-0.74 hits, >= 26% misses, kind C passing
    # 0.51-0.52 and winning 0.33-0.43, kind D passing 0.48
    frac = hit.mean()
    c, dk = kind == "C", kind == "D"
    figures = dict(hits=frac, c_pass=passes[c].mean(), c_win=(idx[c] == aim[c]).mean(), d_pass=passes[dk].mean())
    print(f"cast mix {name}: " + ", ".join(f"{k} {v:.3f}" for k, v in figures.items()))
    assert 0.5 <= frac <= 0.9, figures
    assert 1.0 - frac >= 0.10, figures
    assert 0.35 <= figures["c_pass"] <= 0.65, figures
    assert figures["c_win"] >= 0.25, figures
    assert 0.35 <= figures["d_pass"] <= 0.65, figures
    _oracle_cache[name] = dict(scene=s, osc=osc, o=o, d=d, kind=kind, aim=aim, idx=idx, hit=hit, want=want)
    return _oracle_cache[name]


def accel_nodes(spt, s, k, b):
    k, b = D.shape_for_check(k, b, s.n)
    P = ctypes.c_void_p
    nodes = ctypes.c_uint32(0)
    rc = spt._native.lib().spt_accel_check(s.centers.ctypes.data_as(P), s.radii.ctypes.data_as(P), s.n, k, b,
                                           ctypes.byref(nodes))
    assert rc == 0, spt._native.lib().spt_last_error(None)
    return nodes.value


def check_batch(got_idx, got_hit, w, sel, what):
    """idx, and the hit records bit for bit, of the rays `sel` of the scene's batch."""
    want_idx, want_hit, is_hit = w["idx"][sel], w["want"][sel], w["hit"][sel]
    bad = np.nonzero(got_idx != want_idx)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want_idx)} rays pick another sphere; first ray {bad[0]} "
                           f"(kind {w['kind'][sel][bad[0]]}): got {got_idx[bad[0]]}, want {want_idx[bad[0]]}")
    if got_hit is None:
        return
    g, e = bits(got_hit).reshape(-1, 8), bits(want_hit).reshape(-1, 8)
    assert not g[~is_hit].any(), f"{what}: a miss is not eight +0"
    names = ("Px", "Py", "Pz", "t", "nx", "ny", "nz", "ds")
    bad = np.nonzero((g != e).any(axis=1) & is_hit)[0]
    if bad.size:
        r = bad[0]
        col = int(np.nonzero(g[r] != e[r])[0][0])
        raise AssertionError(f"{what}: {bad.size} hits differ; first ray {r} (kind {w['kind'][sel][r]}) {names[col]}: "
                             f"got {got_hit.reshape(-1, 8)[r, col]!r}, want {want_hit.reshape(-1, 8)[r, col]!r}")


# ---------------------------------------------------------------- casts

@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_cast_rays_match_the_oracle(spt, oracle, golden_scenes, case):
    import torch
    name, (k, b) = case
    w = oracle_side(oracle, spt, golden_scenes, name)
    s, o, d = w["scene"], w["o"], w["d"]
    if name in WALK_NODES:
        lo, hi = WALK_NODES[name]
        nodes = accel_nodes(spt, s, k, b)
        assert lo <= nodes <= hi, f"{name}: {nodes} tree nodes leave the walk's range [{lo}, {hi}]"
    ctx = spt.Context(0)
    try:
        ctx.set_cluster_size(k)
        ctx.set_cluster_tree(b)
        ctx.set_scene(s)  # no camera, no params: a scene is all a cast needs
        every = np.arange(len(o))
        idx, hit = ctx.cast_rays(o, d, hits=True)
        check_batch(idx, hit, w, every, "4099 mixed rays")
        assert np.array_equal(ctx.cast_rays(o[:, :3], d[:, :3]), idx), "(n, 3) arrays, idx only"
        # batch sizes around a wave, and the same rays sorted by kind (coherent waves)
        for m in (1, 63, 64, 65):
            gi, gh = ctx.cast_rays(o[:m], d[:m], hits=True)
            check_batch(gi, gh, w, every[:m], f"{m} rays")
        order = np.argsort(w["kind"], kind="stable")
        gi, gh = ctx.cast_rays(o[order], d[order], hits=True)
        check_batch(gi, gh, w, order, "rays sorted by kind")
        # device pointers on a stream of the caller's
        dev = torch.device("cuda", 0)
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        ti = torch.full((len(o),), 0xABABABAB, dtype=torch.int64, device=dev).to(torch.int32)
        th = torch.full((len(o), 2, 4), -1.0, dtype=torch.float32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        ctx.cast_rays_async(to.data_ptr(), td.data_ptr(), len(o), ti.data_ptr(), th.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(ti.cpu().numpy().view(np.uint32), idx), "async idx"
        assert np.array_equal(bits(th.cpu().numpy()), bits(hit)), "async hit records"
    finally:
        ctx.close()


# ---------------------------------------------------------------- the reference's own answers

@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=[_case_id(("random", s)) for s in RANDOM_SHAPES])
def test_cast_rays_match_the_reference_fixture(spt, golden_scenes, shape):
    """The oracle out of the chain: tests/golden/reference_casts.npz holds what the
    reference's own FindClosestIntersectionSphere, ClosestContactPoint and ContactNormal
    answer on 1031 rays of the mix (make_golden.py --reference-casts; checked on the CPU
    by tests/test_reference_parity.py); the cast must equal it bit for bit."""
    f = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_casts.npz"),
                     allow_pickle=False))
    s = scene_from(spt, golden_scenes, "random")
    ctx = spt.Context(0)
    try:
        ctx.set_cluster_size(shape[0])
        ctx.set_cluster_tree(shape[1])
        ctx.set_scene(s)
        idx, hit = ctx.cast_rays(f["o"], f["d"], hits=True)
        is_hit = f["idx"] < s.n
        assert is_hit.any() and not is_hit.all()
        bad = np.nonzero(idx != f["idx"])[0]
        assert bad.size == 0, f"{bad.size} rays pick another sphere; first ray {bad[0]}: got {idx[bad[0]]}, want {f['idx'][bad[0]]}"
        g, e = bits(hit).reshape(-1, 8), bits(f["hit"]).reshape(-1, 8)
        assert not g[~is_hit].any(), "a miss is not eight +0"
        bad = np.nonzero((g != e).any(axis=1))[0]
        assert bad.size == 0, (f"{bad.size} hit records differ; first ray {bad[0]}: got {hit.reshape(-1, 8)[bad[0]]!r}, "
                               f"want {f['hit'].reshape(-1, 8)[bad[0]]!r}")
    finally:
        ctx.close()


# ---------------------------------------------------------------- primary hits

def _camera_ctx(spt, golden_scenes, W, H, spp, depth=8, seed=3):
    ctx = spt.Context(0)
    s = scene_from(spt, golden_scenes, "random")
    setup(ctx, s, W, H, spp, depth, seed=seed, view=golden_scenes["view"])
    return ctx, s


def _oracle_frame(oracle, golden_scenes, s, W, H, spp, depth=8, seed=3):
    osc = oracle.OracleScene(s.centers, s.radii, s.colors, s.materials, s.fuzz)
    return osc, oracle.make_frame(golden_scenes["view"], EYE, SKY, W, H, spp, depth, seed)


def test_primary_hits_match_the_oracle(spt, oracle, golden_scenes):
    W, H, spp = 320, 200, 8
    rng = np.random.default_rng(5)
    xys = np.stack([rng.integers(0, W, 2000), rng.integers(0, H, 2000), rng.integers(0, spp, 2000)], axis=1)
    xys = xys.astype(np.uint32)
    ctx, s = _camera_ctx(spt, golden_scenes, W, H, spp)
    try:
        osc, fr = _oracle_frame(oracle, golden_scenes, s, W, H, spp)
        want = oracle.primary_winners(osc, fr, xys)
        assert 0.2 < (want < s.n).mean() and (want == s.n).any()
        idx, hit, dirs = ctx.primary_hits(xys, hits=True, dirs=True)
        assert np.array_equal(idx, want)
        assert np.array_equal(ctx.primary_hits(xys), want)
        # the directions it reports are the rays it cast
        assert not dirs[:, 3].any()
        eye = np.tile(np.asarray(EYE, np.float32), (len(xys), 1))
        idx2, hit2 = ctx.cast_rays(eye, dirs, hits=True)
        assert np.array_equal(idx2, want)
        assert np.array_equal(bits(hit2), bits(hit))
    finally:
        ctx.close()


def test_id_buffer_is_sample_zero_of_every_pixel(spt, oracle, golden_scenes):
    W, H, spp = 64, 40, 4
    ctx, s = _camera_ctx(spt, golden_scenes, W, H, spp)
    try:
        osc, fr = _oracle_frame(oracle, golden_scenes, s, W, H, spp)
        ys, xs = np.mgrid[0:H, 0:W]
        xys = np.stack([xs.ravel(), ys.ravel(), np.zeros(W * H, np.int64)], axis=1).astype(np.uint32)
        want = oracle.primary_winners(osc, fr, xys).reshape(H, W)
        got = ctx.id_buffer()
        assert got.shape == (H, W) and got.dtype == np.uint32
        assert np.array_equal(got, want)
        assert len(np.unique(want)) > 3
    finally:
        ctx.close()


# ---------------------------------------------------------------- non-interference

COUNTERS = ("samples", "casts", "dropped", "launches", "render_ms", "fold_ms", "batches", "batched_calls",
            "svc_sessions", "svc_jobs")


@pytest.mark.parametrize("service", [False, True], ids=["launched", "service"])
def test_casts_leave_renders_and_stats_alone(spt, oracle, golden_scenes, service):
    W, H, spp = 64, 40, 4
    ctx, s = _camera_ctx(spt, golden_scenes, W, H, spp)
    try:
        osc, fr = _oracle_frame(oracle, golden_scenes, s, W, H, spp)
        want, _ = oracle.render_segment(osc, fr, 0, H, 0, W)
        o, d, _, _ = make_rays(s.centers, s.radii, n=1000, seed=9)
        if service:
            ctx.service_start()
        before = ctx.render_segment(0, H, 0, W)
        if service:
            assert ctx.stats()["svc_running"] == 1
        else:
            ctx.synchronize()
        st0 = ctx.stats()
        idx = ctx.cast_rays(o, d)
        st1 = ctx.stats()
        assert st1["svc_running"] == 0
        if not service:  # (a session's device counters arrive when it ends: the cast ends it)
            assert {k: st0[k] for k in COUNTERS} == {k: st1[k] for k in COUNTERS}
        ctx.id_buffer()
        after = ctx.render_segment(0, H, 0, W)
        assert np.array_equal(bits(before[:, :3]), bits(want[:, :3]))
        assert np.array_equal(bits(after[:, :3]), bits(want[:, :3]))
        assert np.array_equal(ctx.cast_rays(o, d), idx)
        if service:
            ctx.service_stop()
    finally:
        ctx.close()


# ---------------------------------------------------------------- argument errors

def test_cast_argument_errors(spt, golden_scenes):
    L = spt._native.lib()
    o = np.zeros((4, 4), np.float32)
    d = np.tile(np.float32([0, 0, 1, 0]), (4, 1))
    xys = np.zeros((4, 3), np.uint32)
    ctx = spt.Context(0)
    try:
        for call in (lambda: ctx.cast_rays(o, d), lambda: ctx.primary_hits(xys),
                     lambda: ctx.cast_rays_async(1, 1, 4, 1)):
            with pytest.raises(spt._native.SptError) as e:
                call()
            assert e.value.code == 2  # SPT_ERR_STATE: no scene
        s = scene_from(spt, golden_scenes, "random")
        ctx.set_scene(s)
        with pytest.raises(spt._native.SptError) as e:
            ctx.primary_hits(xys)
        assert e.value.code == 2  # no camera, no params
        ctx.set_camera(golden_scenes["view"], EYE, SKY)
        ctx.set_params(32, 16, 2, 4, 1)
        assert ctx.primary_hits(np.uint32([[31, 15, 1]])).shape == (1,)  # the last pixel's last sample
        for bad in ([32, 0, 0], [0, 16, 0], [0, 0, 2], [0xFFFFFFFF, 0, 0]):
            with pytest.raises(spt._native.SptError) as e:
                ctx.primary_hits(np.uint32([[0, 0, 0], bad]))
            assert e.value.code == 1, bad
        # n == 0 touches nothing, whatever the pointers; null required pointers otherwise
        P = ctypes.c_void_p
        h = ctx.handle
        assert L.spt_cast_rays(h, None, None, 0, None, None) == 0
        assert L.spt_cast_rays_async(h, None, None, 0, None, None, None) == 0
        assert L.spt_primary_hits(h, None, 0, None, None, None) == 0
        assert len(ctx.cast_rays(o[:0], d[:0])) == 0
        op, dp, xp = o.ctypes.data_as(P), d.ctypes.data_as(P), xys.ctypes.data_as(P)
        idx = np.zeros(4, np.uint32)
        ip = idx.ctypes.data_as(P)
        assert L.spt_cast_rays(h, op, dp, 4, None, None) == 1
        assert L.spt_cast_rays(h, None, dp, 4, ip, None) == 1
        assert L.spt_cast_rays(h, op, None, 4, ip, None) == 1
        assert L.spt_cast_rays_async(h, op, dp, 4, None, None, None) == 1
        assert L.spt_primary_hits(h, xp, 4, None, None, None) == 1
        assert L.spt_primary_hits(h, None, 4, ip, None, None) == 1
        assert b"null" in L.spt_last_error(h)
        with pytest.raises(ValueError):
            ctx.cast_rays(o, d[:3])
        with pytest.raises(ValueError):
            ctx.cast_rays(o[:, :2], d[:, :2])
    finally:
        ctx.close()
