"""Path queries (spt_trace_rays, spt_trace_rays_async) against the oracle, path by path, on
every traversal the render kernels have; against the render itself; and against the
reference's own recorded answers.

The paths are tests/trace_rays.make_paths': 1031 (prime: a partial last wave) of which half
are the scene's primary rays and half the adversarial cast mix of tests/cast_rays.py, each
on the reference's stream of its own 32-bit seed, traced at depths 1, 2, 10 and 50.

    case        scene, culling shape                          walk (launch_cast's rule)
    random-*    golden `random` (149 spheres) on (0,0),       brute force, flat lists of 4 / 8
                (4,0), (8,0), (8,2), (3,16), (AUTO,AUTO)      slots, the wave's tree walk
    lds         generate_stress(2, 400), AUTO                 LDS lane walk (64..2431 nodes)
    global      generate_stress(2, 12500), AUTO               global lane walk (..9000 nodes)
    wave        generate_stress(2, 46000), AUTO               wave walk (> 9000 nodes)

Every path's colour must equal spo_trace_ray's bit for bit (NaN lanes: NaN), its info
words the oracle's cast count, specular events and cut bit.  The oracle's event counts must
show the mix is live before any of that counts.
"""
import ctypes
import os

import numpy as np
import pytest

import degenerate_scenes as D
from cast_rays import make_rays
from test_gpu_cast import CASES, COUNTERS, STRESS, STRESS_SEED, WALK_NODES, _case_id, accel_nodes
from test_gpu_parity import EYE, SKY, bits, same_bits_or_nan, scene_from, setup
from trace_rays import BOUNCES, FRAME, device_info, make_paths, oracle_trace, scene_states

pytestmark = pytest.mark.gpu

SLICES = (slice(0, 1), slice(0, 63), slice(0, 64), slice(0, 65), slice(64, None))


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


def oracle_side(oracle, spt, golden_scenes, name):
    """The scene, its paths and the oracle's answers at every depth, computed once per scene
    and shared by every shape; on `random`, asserts the mix is live."""
    if name in _oracle_cache:
        return _oracle_cache[name]
    s = scene_from(spt, golden_scenes, "random") if name == "random" else spt.generate_stress(STRESS_SEED, STRESS[name])
    osc = oracle.OracleScene(s.centers, s.radii, s.colors, s.materials, s.fuzz)
    fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, FRAME[0], FRAME[1], 1, 10, 1)
    o, d, seeds = make_paths(oracle, s, fr)
    states = scene_states(seeds)
    assert [int(v) for v in states[:4]] == [oracle.scene_state(int(v)) for v in seeds[:4]]
    want = {}
    for b in BOUNCES:
        col, casts, info = oracle_trace(oracle, osc, fr, o, d, b, states)
        want[b] = (col, device_info(casts, info), info)
    if name == "random":
        # the mix is live (on the CPU: 811 paths with a diffuse event, 102 mirror, 14 glass
        # reflections, 59 refracting twice, 7 total internal reflections, 220 ending in the
        # sky; 811, 203, 7 and 0 out of bounces at depths 1, 2, 10 and 50; none cut)
        for b in BOUNCES:
            ev = {k: int((want[b][2][:, 2 + i] > 0).sum()) for i, k in enumerate(oracle.EV)}
            print(f"trace mix random, depth {b}: {ev}")
            assert ev["cut"] == 0 and not want[b][2][:, 1].any(), ev
            for k in ("diffuse", "mirror", "glass_reflect", "refract_twice", "tir", "end_sky"):
                assert ev[k] >= 5, (b, k, ev)
            if b in (1, 2, 10):
                assert ev["end_bounces"] >= 1, (b, ev)
    _oracle_cache[name] = dict(scene=s, osc=osc, fr=fr, o=o, d=d, seeds=seeds, states=states, want=want)
    return _oracle_cache[name]


def check_paths(got, got_info, want_col, want_info, what):
    assert got.shape == want_col.shape and got.dtype == np.float32
    same_bits_or_nan(got[:, :3], want_col[:, :3], f"{what}: colours")
    assert not bits(got[:, 3]).any(), f"{what}: w lanes are not +0"
    if got_info is not None:
        bad = np.nonzero((got_info != want_info).any(axis=1))[0]
        assert bad.size == 0, (f"{what}: {bad.size} of {len(want_info)} info records differ; first path {bad[0]}: "
                               f"got {got_info[bad[0]]}, want {want_info[bad[0]]}")


def trace_ctx(spt, scene, view, k=D.AUTO, b=D.AUTO, eye=EYE, sky=SKY):
    """A context with scene and camera, no params: all a trace needs."""
    ctx = spt.Context(0)
    ctx.set_cluster_size(k)
    ctx.set_cluster_tree(b)
    ctx.set_scene(scene)
    ctx.set_camera(view, eye, sky)
    return ctx


# ---------------------------------------------------------------- 1, 2: oracle parity on every walk

@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_trace_rays_match_the_oracle(spt, oracle, golden_scenes, case):
    name, (k, b) = case
    w = oracle_side(oracle, spt, golden_scenes, name)
    s, o, d, states = w["scene"], w["o"], w["d"], w["states"]
    if name in WALK_NODES:
        lo, hi = WALK_NODES[name]
        nodes = accel_nodes(spt, s, k, b)
        assert lo <= nodes <= hi, f"{name}: {nodes} tree nodes leave the walk's range [{lo}, {hi}]"
    ctx = trace_ctx(spt, s, golden_scenes["view"], k, b)
    try:
        for depth in BOUNCES:
            col, inf, _ = w["want"][depth]
            got, got_info = ctx.trace_rays(o, d, depth, states=states, info=True)
            check_paths(got, got_info, col, inf, f"depth {depth}")
        # (n, 3) arrays, colours only
        got = ctx.trace_rays(o[:, :3], d[:, :3], 10, states=states)
        check_paths(got, None, w["want"][10][0], None, "(n, 3) arrays")
        if name == "random" and (k, b) == (D.AUTO, D.AUTO):
            # the refill's edges: batches around a wave, and one that starts inside a run
            col, inf, _ = w["want"][10]
            for sl in SLICES:
                got, got_info = ctx.trace_rays(o[sl], d[sl], 10, states=states[sl], info=True)
                check_paths(got, got_info, col[sl], inf[sl], f"paths {sl.start}:{sl.stop}")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3: long paths and the cap

def test_long_paths_and_the_specular_cap(spt, oracle):
    """The mirror room through its own frame's primary rays at its own depth: paths of over
    a thousand casts beside short ones in the same waves, and the 1024-event cap."""
    v = D.variants("spec_cap")[0]
    W, H, spp, depth, seed = v.frame
    view = oracle.camera_basis(v.eye, v.look, D.UP)
    osc = oracle.OracleScene(*v.arrays)
    fr = oracle.make_frame(view, v.eye, v.sky, W, H, spp, depth, seed)
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.ravel(), ys.ravel()], axis=1)
    d = oracle.primary_rays(fr, xy, seed)
    o = np.tile(np.float32(v.eye), (len(d), 1))
    states = scene_states(np.random.default_rng(seed).integers(0, 1 << 32, len(d), dtype=np.uint64))
    col, casts, info = oracle_trace(oracle, osc, fr, o, d, depth, states)
    cut = info[:, 1] != 0
    assert cut.any() and (~cut).any() and (info[~cut, 0] > 512).any(), (int(cut.sum()), int(info[~cut, 0].max()))
    assert casts.max() > 1024  # (a cut path: 1025 specular events, a cast before each)
    assert not bits(col[cut, :3]).any()  # a cut path is black
    ctx = trace_ctx(spt, spt.Scene(*v.arrays), view, eye=v.eye, sky=v.sky)
    try:
        got, got_info = ctx.trace_rays(o, d, depth, states=states, info=True)
        check_paths(got, got_info, col, device_info(casts, info), "mirror room")
        assert np.array_equal(got_info[:, 1] >> 31 != 0, cut)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4: the render, no oracle

def test_trace_rays_equal_the_render_sample_by_sample(spt, golden_scenes):
    """Tracing a render's own primary rays on its own keyed streams, two draws in, gives
    the render's samples: no oracle in the chain."""
    W, H, spp, depth, seed = 64, 48, 4, 10, 12345
    ctx = spt.Context(0)
    try:
        setup(ctx, scene_from(spt, golden_scenes, "random"), W, H, spp, depth, seed=seed, view=golden_scenes["view"])
        want = ctx.render_samples(0, H, 0, W, spp)  # (pixel, sample, 4), SEGMENT mode
        ys, xs, ss = np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing="ij")
        xys = np.stack([xs.ravel(), ys.ravel(), ss.ravel()], axis=1).astype(np.uint32)
        _, dirs = ctx.primary_hits(xys, dirs=True)
        states = spt.sample_state(seed, xys[:, 1] * W + xys[:, 0], xys[:, 2], 2)
        eye = np.tile(np.float32(EYE), (len(xys), 1))
        got = ctx.trace_rays(eye, dirs, depth, states=states)
        assert len(np.unique(bits(want[:, :, :3]).reshape(-1, 3), axis=0)) > 100
        assert np.array_equal(bits(got[:, :3]), bits(want.reshape(-1, 4)[:, :3]))
        # states=None: ray i draws from the keyed stream of (seed, pixel i, sample 0)
        a = ctx.trace_rays(eye[:100], dirs[:100], depth, seed=7)
        b = ctx.trace_rays(eye[:100], dirs[:100], depth, states=spt.sample_state(7, np.arange(100), 0))
        assert np.array_equal(bits(a), bits(b))
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5: the reference's own answers

@pytest.mark.parametrize("shape", [(0, 0), (D.AUTO, D.AUTO)], ids=["brute", "auto"])
def test_trace_rays_match_the_reference_fixture(spt, golden_scenes, shape):
    """The oracle out of the chain: tests/golden/reference_traces.npz holds what the
    reference's own TraceAndSampleColor returns on the 1031 paths of the mix
    (tests/golden/make_reference_traces.py; checked on the CPU by
    tests/test_reference_traces.py).  Uncut paths only: the reference has no cap."""
    f = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_traces.npz"),
                     allow_pickle=False))
    ctx = trace_ctx(spt, scene_from(spt, golden_scenes, "random"), golden_scenes["view"], *shape)
    try:
        states = scene_states(f["seeds"])
        compared = 0
        for depth in BOUNCES:
            sel = np.nonzero(f["bounces"] == depth)[0]
            assert len(sel) >= 250
            got, info = ctx.trace_rays(f["o"][sel], f["d"][sel], depth, states=states[sel], info=True)
            keep = info[:, 1] >> 31 == 0
            same_bits_or_nan(got[keep, :3], f["rgba"][sel][keep, :3], f"depth {depth}")
            compared += int(keep.sum())
        assert compared == len(f["o"])  # no path of this mix is cut
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6: device pointers, streams

def test_trace_rays_async_on_two_streams(spt, oracle, golden_scenes):
    import torch
    w = oracle_side(oracle, spt, golden_scenes, "random")
    o, d, states = w["o"], w["d"], w["states"]
    n = len(o)
    ctx = trace_ctx(spt, w["scene"], golden_scenes["view"])
    try:
        want = {depth: ctx.trace_rays(o, d, depth, states=states, info=True) for depth in (2, 50)}
        dev = torch.device("cuda", 0)
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        ts = torch.from_numpy(states.view(np.int64)).to(dev)
        outs, streams = {}, {}
        torch.cuda.synchronize(dev)
        for depth in (2, 50):  # back to back, neither waits for the other
            rgba = torch.full((n, 4), -1.0, dtype=torch.float32, device=dev)
            info = torch.full((n, 2), -1, dtype=torch.int32, device=dev)
            streams[depth] = torch.cuda.Stream(device=dev)
            streams[depth].wait_stream(torch.cuda.current_stream(dev))
            outs[depth] = (rgba, info)
        for depth in (2, 50):
            rgba, info = outs[depth]
            ctx.trace_rays_async(to.data_ptr(), td.data_ptr(), ts.data_ptr(), n, depth, rgba.data_ptr(), info.data_ptr(),
                                 streams[depth].cuda_stream)
        for depth in (2, 50):
            streams[depth].synchronize()
            rgba, info = outs[depth]
            assert np.array_equal(bits(rgba.cpu().numpy()), bits(want[depth][0])), f"async colours, depth {depth}"
            assert np.array_equal(info.cpu().numpy().view(np.uint32), want[depth][1]), f"async info, depth {depth}"
        # without info, on the default stream
        rgba = torch.full((n, 4), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.trace_rays_async(to.data_ptr(), td.data_ptr(), ts.data_ptr(), n, 50, rgba.data_ptr())
        torch.cuda.synchronize(dev)
        assert np.array_equal(bits(rgba.cpu().numpy()), bits(want[50][0]))
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7: non-interference

@pytest.mark.parametrize("service", [False, True], ids=["launched", "service"])
def test_traces_leave_renders_and_stats_alone(spt, oracle, golden_scenes, service):
    W, H, spp = 64, 40, 4
    ctx = spt.Context(0)
    try:
        s = scene_from(spt, golden_scenes, "random")
        setup(ctx, s, W, H, spp, 8, seed=3, view=golden_scenes["view"])
        osc = oracle.OracleScene(s.centers, s.radii, s.colors, s.materials, s.fuzz)
        fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W, H, spp, 8, 3)
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
        col = ctx.trace_rays(o, d, 50, seed=4)  # another depth than the context's
        st1 = ctx.stats()
        assert st1["svc_running"] == 0
        if not service:  # (a session's device counters arrive when it ends: the trace ends it)
            assert {k: st0[k] for k in COUNTERS} == {k: st1[k] for k in COUNTERS}
        after = ctx.render_segment(0, H, 0, W)
        assert np.array_equal(bits(before[:, :3]), bits(want[:, :3]))
        assert np.array_equal(bits(after[:, :3]), bits(want[:, :3]))
        assert np.array_equal(bits(ctx.trace_rays(o, d, 50, seed=4)), bits(col))
        if service:
            ctx.service_stop()
    finally:
        ctx.close()


# ---------------------------------------------------------------- 8: argument errors

def test_trace_argument_errors(spt, golden_scenes):
    L = spt._native.lib()
    o = np.zeros((4, 4), np.float32)
    d = np.tile(np.float32([0, 0, 1, 0]), (4, 1))
    st = np.arange(4, dtype=np.uint64)
    ctx = spt.Context(0)
    try:
        for call in (lambda: ctx.trace_rays(o, d, 4), lambda: ctx.trace_rays_async(1, 1, 1, 4, 4, 1)):
            with pytest.raises(spt._native.SptError) as e:
                call()
            assert e.value.code == 2  # SPT_ERR_STATE: no scene
        ctx.set_scene(scene_from(spt, golden_scenes, "random"))
        with pytest.raises(spt._native.SptError) as e:
            ctx.trace_rays(o, d, 4)
        assert e.value.code == 2 and "camera" in str(e.value)  # no camera: no sky
        ctx.set_camera(golden_scenes["view"], EYE, SKY)
        assert ctx.trace_rays(o, d, 4).shape == (4, 4)  # no params needed
        with pytest.raises(spt._native.SptError) as e:
            ctx.trace_rays(o, d, 0)
        assert e.value.code == 1  # bounces = 0
        # n == 0 touches nothing, whatever the pointers; null required pointers otherwise
        P = ctypes.c_void_p
        h = ctx.handle
        assert L.spt_trace_rays(h, None, None, None, 0, 4, None, None) == 0
        assert L.spt_trace_rays_async(h, None, None, None, 0, 4, None, None, None) == 0
        rgba = np.full((4, 4), -1.0, np.float32)
        info = np.full((4, 2), 0xABABABAB, np.uint32)
        op, dp, sp, rp, ip = (a.ctypes.data_as(P) for a in (o, d, st, rgba, info))
        assert L.spt_trace_rays(h, op, dp, sp, 0, 4, rp, ip) == 0
        assert (rgba == -1.0).all() and (info == 0xABABABAB).all()
        assert len(ctx.trace_rays(o[:0], d[:0], 4)) == 0
        assert L.spt_trace_rays(h, None, dp, sp, 4, 4, rp, None) == 1
        assert L.spt_trace_rays(h, op, None, sp, 4, 4, rp, None) == 1
        assert L.spt_trace_rays(h, op, dp, None, 4, 4, rp, None) == 1
        assert L.spt_trace_rays(h, op, dp, sp, 4, 4, None, None) == 1
        assert L.spt_trace_rays_async(h, op, dp, sp, 4, 4, None, None, None) == 1
        assert b"null" in L.spt_last_error(h)
        assert L.spt_trace_rays(h, op, dp, sp, 4, 0, rp, None) == 1
        assert (rgba == -1.0).all()
        with pytest.raises(ValueError):
            ctx.trace_rays(o, d[:3], 4)
        with pytest.raises(ValueError):
            ctx.trace_rays(o, d, 4, states=st[:3])
    finally:
        ctx.close()
