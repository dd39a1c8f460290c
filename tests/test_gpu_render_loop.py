"""render_body's refill and queue transitions against the oracle.

A primary batch (spt_kernels.hip render_body, PRIM) parks the wave's live paths in its LDS
queue by rank, starts 64 new paths in the lanes and leaves the survivors where they are;
idle lanes pop the queued paths at the next refill.  What can go wrong is a transition, not
the workload's size: a path parked and never popped or popped twice, a row overwritten
before it was read, a batch with fewer than 64 items, a queue that holds only own paths or
none, own paths waiting behind long survivors, the last batch finding no item, a finished
sample counted twice or not at all.

Every case renders in segment and in task mode and compares with the oracle: the float
pixels bit for bit (or NaN on both sides), the g_data bytes (untouched ones included), the
samples stats() counts, the task mode's dropped count, and the segment mode's ray count
(RenderSegmentTask casts twice per specular event, TaskBasedPathTracer.hpp:9-30, so its
own count is not the device's).

Frames: 8 x 8 x 1 spp (one batch of 64 items), 7 x 5 x 1 (fewer than 64 items in all),
9 x 7 x 2 (ragged tiles: batches under 64 lanes), 41 x 27 x 9 (tests/test_gpu_shade_flat.py's)
and 16 x 16 x 3.  Depths: 1 (every path ends inside its batch: the queue only ever holds own
paths), 2 and 50.  Scenes: config 2's; `sky`, one ball behind the eye (every primary ray
hits sky: every lane is idle after a batch); spec_cap/mirror_room at 1 spp and depth 2 (a
thousand rays a path: own paths wait in the queue behind long survivors); mixed/wall of
tests/test_gpu_shade_flat.py (every outcome of the shading step in one wave; its 690 balls
make a tree of the LDS lane walk, so it checks the wave counts without batches).  Kernels:
the plain launch; the batched launch (two render_segment calls from two threads on one
context: render_kernel_batch); the render service (three frames between service_start and
service_stop: render_kernel_svc, and render_kernel_svc_lds for the LDS trees, with the ray
count of the session as a total); and, at 16 x 16 x 2, stress
scenes whose trees go to the LDS and the global-memory lane walks, which share render_body
and have no primary batches.
Run on an MI355X with `pytest -m gpu`."""
import threading

import numpy as np
import pytest

import degenerate_scenes as D
from test_gpu_parity import same_bits_or_nan, setup
from test_gpu_shade_flat import mixed_scene

pytestmark = pytest.mark.gpu

FRAMES = ((8, 8, 1), (7, 5, 1), (9, 7, 2), (41, 27, 9), (16, 16, 3))
DEPTHS = (1, 2, 50)
CAP = "spec_cap/mirror_room"
STRESS = {"stress/lds": 400, "stress/global": 12500}  # generate_stress(2, n): the walk the tree goes to
STRESS_FRAME = (16, 16, 2)


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


def _arrays(s):
    return (s.centers, s.radii, s.colors, s.materials, s.fuzz)


def scene_of(spt, sid):
    if sid == "mixed/wall":
        return mixed_scene()
    if sid == "c2/random":
        return D.Variant("c2", "random", _arrays(spt.generate_spheres(1)))
    if sid == "sky/behind":
        # one diffuse ball behind the eye: no primary ray meets it
        return D.Variant("sky", "behind", (np.array([[0, 1, -9, 0]], np.float32), np.array([0.5], np.float32),
                                           np.array([[200, 90, 40, 0]], np.float32), np.array([D.DIFFUSE], np.uint8),
                                           np.array([0], np.float32)))
    if sid in STRESS:
        return D.Variant("stress", sid.split("/")[1], _arrays(spt.generate_stress(2, STRESS[sid])))
    return D.by_id(sid)


def _shape(sid, frame, depth):
    """The cap scene runs at 1 spp and depth 2 whatever the frame asks."""
    w, h, spp = frame
    return (w, h, 1, 2) if sid == CAP else (w, h, spp, depth)


_want = {}


def oracle_side(oracle, spt, sid, frame, depth, regions=None):
    """The oracle's frames of a case over `regions` (default: the whole frame), both modes:
    per region the float pixels and the ray count, the frame's g_data bytes, the dropped
    count.  Computed once and shared by the kernels that render the case."""
    W, H, spp, depth = _shape(sid, frame, depth)
    regions = tuple(regions or ((0, H, 0, W),))
    key = (sid, W, H, spp, depth, regions)
    if key in _want:
        return _want[key]
    v = scene_of(spt, sid)
    seed = v.frame[4]
    view = spt.camera_basis(v.eye, v.look, D.UP)
    sc = oracle.OracleScene(*v.arrays)
    fr = oracle.make_frame(view, v.eye, v.sky, W, H, spp, depth, seed)
    out = dict(v=v, W=W, H=H, spp=spp, depth=depth, seed=seed, view=view, regions=regions, samples=0, dropped=0)
    for task in (False, True):
        g = np.full(W * H * 3, 0xAB, np.uint8)
        tiles = [oracle.render_segment(sc, fr, *r, task=task, rgb8=g) for r in regions]
        out[task] = ([t[0] for t in tiles], g, sum(t[1] for t in tiles))
    for r in regions:
        out["samples"] += (r[1] - r[0]) * (r[3] - r[2]) * spp
        out["dropped"] += int(oracle.trace_region(sc, fr, *r, task=True)[3].sum())
    _want[key] = out
    return out


def make_ctx(spt, w):
    ctx = spt.Context(0)
    v = w["v"]
    setup(ctx, spt.Scene(*v.arrays), w["W"], w["H"], w["spp"], w["depth"], seed=w["seed"], view=w["view"])
    ctx.set_camera(w["view"], v.eye, v.sky)
    return ctx


def check_frame(w, task, got, g, what):
    want, want8, _ = w[task]
    for k, r in enumerate(w["regions"]):
        same_bits_or_nan(got[k][:, :3], want[k][:, :3], f"{what}: region {r}, task={task}")
    assert np.array_equal(g, want8), f"{what}: {np.count_nonzero(g != want8)} g_data bytes differ, task={task}"


def check_stats(w, task, st, what, frames=1):
    assert st["samples"] == frames * w["samples"], f"{what}: samples, task={task}"
    if not task:
        assert st["casts"] == frames * w[False][2], f"{what}: ray count"
    assert st["dropped"] == (w["dropped"] if task else 0), f"{what}: dropped paths, task={task}"


def _plain_cases():
    out = [(s, f, d) for s in ("c2/random", "sky/behind", "mixed/wall") for f in FRAMES for d in DEPTHS]
    out += [(CAP, f, 2) for f in FRAMES]
    return out + [(s, STRESS_FRAME, d) for s in STRESS for d in (1, 50)]


def _id(c):
    s, f, d = c
    return f"{s}-{f[0]}x{f[1]}x{f[2]}-d{d}"


@pytest.mark.parametrize("case", _plain_cases(), ids=_id)
def test_plain_launch_vs_oracle(spt, oracle, case):
    sid, frame, depth = case
    w = oracle_side(oracle, spt, sid, frame, depth)
    what = _id(case)
    ctx = make_ctx(spt, w)
    try:
        for task in (False, True):
            g = np.full(w["W"] * w["H"] * 3, 0xAB, np.uint8)
            ctx.reset_stats()
            got = ctx.render_segment(0, w["H"], 0, w["W"], g_data=g, task=task)
            check_frame(w, task, [got], g, what)
            st = ctx.stats()
            check_stats(w, task, st, what)
            # the kernel that ran: 1024 threads = the LDS lane walk (mixed/wall's 690 balls
            # give such a tree too: it checks render_body without batches), else 256
            assert st["block_threads"] == (1024 if sid in ("stress/lds", "mixed/wall") else 256), st["block_threads"]
    finally:
        ctx.close()


# the batched launch and the service: one case a transition, the big frame on two scenes
_SHARED = [("c2/random", (41, 27, 9), 50), ("mixed/wall", (41, 27, 9), 50), ("mixed/wall", (9, 7, 2), 2),
           ("c2/random", (8, 8, 1), 1), ("sky/behind", (16, 16, 3), 50), ("c2/random", (7, 5, 1), 50),
           (CAP, (16, 16, 3), 2), ("stress/lds", STRESS_FRAME, 50)]


@pytest.mark.parametrize("case", _SHARED, ids=_id)
def test_batched_launch_vs_oracle(spt, oracle, case):
    """Two render_segment calls from two threads on one context, the left and the right
    part of the frame: spt_batch.cpp puts concurrent calls into one render_kernel_batch
    launch (one call alone is a batch of one: the same kernel)."""
    sid, frame, depth = case
    W, H, _, _ = _shape(sid, frame, depth)
    regions = ((0, H, 0, W // 2), (0, H, W // 2, W))
    w = oracle_side(oracle, spt, sid, frame, depth, regions)
    what = _id(case) + " batched"
    ctx = make_ctx(spt, w)
    try:
        for task in (False, True):
            g = np.full(W * H * 3, 0xAB, np.uint8)
            got, errors = [None, None], []
            go = threading.Barrier(2)

            def job(k):
                try:
                    go.wait()
                    got[k] = ctx.render_segment(*regions[k], g_data=g, task=task)
                except Exception as e:  # pragma: no cover
                    errors.append(e)

            ctx.reset_stats()
            th = [threading.Thread(target=job, args=(k,)) for k in range(2)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not errors, errors
            check_frame(w, task, got, g, what)
            st = ctx.stats()
            check_stats(w, task, st, what)
            assert st["batched_calls"] == 2 and 1 <= st["batches"] <= 2 and st["launches"] == st["batches"], st
    finally:
        ctx.close()


# the service: the wave-walk kernel's scenes (render_kernel_svc) and, with LDS-tree sessions
# switched on (SPT_SVC_LDS=1, read when the context is made), the LDS lane walk's
# (render_kernel_svc_lds: stress/lds and mixed/wall)
_SERVICE = [c for c in _SHARED if c[0] != "mixed/wall" or c[1] == (41, 27, 9)] + [("c2/random", (9, 7, 2), 2)]


@pytest.mark.parametrize("case", _SERVICE, ids=_id)
def test_service_vs_oracle(spt, oracle, monkeypatch, case):
    """Three frames as jobs of one service session: segment, task, segment.  The session's
    counters arrive when it ends, so the ray count is checked as a total: twice the oracle's
    segment-mode count and the count of a plain task-mode launch of the same frame on the
    same context before the session (the device's own task-mode count, which the oracle's
    RenderSegmentTask does not give).  A session's waves add their counts at every job
    change and idle spell: a ray lost or counted twice there shows here."""
    sid, frame, depth = case
    w = oracle_side(oracle, spt, sid, frame, depth)
    what = _id(case) + " service"
    lds = sid in ("stress/lds", "mixed/wall")
    if lds:
        monkeypatch.setenv("SPT_SVC_LDS", "1")
    ctx = make_ctx(spt, w)
    try:
        ctx.reset_stats()
        g = np.full(w["W"] * w["H"] * 3, 0xAB, np.uint8)
        got = ctx.render_segment(0, w["H"], 0, w["W"], g_data=g, task=True)
        check_frame(w, True, [got], g, what + ", the plain task launch")
        st = ctx.stats()
        task_casts = st["casts"]
        assert st["svc_jobs"] == 0 and st["samples"] == w["samples"] and task_casts >= w["samples"], st
        ctx.reset_stats()
        ctx.service_start()
        for task in (False, True, False):
            g = np.full(w["W"] * w["H"] * 3, 0xAB, np.uint8)
            got = ctx.render_segment(0, w["H"], 0, w["W"], g_data=g, task=task)
            check_frame(w, task, [got], g, what)
        ctx.service_stop()
        st = ctx.stats()
        assert st["svc_jobs"] == 3 and st["svc_running"] == 0, st
        assert st["samples"] == 3 * w["samples"], f"{what}: samples"
        assert st["casts"] == 2 * w[False][2] + task_casts, f"{what}: ray count"
        assert st["dropped"] == w["dropped"], f"{what}: dropped paths"
    finally:
        ctx.close()
