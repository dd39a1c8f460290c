"""Degenerate scenes and the specular-event cap against the oracle, on every traversal path.

The scenes (tests/degenerate_scenes.py) hold what spt_set_scene lets through unchecked:
signed, zero and denormal radii, nested balls and eyes inside balls, exact distance ties
between materials, magnitudes up to 2^64, non-finite geometry, fuzz and colours, unknown
material bytes, sky colours outside 0..255, and a mirror room whose paths run into
kSpecularCap.  tests/test_degenerate_oracle.py establishes on the CPU that their traversal
tables are valid, that the odd spheres are seen and that NaN stays a small share.

Every case renders a 64 x 48 frame at 4 spp, depth 12 (spec_cap: 32 x 32, 4 spp, depth 2;
behind filler: a 32 x 24 region at 2 spp) three ways and compares with the oracle: every
sample's colour bit for bit (or NaN on both sides) and the ray count; the segment-mode and
the task-mode frame's float pixels, the g_data bytes (untouched ones included) and the
task mode's dropped count.

    path       what runs                                   proved by stats()        variants
    brute      cluster size 0: every sphere in one list    block_threads == 256     all
    auto       8-slot leaves under the 4-ary tree, the     block_threads == 256,    all
               wave's walk; primary lists where they       prim_list_blocks > 0
               build (not at 2^62, 2^64, 2^-20)
    flat4      (4, 0): flat list of 4-slot leaves          block_threads == 256     picked
    flat8      (8, 0): flat list of 8-slot leaves          (node counts: the CPU    picked
    tree2      (8, 2): binary tree                          test's spt_accel_check) picked
    tree16     (3, 16): 3 members a leaf; one level of the                          picked
               16-ary tree = a flat list at these sizes
    nolists    SPT_PRIM_LISTS=0 on the auto shape          prim_list_blocks == 0    first
    wavefront  ENGINE_WAVEFRONT on the auto shape          (set_engine succeeded)   first
    service    both frames as jobs of one service session  svc_jobs == 2            first
    lds        + 400 filler spheres: LDS lane walk         block_threads == 1024    first
    global     + 12 500: global-memory lane walk           block_threads == 256     first
    wave       + 46 000: the wave's scalar octant walk     block_threads == 256     signed_radii

"picked" = degenerate_scenes.PICKED (one or two variants a family, the most live ones; for
magnitudes the two that reach the flat list's never-cull node record), "first" = the first
of each family's picks.  spec_cap runs brute, auto, wavefront and service.  The families
run in the order signed_radii, nested, ties_mixed, sky_bytes, magnitudes, spec_cap,
nonfinite: the inputs most able to produce a bad index on the device come last.
"""
import numpy as np
import pytest

import degenerate_scenes as D
from test_gpu_parity import same_bits_or_nan, setup

pytestmark = pytest.mark.gpu

SHAPES = {"brute": (0, 0), "auto": (D.AUTO, D.AUTO), "flat4": (4, 0), "flat8": (8, 0), "tree2": (8, 2),
          "tree16": (3, 16)}


def _cases():
    out = []
    for fam in D.FAMILIES:
        vs = D.variants(fam)
        if fam == "spec_cap":
            out += [(vs[0].id, p) for p in ("brute", "auto", "wavefront", "service")]
            continue
        picked = D.PICKED[fam]
        out += [(v.id, p) for v in vs for p in ("brute", "auto")]
        out += [(vid, p) for vid in picked for p in ("flat4", "flat8", "tree2", "tree16")]
        first = picked[0]
        out += [(first, p) for p in ("nolists", "wavefront", "service", "lds", "global")]
        if first in D.WAVE_WALK:
            out.append((first, "wave"))
    return out


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


_want = {}


def oracle_side(oracle, spt, vid, walk):
    """The oracle's samples, frames and bytes of a variant (behind `walk`'s filler, its
    region and spp), computed once and shared by the paths that render it."""
    key = (vid, walk)
    if key in _want:
        return _want[key]
    v = D.by_id(vid)
    W, H, spp, depth, seed = v.frame
    arrays, region = v.arrays, (0, H, 0, W)
    if walk:
        s = spt.generate_stress(D.FILLER_SEED, D.FILLER[walk])
        arrays = D.with_filler(v, (s.centers, s.radii, s.colors, s.materials, s.fuzz))
        region, spp = D.FILLER_REGION, D.FILLER_SPP
    view = spt.camera_basis(v.eye, v.look, D.UP)
    sc = oracle.OracleScene(*arrays)
    fr = oracle.make_frame(view, v.eye, v.sky, W, H, spp, depth, seed)
    col, casts, _, _ = oracle.trace_region(sc, fr, *region)
    _, _, _, tdrop = oracle.trace_region(sc, fr, *region, task=True)
    frames = {}
    for task in (False, True):
        g = np.full(W * H * 3, 0xAB, np.uint8)
        rgba, n = oracle.render_segment(sc, fr, *region, task=task, rgb8=g)
        frames[task] = (rgba, g, n)
    assert frames[False][2] == int(casts.sum())
    _want[key] = dict(v=v, arrays=arrays, region=region, spp=spp, view=view, col=col, casts=int(casts.sum()),
                      dropped=int(tdrop.sum()), frames=frames)
    return _want[key]


@pytest.mark.parametrize("vid,path", _cases(), ids=[f"{v}-{p}" for v, p in _cases()])
def test_degenerate_scene_vs_oracle(spt, oracle, monkeypatch, vid, path):
    walk = path if path in D.FILLER else None
    w = oracle_side(oracle, spt, vid, walk)
    v, region, spp = w["v"], w["region"], w["spp"]
    W, H, _, depth, seed = v.frame
    if path == "nolists":
        monkeypatch.setenv("SPT_PRIM_LISTS", "0")
    ctx = spt.Context(0)
    try:
        if path == "wavefront":
            ctx.set_engine(spt._native.ENGINE_WAVEFRONT)
        k, b = SHAPES.get(path, SHAPES["auto"])
        ctx.set_cluster_size(k)
        ctx.set_cluster_tree(b)
        setup(ctx, spt.Scene(*w["arrays"]), W, H, spp, depth, seed=seed, view=w["view"])
        ctx.set_camera(w["view"], v.eye, v.sky)
        if path == "service":
            ctx.service_start()
        else:
            # every sample's colour, and the ray count
            ctx.reset_stats()
            samp = ctx.render_samples(*region, spp)
            st = ctx.stats()
            same_bits_or_nan(samp[:, :, :3], w["col"][:, :, :3], f"{vid} {path}: per-sample colours")
            assert st["casts"] == w["casts"], f"{vid} {path}: ray count"
            if path != "wavefront":  # the megakernel launched: 1024 threads = the LDS lane walk
                assert st["block_threads"] == (1024 if path == "lds" else 256), st["block_threads"]
            if path == "nolists":
                assert st["prim_list_blocks"] == 0
            elif path == "auto":
                assert (st["prim_list_blocks"] > 0) == (vid not in D.LISTS_OFF + D.LISTS_ALL_WALK)
        # both modes' frames: float pixels, g_data bytes, dropped paths (a service session's
        # counters arrive when it ends: read once, after service_stop)
        for task in (False, True):
            want, want8, want_casts = w["frames"][task]
            g = np.full(W * H * 3, 0xAB, np.uint8)
            if path != "service" or not task:
                ctx.reset_stats()
            got = ctx.render_segment(*region, g_data=g, task=task)
            same_bits_or_nan(got[:, :3], want[:, :3], f"{vid} {path}: frame, task={task}")
            assert np.array_equal(g, want8), f"{vid} {path}: {np.count_nonzero(g != want8)} g_data bytes differ, task={task}"
            if path == "service":
                continue
            st = ctx.stats()
            if not task:  # RenderSegmentTask casts twice per specular event (TaskBasedPathTracer.hpp:9-30)
                assert st["casts"] == want_casts, f"{vid} {path}: ray count of the frame"
            assert st["dropped"] == (w["dropped"] if task else 0), f"{vid} {path}: dropped paths, task={task}"
        if path == "service":
            ctx.service_stop()
            st = ctx.stats()
            assert st["svc_jobs"] == 2 and st["svc_running"] == 0, st
            assert st["dropped"] == w["dropped"], f"{vid} {path}: dropped paths"
    finally:
        ctx.close()
