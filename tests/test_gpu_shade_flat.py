"""The shading step's wave masks against the oracle.

shade_step_body (spt_path.h) decides a lane's outcome -- sky, first diffuse hit, a turn or
the end of the diffuse loop, mirror, glass -- as wave masks joined on the scalar unit and
picks its values by selects; finish_step branches once on the mode.  A wrong mask shows
where a wave holds several outcomes at once, and at the depths where the loop's end
decision differs: depth 1 (the loop ends at its first turn), 2 (one turn) and 50.

Every case renders a 41 x 27 frame (ragged 8 x 8 tiles) at 9 spp and compares with the
oracle: every sample's colour bit for bit (or NaN on both sides) and the ray count; the
segment-mode and the task-mode frame's float pixels, the g_data bytes (untouched ones
included), the ray count and the task mode's dropped count.

Scenes: every variant of tests/degenerate_scenes.py (the mirror room, whose paths run into
the specular cap and, in task mode, past the last pass, at 1 spp and depth 2: each of its
paths casts a thousand rays), and `mixed`, built here: two layers of small balls one to
two pixels wide, diffuse / mirror with fuzz 0 / mirror with fuzz 1 / glass in turn, with
sky between them, so that the lanes of one wave take all the outcomes in the same step:
sky, a first diffuse hit, a loop ending by miss and by bounce count, both mirrors, glass
entered and left.  (Total internal reflection needs a ray that starts inside glass: only
the degenerate scenes' nested and signed balls can give one.)
Run on an MI355X with `pytest -m gpu`."""
import numpy as np
import pytest

import degenerate_scenes as D
from test_gpu_parity import same_bits_or_nan, setup

pytestmark = pytest.mark.gpu

W, H, SPP = 41, 27, 9
DEPTHS = (1, 2, 50)
CAP = "spec_cap/mirror_room"


def mixed_scene():
    """Two layers of balls 0.6 apart (two pixels of this frame, whose view spans about 13 x 8
    units at the wall's distance), the four kinds in turn along a row and shifted by one
    from row to row; the second layer, behind the gaps of the first, keeps some loops going."""
    kinds = ((D.DIFFUSE, 0.0), (D.MIRROR, 0.0), (D.MIRROR, 1.0), (D.GLASS, 0.0))
    c, r, col, m, f = [], [], [], [], []
    for layer, (z, rad) in enumerate(((1.0, 0.17), (1.9, 0.2))):
        for iy in range(15):
            for ix in range(23):
                mat, fuzz = kinds[(ix + iy + layer) % 4]
                c.append([-4.8 + 0.6 * ix + 0.3 * layer, -5.3 + 0.6 * iy + 0.3 * layer, z + 0.05 * ((ix + 2 * iy) % 3), 0.0])
                r.append(rad)
                col.append([40.0 + 9 * ix, 230.0 - 12 * iy, 90.0 + 70 * layer, 0.0])
                m.append(mat)
                f.append(fuzz)
    return D.Variant("mixed", "wall", (np.array(c, np.float32), np.array(r, np.float32), np.array(col, np.float32),
                                       np.array(m, np.uint8), np.array(f, np.float32)))


def scene_of(sid):
    return mixed_scene() if sid == "mixed/wall" else D.by_id(sid)


def _cases():
    out = []
    for v in D.variants():
        out += [(v.id, 2)] if v.id == CAP else [(v.id, d) for d in DEPTHS]
    return out + [("mixed/wall", d) for d in DEPTHS]


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


def oracle_side(oracle, spt, sid, depth):
    v = scene_of(sid)
    spp, seed = (1 if sid == CAP else SPP), v.frame[4]
    view = spt.camera_basis(v.eye, v.look, D.UP)
    sc = oracle.OracleScene(*v.arrays)
    fr = oracle.make_frame(view, v.eye, v.sky, W, H, spp, depth, seed)
    col, casts, spec, _ = oracle.trace_region(sc, fr, 0, H, 0, W)
    _, _, _, tdrop = oracle.trace_region(sc, fr, 0, H, 0, W, task=True)
    frames = {}
    for task in (False, True):
        g = np.full(W * H * 3, 0xAB, np.uint8)
        rgba, n = oracle.render_segment(sc, fr, 0, H, 0, W, task=task, rgb8=g)
        frames[task] = (rgba, g, n)
    assert frames[False][2] == int(casts.sum())
    return dict(v=v, spp=spp, seed=seed, view=view, sc=sc, fr=fr, col=col, casts=casts, spec=spec,
                dropped=int(tdrop.sum()), frames=frames)


def test_mixed_scene_mixes_the_outcomes_inside_a_tile(spt, oracle):
    """The oracle's view of `mixed`: most 8 x 8 tiles hold primary rays of all four kinds."""
    w = oracle_side(oracle, spt, "mixed/wall", 50)
    v = w["v"]
    mats = np.append(v.arrays[3], np.uint8(D.SKYBOX))  # primary_winners: index n = no hit
    fuzz = np.append(v.arrays[4], np.float32(0))
    full = 0
    tiles = [(ty, tx) for ty in range(0, H, 8) for tx in range(0, W, 8)]
    for ty, tx in tiles:
        xys = np.array([(x, y, s) for y in range(ty, min(ty + 8, H)) for x in range(tx, min(tx + 8, W)) for s in (0, 1)],
                       np.uint32)
        win = oracle.primary_winners(w["sc"], w["fr"], xys)
        kinds = set(zip(mats[win].tolist(), (fuzz[win] > 0).tolist()))
        full += {(D.SKYBOX, False), (D.DIFFUSE, False), (D.MIRROR, False), (D.MIRROR, True), (D.GLASS, False)} <= kinds
    assert 2 * full > len(tiles), f"{full} of {len(tiles)} tiles hold all five kinds of primary hit"
    # sky at the first cast, specular events, and loops of several turns at depth 50
    assert int((w["casts"] == 1).sum()) > 0 and int((w["spec"] > 0).sum()) > 0 and int(w["casts"].max()) >= 6
    # at depth 2 a loop ends both ways: a path without specular events casts 2 rays when its
    # first turn misses and 3 when the bounce count ends it
    w2 = oracle_side(oracle, spt, "mixed/wall", 2)
    plain = w2["casts"][w2["spec"] == 0]
    assert int((plain == 2).sum()) > 0 and int((plain == 3).sum()) > 0 and int(plain.max()) == 3


@pytest.mark.parametrize("sid,depth", _cases(), ids=[f"{s}-d{d}" for s, d in _cases()])
def test_shading_step_vs_oracle(spt, oracle, sid, depth):
    w = oracle_side(oracle, spt, sid, depth)
    v, spp = w["v"], w["spp"]
    if sid == CAP:
        # the cap is reached (kSpecularCap = 1024 events), and task mode drops paths at pass 10
        assert int(w["spec"].max()) > 1024 and w["dropped"] > 0
    ctx = spt.Context(0)
    try:
        setup(ctx, spt.Scene(*v.arrays), W, H, spp, depth, seed=w["seed"], view=w["view"])
        ctx.set_camera(w["view"], v.eye, v.sky)
        ctx.reset_stats()
        samp = ctx.render_samples(0, H, 0, W, spp)
        st = ctx.stats()
        same_bits_or_nan(samp[:, :, :3], w["col"][:, :, :3], f"{sid} depth {depth}: per-sample colours")
        assert st["casts"] == int(w["casts"].sum()), f"{sid} depth {depth}: ray count"
        for task in (False, True):
            want, want8, want_casts = w["frames"][task]
            g = np.full(W * H * 3, 0xAB, np.uint8)
            ctx.reset_stats()
            got = ctx.render_segment(0, H, 0, W, g_data=g, task=task)
            same_bits_or_nan(got[:, :3], want[:, :3], f"{sid} depth {depth}: frame, task={task}")
            assert np.array_equal(g, want8), f"{sid} depth {depth}: {np.count_nonzero(g != want8)} g_data bytes differ, task={task}"
            st = ctx.stats()
            if not task:  # RenderSegmentTask casts twice per specular event (TaskBasedPathTracer.hpp:9-30)
                assert st["casts"] == want_casts, f"{sid} depth {depth}: ray count of the frame"
            assert st["dropped"] == (w["dropped"] if task else 0), f"{sid} depth {depth}: dropped paths, task={task}"
    finally:
        ctx.close()
