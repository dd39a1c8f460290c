"""The megakernel's issue diet against the oracle: the sampler's even dealing of helper
lanes (coop_ball_vector), glibc-powf's coefficients formed at their use (spt_powf.h) and
the parked paths' rows addressed from the lane's own row (render_body) change no result.  Per-sample colours and ray counts (spt_render_samples),
both modes' frames, g_data bytes and dropped paths, on the megakernel, the wavefront
engine, jobs of the render service and a 2-rank split into interleaved 4-row strips
(rehearsed on one GPU), for

  c2        the config-2 scene at 64 x 40, 8 spp, depth 50 (full 8x8 tiles only)
  cornell3  40 x 24, 4 spp, depth 8: fuzzy mirrors scale the sampler's vector
  ragged    43 x 21 at 3 spp: edge tiles, a last band of 5 rows, batches across samples
  rows5     a 5-row region of the 64 x 40 frame (fewer rows than a band)
  glass     config 2 seen from inside the glass ball: most paths refract (powf)

each compared bit for bit with the CPU restatement (oracle/: RenderSegment /
RenderSegmentTask, SingleThreadPathTracer.hpp:118-136, TaskBasedPathTracer.hpp:61-210)."""
import numpy as np
import pytest

from test_gpu_parity import EYE, LOOK, SKY, UP, assert_bitwise, oscene_from, scene_from

pytestmark = pytest.mark.gpu

INSIDE = ([0.0, 1.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0])  # eye inside the glass ball (tests/test_prim_lists.py)
# scene, frame (W, H, spp, depth, seed), region (yB, yE, xB, xE), (eye, look)
CASES = {
    "c2": ("random", (64, 40, 8, 50, 21), (0, 40, 0, 64), (EYE, LOOK)),
    "cornell3": ("cornell3", (40, 24, 4, 8, 22), (0, 24, 0, 40), (EYE, LOOK)),
    "ragged": ("random", (43, 21, 3, 50, 23), (0, 21, 0, 43), (EYE, LOOK)),
    "rows5": ("random", (64, 40, 8, 50, 24), (17, 22, 0, 64), (EYE, LOOK)),
    "glass": ("random", (64, 40, 8, 50, 25), (0, 40, 0, 64), INSIDE),
}
PATHS = ("megakernel", "wavefront", "service", "strips")


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


_want = {}


def oracle_side(oracle, spt, golden_scenes, case):
    """The oracle's samples, frames, bytes and counts of a case, computed once and shared by
    the paths that render it."""
    if case in _want:
        return _want[case]
    name, (W, H, spp, depth, seed), region, (eye, look) = CASES[case]
    view = spt.camera_basis(eye, look, UP)
    sc = oscene_from(oracle, golden_scenes, name)
    fr = oracle.make_frame(view, eye, SKY, W, H, spp, depth, seed)
    col, casts, _, _ = oracle.trace_region(sc, fr, *region)
    _, _, _, tdrop = oracle.trace_region(sc, fr, *region, task=True)
    frames = {}
    for task in (False, True):
        g = np.full(W * H * 3, 0xAB, np.uint8)
        rgba, n = oracle.render_segment(sc, fr, *region, task=task, rgb8=g)
        frames[task] = (rgba, g, n)
    assert frames[False][2] == int(casts.sum())
    _want[case] = dict(view=view, eye=eye, col=col, casts=int(casts.sum()), dropped=int(tdrop.sum()), frames=frames)
    return _want[case]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", list(CASES))
def test_issue_diet_vs_oracle(spt, oracle, golden_scenes, case, path):
    import torch
    w = oracle_side(oracle, spt, golden_scenes, case)
    name, (W, H, spp, depth, seed), region, _ = CASES[case]
    yB, yE, xB, xE = region
    ctx = spt.Context(0)
    try:
        if path == "wavefront":
            ctx.set_engine(spt._native.ENGINE_WAVEFRONT)
        ctx.set_scene(scene_from(spt, golden_scenes, name))
        ctx.set_camera(w["view"], w["eye"], SKY)
        ctx.set_params(W, H, spp, depth, seed)
        if path == "strips":
            # two ranks' shares of interleaved 4-row strips (an 8x8 tile of a share spans two
            # strips), assembled: the frame and bytes of the whole region, and its rays
            parts, strip = 2, 4
            rows = [spt.rows_count(yB, yE, strip, parts, p) for p in range(parts)]
            mr = max(rows)
            tiles = torch.zeros((parts, mr * (xE - xB), 4), dtype=torch.float32, device="cuda")
            ctx.reset_stats()
            for p in range(parts):
                if rows[p]:
                    ctx.render_rows_async(0, yB, yE, strip, parts, p, xB, xE, tiles[p].data_ptr(), 0)
            frame = torch.zeros(((yE - yB) * (xE - xB), 4), dtype=torch.float32, device="cuda")
            g = torch.full((W * H * 3,), 0xAB, dtype=torch.uint8, device="cuda")
            ctx.assemble_rows_async(tiles.data_ptr(), mr, yB, yE, strip, parts, xB, xE, frame.data_ptr(), g.data_ptr())
            ctx.synchronize()
            want, want8, want_casts = w["frames"][False]
            assert_bitwise(frame.cpu().numpy()[:, :3], want[:, :3], f"{case} strips: frame")
            assert np.array_equal(g.cpu().numpy(), want8), f"{case} strips: g_data bytes"
            st = ctx.stats()
            assert st["casts"] == want_casts and st["dropped"] == 0, f"{case} strips: ray and dropped counts"
            return
        if path == "service":
            ctx.service_start()
        else:
            ctx.reset_stats()
            samp = ctx.render_samples(*region, spp)
            st = ctx.stats()
            assert_bitwise(samp[:, :, :3], w["col"][:, :, :3], f"{case} {path}: per-sample colours")
            assert st["casts"] == w["casts"], f"{case} {path}: ray count"
        # both modes' frames: float pixels, g_data bytes, dropped paths (a service session's
        # counters arrive when it ends: read once, after service_stop)
        for task in (False, True):
            want, want8, want_casts = w["frames"][task]
            g = np.full(W * H * 3, 0xAB, np.uint8)
            if path != "service" or not task:
                ctx.reset_stats()
            got = ctx.render_segment(*region, g_data=g, task=task)
            assert_bitwise(got[:, :3], want[:, :3], f"{case} {path}: frame, task={task}")
            assert np.array_equal(g, want8), f"{case} {path}: {np.count_nonzero(g != want8)} g_data bytes differ, task={task}"
            if path == "service":
                continue
            st = ctx.stats()
            if not task:  # RenderSegmentTask casts twice per specular event (TaskBasedPathTracer.hpp:9-30)
                assert st["casts"] == want_casts, f"{case} {path}: ray count of the frame"
            assert st["dropped"] == (w["dropped"] if task else 0), f"{case} {path}: dropped paths, task={task}"
        if path == "service":
            ctx.service_stop()
            st = ctx.stats()
            assert st["svc_jobs"] == 2 and st["svc_running"] == 0, st
            assert st["dropped"] == w["dropped"], f"{case} service: dropped paths"
    finally:
        ctx.close()
