"""The drop-in promise itself: the reference's own Renderer.hpp and Main.cpp, unmodified,
render through the shim on the GPU, byte for byte what the context renders.

oracle/_ref/ref_dropin_main is the reference's Main.cpp as the only translation unit;
oracle/_ref/ref_dropin_driver (oracle/ref_dropin_driver.cpp) calls Renderer.hpp's functions
by name for what Main.cpp's constexpr choices never reach.  Both are built by `make -C
oracle ref` where the reference's headers are, with include/dropin in front of them, behind
null GL/GLFW/stb stand-ins (oracle/ref_app_standins/), and linked against libspt_hip.so;
tests/test_dropin_build.py checks the build.  Here they run, one fresh process per run under
a 300 s limit (pyoracle.run_dropin_main / run_dropin_driver), and the g_data that the
reference's io::SaveImage hands to stbi_write_bmp is compared with a Context configured
from the product's own producers: spt.init_spheres / spt.generate_spheres of the clock's
seed (pinned against the reference's generators by test_reference_parity.test_generators
and test_oracle_kat), camera_basis(EYE, LOOK, UP), the sky (137, 207, 240) and
set_params(1440, 1440, 100, 10, 1) -- the reference's frame, which is constexpr and cannot
be made smaller.  Bytes are compared for equality: no tolerance anywhere.

Nothing of the reference is read here, only oracle/_ref/; where the binaries are absent the
tests skip and say so.  After a child that ended by a signal, ran into its time limit or
printed HIP's illegal-access error, every later test of this module skips instead of
starting another GPU process.

Oracle figures of test_application_matches_the_oracle, measured on the CPU (InitSpheres of
seed 1, 34 pixels x 100 spp): see ORACLE_REGIONS below.
"""
import os
import time

import numpy as np
import pytest

from cast_rays import make_rays

pytestmark = pytest.mark.gpu

EYE, LOOK, UP, SKY = [0, 1, -3, 0], [0, 1, 0, 0], [0, 1, 0, 0], [137, 207, 240, 0]
MOVED_EYE = [0.6, 1.3, -3, 0]  # ref_dropin_driver frames: before the third frame
W = H = 1440
SPP, BOUNCES, SEED = 100, 10, 1  # Globals.hpp's constexpr frame; the shim's default seed
TC = 4  # min(2 * hardware threads, g_maxThreads = 4): 4 x 4 tiles of 360 x 360
CLOCK = 1  # the reading of the reference's clock: the scene generators' seed
# (yBegin, yEnd, xBegin, xEnd): the corner where four tiles meet (rows and columns 358..361),
# the frame's last rows and columns, and the `reference` scene's column of mirror, glass
# and mirror balls that test_reference_parity uses.  Measured with the oracle on the CPU:
# 27, 3 and 24 distinct byte values in the three regions (the second is plain sky), and all of
# the glass region's 900 paths have specular events (up to 16 on one path).
ORACLE_REGIONS = ((358, 362, 358, 362), (1437, 1440, 1437, 1440), (556, 559, 724, 727))
GLASS_REGION = ORACLE_REGIONS[2]
N_PICK_RAYS = 1031
FRAMES_ENVS = {"default": {}, "readahead0": {"SPT_READAHEAD": "0"}, "service": {"SPT_SERVICE": "1"}}


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


@pytest.fixture
def dropin(oracle, spt):
    if not oracle.dropin_available():
        pytest.skip("oracle/_ref/ref_dropin_main and ref_dropin_driver are not here: they are built where the "
                    "reference's headers are (make -C oracle ref)")
    if oracle.dropin_fault:
        pytest.skip(f"an earlier run faulted ({oracle.dropin_fault}): no further GPU process is started")
    return oracle


# ---------------------------------------------------------------- the expected side

_scenes, _frames, _runs = {}, {}, {}


def scene(spt, name):
    if name not in _scenes:
        _scenes[name] = spt.init_spheres(CLOCK) if name == "init" else spt.generate_spheres(CLOCK)
    return _scenes[name]


def context(spt, name, eye=EYE):
    c = spt.Context(0)
    c.set_scene(scene(spt, name))
    c.set_camera(spt.camera_basis(eye, LOOK, UP), eye, SKY)
    c.set_params(W, H, SPP, BOUNCES, SEED)
    return c


def expected(spt, name, how, eye=EYE):
    """The context's g_data, computed once and left unchanged: how = "tiles" (the 16
    RenderSegment tiles of RenderImageParallelMain) or "image" (RenderSegmentTask over the
    whole frame, RenderImage)."""
    key = (name, how, tuple(eye))
    if key not in _frames:
        c = context(spt, name, eye)
        g = np.zeros(W * H * 3, np.uint8)
        if how == "tiles":
            s = W // TC
            for j in range(TC):
                for i in range(TC):
                    c.render_segment(s * j, s * j + s, s * i, s * i + s, g)
        else:
            c.render_segment(0, H, 0, W, g, task=True)
        c.close()
        g.setflags(write=False)
        _frames[key] = g
    return _frames[key]


def run_once(key, fn):
    """One child process per key for the whole module (a failed or faulted run is kept too:
    it is not started again)."""
    if key not in _runs:
        t0 = time.perf_counter()
        _runs[key] = fn()
        run = _runs[key][0] if isinstance(_runs[key], tuple) else _runs[key]
        print(f"{key}: exit {run.returncode}, {len(run.dumps)} dump(s), {time.perf_counter() - t0:.2f} s")
    return _runs[key]


def assert_ran(run, saves, what):
    assert run.returncode == 0, f"{what}: exit status {run.returncode}\n{run.output[-2000:]}"
    assert run.saves == [("output100s10b.bmp", W, H, 3)] * saves, f"{what}: stbi_write_bmp calls {run.saves}"
    assert [d.size for d in run.dumps] == [W * H * 3] * saves, what


def assert_frame(got, want, what):
    bad = np.nonzero(got != want)[0]
    if bad.size:
        px = bad // 3
        s = W // TC
        tiles = sorted(set(zip(((H - 1 - px // W) // s).tolist(), ((px % W) // s).tolist())))
        p = int(px[0])
        raise AssertionError(f"{what}: {bad.size} bytes differ in tiles (row, col) {tiles[:16]} (of {len(tiles)}); first at "
                             f"pixel (x, y) = ({p % W}, {H - 1 - p // W}): {got[3 * p:3 * p + 3]} for {want[3 * p:3 * p + 3]}")


def region_offsets(yB, yE, xB, xE):
    """The g_data offsets of a region's bytes (IOHelpers.hpp / the tracers' index: rows from
    the end of the buffer)."""
    y, x = np.mgrid[yB:yE, xB:xE]
    first = W * H * 3 - ((W - x) * 3 + y * W * 3)
    return (first.reshape(-1, 1) + np.arange(3)).reshape(-1)


# ---------------------------------------------------------------- 1, 2, 6: the application

def main_run(oracle):
    return run_once("main", lambda: oracle.run_dropin_main(CLOCK))


def test_application_renders_like_the_context(dropin, spt, tmp_path):
    """The reference's Main.cpp: Init, Startup, MainLoop (InitSpheres, RenderImageParallel:
    16 RenderJob threads, each calling RenderSegment -- g_generationType is
    TASK_MULTI_THREAD and the names are crossed in RenderJob), SaveImage once, exit 0."""
    want = expected(spt, "init", "tiles")
    assert np.unique(want).size > 50
    run = main_run(dropin)
    assert_ran(run, 1, "ref_dropin_main")
    # the file name io::SaveImage chose is the Python mirror's
    g = spt.Globals(scene(spt, "init"), width=8, height=8, samples=SPP, bounces=BOUNCES)
    try:
        assert os.path.basename(spt.SaveImage(g, str(tmp_path))) == run.saves[0][0]
    finally:
        g.ctx.close()
    assert_frame(run.dumps[0], want, "ref_dropin_main")


def test_application_matches_the_oracle(dropin):
    """The same dump against the CPU restatement, so that the comparison does not rest on
    the product alone: three regions, 34 pixels x 100 spp."""
    osc = dropin.init_spheres(CLOCK)
    fr = dropin.make_frame(dropin.camera_basis(EYE, LOOK, UP), EYE, SKY, W, H, SPP, BOUNCES, SEED)
    want = np.zeros(W * H * 3, np.uint8)
    offsets = []
    for r in ORACLE_REGIONS:
        dropin.render_segment(osc, fr, *r, rgb8=want)
        offsets.append(region_offsets(*r))
    offsets = np.concatenate(offsets)
    assert offsets.size == 34 * 3 and np.count_nonzero(want) <= offsets.size
    # liveness, on the oracle's side alone
    distinct = np.unique(want[offsets]).size
    _, _, spec, _ = dropin.trace_region(osc, fr, *GLASS_REGION)
    print(f"oracle regions: {distinct} distinct bytes, {np.count_nonzero(spec)} of {spec.size} glass-region paths "
          f"with specular events (most {spec.max()})")
    assert distinct >= 10
    assert np.count_nonzero(spec) > 0
    run = main_run(dropin)
    assert_ran(run, 1, "ref_dropin_main")
    got = run.dumps[0]
    bad = np.nonzero(got[offsets] != want[offsets])[0]
    assert bad.size == 0, (f"{bad.size} of {offsets.size} bytes differ from the oracle; first at offset {offsets[bad[0]]}: "
                           f"{got[offsets[bad[0]]]} for {want[offsets[bad[0]]]}")


def test_binaries_include_the_shim_not_the_reference_tracers(dropin):
    """What ran above ran the shim: a child's work is invisible to Context.stats(), so
    this rests on the include graph the compiler recorded beside each binary."""
    for path in (dropin.DROPIN_MAIN, dropin.DROPIN_DRIVER):
        errors = dropin.dropin_shadowing_errors(path)
        assert not errors, (path, errors)


# ---------------------------------------------------------------- 3: RenderImage

@pytest.mark.parametrize("name", ["init", "random"])
def test_render_image(dropin, spt, name):
    """RenderImage(): RenderSegmentTask over the whole (square: no aliasing) frame."""
    want = expected(spt, name, "image")
    if name == "random":
        assert scene(spt, "random").n > 100
        assert np.unique(want).size > 50
        assert np.count_nonzero(want != expected(spt, "init", "image")) > want.size // 100
    run = run_once(("image", name), lambda: dropin.run_dropin_driver("image", name, CLOCK))
    assert_ran(run, 1, f"image {name}")
    assert_frame(run.dumps[0], want, f"image {name}")


# ---------------------------------------------------------------- 4: three frames

@pytest.mark.parametrize("variant", list(FRAMES_ENVS))
def test_frames(dropin, spt, variant):
    """RenderImageParallelMain three times in one process over the RANDOM scene: the cold
    frame, the frame the armed read-ahead serves, and a frame after eyePos and viewMatrix
    changed (sync_globals' change detection on the reference's own Vec4 and Mat4); also with
    the read-ahead off and with the tiles as jobs of the render service."""
    first, third = expected(spt, "random", "tiles"), expected(spt, "random", "tiles", MOVED_EYE)
    assert np.count_nonzero(first != third) > first.size // 100
    run = run_once(("frames", variant),
                   lambda: dropin.run_dropin_driver("frames", "random", CLOCK, env=FRAMES_ENVS[variant]))
    assert_ran(run, 3, f"frames {variant}")
    for k, want in enumerate((first, first, third)):
        got = run.dumps[k]
        canaries = np.count_nonzero((got == 0xAB) & (want != 0xAB))
        assert canaries == 0, f"frames {variant}: {canaries} bytes of frame {k + 1} were never written"
        assert_frame(got, want, f"frames {variant}, frame {k + 1}")
    assert np.array_equal(run.dumps[0], run.dumps[1])


# ---------------------------------------------------------------- 5: picking and ray queries

def test_pick(dropin, spt):
    """spt_shim::PickSphere and spt_shim::FindClosestIntersectionSpheres on the reference's
    own globals, after a frame: what Context.primary_hits (sample 0) and Context.cast_rays
    answer."""
    s = scene(spt, "random")
    xs = np.linspace(0, W - 1, 8).astype(np.uint32)
    xy = np.array([(x, y) for y in xs for x in xs], np.uint32)  # 64 pixels, the frame's corners among them
    o, d, _, _ = make_rays(s.centers, s.radii, n=N_PICK_RAYS)
    c = context(spt, "random")
    want_pick = c.primary_hits(np.concatenate([xy, np.zeros((len(xy), 1), np.uint32)], axis=1))
    want_cast = c.cast_rays(o, d)
    c.close()
    # liveness: spheres and sky under the pixels; hits and misses among the rays, as test_gpu_cast asks
    assert 0 < np.count_nonzero(want_pick < s.n) < len(xy) and np.unique(want_pick).size >= 4
    frac = (want_cast < s.n).mean()
    print(f"pick: {np.count_nonzero(want_pick < s.n)} of 64 pixels on a sphere, {frac:.3f} of the rays hit")
    assert 0.5 <= frac <= 0.9
    run, pick, cast = run_once("pick", lambda: dropin.run_dropin_driver("pick", seed=CLOCK, pixels=xy, origins=o, dirs=d))
    assert_ran(run, 1, "pick")
    assert np.array_equal(pick, want_pick), np.nonzero(pick != want_pick)[0][:16]
    assert np.array_equal(cast, want_cast), np.nonzero(cast != want_cast)[0][:16]
    assert_frame(run.dumps[0], expected(spt, "random", "tiles"), "pick's frame")
