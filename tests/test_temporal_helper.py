"""The temporal accumulation's definition itself (tests/temporal.py, the numpy restatement the
GPU tests compare against), checked on the CPU against the oracle alone: its rules have to be
live, it has to bring a frame closer to the converged image, its geometry has to land on the
same surface point, and a camera that stands still has to return every pixel to itself.

The "oracle pair" is the golden `random` scene seen by two cameras: camera 1 through
golden_scenes["view"] from the eye [0, 1, -3], camera 2 yawed 2 degrees from the eye
[0.15, 1.05, -2.9] (camera 3, for chains: 4 degrees, [0.3, 1.1, -2.8]).  Frame k of a sequence
has seed 3 + k, depth 8; colours and samples are the oracle's, features tests/features.py's,
moments tests/moments.py's.  Measured with this helper at 45 x 37 x 7 with the defaults: 89 %
of camera 2's pixels find history; 123 / 270 / 81 / 436 taps are rejected by the outside, ids,
normal and depth rule alone; the RMSE against the oracle's 300-spp image of camera 2 (seed
103) falls from 7.03 (raw) to 6.27.  Geometry at 48 x 32 x 4: the median distance is about a
third of a pixel footprint.
"""
import numpy as np

from denoise import rmse
from features import expected_features
from moments import expected_moments
from temporal import DEFAULTS, expected_temporal, inverse3, reproject, yawed
from test_gpu_features import DEPTH, SEED
from test_gpu_parity import EYE, SKY, bits, oscene_from

F = np.float32
W1, H1, S1 = 45, 37, 7
REF_SPP, REF_SEED = 300, 103
EYES = ([0, 1, -3, 0], [0.15, 1.05, -2.9, 0], [0.3, 1.1, -2.8, 0])
YAWS = (0.0, 2.0, 4.0)

_frames = {}


def camera(golden_scenes, k):
    """(view (16,), eye (4,)) of camera k = 0, 1, 2 (the docstring's cameras 1, 2, 3)."""
    assert EYES[0] == EYE
    view = np.ascontiguousarray(np.asarray(golden_scenes["view"], F).reshape(16))
    return (view if k == 0 else yawed(view, YAWS[k])), np.asarray(EYES[k], F)


def scene_arrays(golden_scenes):
    return tuple(golden_scenes[f"random_{k}"] for k in ("centers", "radii", "colors", "materials", "fuzz"))


def oracle_frame(oracle, golden_scenes, cam, W, H, spp, seed):
    """The oracle's frame of camera `cam` (a (view, eye) pair, or 0 / 1 / 2): a dict of rgba
    (H, W, 4), mom (H, W, 4), feat (H, W, 2, 4), ids (H, W), view and eye; computed once."""
    view, eye = camera(golden_scenes, cam) if isinstance(cam, int) else cam
    key = (bits(view).tobytes(), bits(eye).tobytes(), W, H, spp, seed)
    if key not in _frames:
        osc = oscene_from(oracle, golden_scenes, "random")
        fr = oracle.make_frame(view, eye, SKY, W, H, spp, DEPTH, seed)
        rgba, _ = oracle.render_segment(osc, fr, 0, H, 0, W)
        col = oracle.trace_region(osc, fr, 0, H, 0, W)[0]
        w = expected_features(oracle, osc, fr, scene_arrays(golden_scenes), (0, H, 0, W))
        _frames[key] = dict(rgba=rgba.reshape(H, W, 4), mom=expected_moments(col).reshape(H, W, 4),
                            feat=w["feat"].reshape(H, W, 2, 4), ids=w["ids"].reshape(H, W), view=view, eye=eye)
    return _frames[key]


def oracle_pair(oracle, golden_scenes, W, H, spp, cams=(0, 1)):
    """Frames 0 and 1 of a sequence: (history frame of cams[0], seed 3; current frame of cams[1], seed 4)."""
    return (oracle_frame(oracle, golden_scenes, cams[0], W, H, spp, SEED),
            oracle_frame(oracle, golden_scenes, cams[1], W, H, spp, SEED + 1))


def accumulate(cur, prev, minv=None, **kw):
    """expected_temporal of frame `cur` against the history frame `prev` (its rgba and mom as
    they are); kw may replace parts of the history ("history") or the parameters."""
    history = kw.pop("history", (prev["rgba"], prev["mom"], prev["feat"], prev["ids"]))
    H, W = cur["ids"].shape
    return expected_temporal(cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"], W, H, history,
                             prev["view"], prev["eye"], inverse3(prev["view"]) if minv is None else minv, **kw)


def test_every_rule_is_live_on_the_oracle_pair(oracle, golden_scenes):
    prev, cur = oracle_pair(oracle, golden_scenes, W1, H1, S1)
    out, out_mom, info = accumulate(cur, prev, **DEFAULTS)
    print(f"temporal 45x37x7: history in {info['history']:.3f} of the pixels, {info['taken']} taps taken, "
          f"rejected alone {info['alone']}")
    assert 0.5 <= info["history"] < 1.0 and (~info["has"]).any()
    for rule, n in info["alone"].items():
        assert n >= 1, rule
    sky = ~(cur["feat"][:, :, 0, 3] > 0)
    assert (sky & info["has"]).any(), "some sky pixel has history"
    # where there is history the sample counts add up, elsewhere the pixel passes through
    has = info["has"]
    assert (out_mom[has][:, 3] > S1).all() and (out_mom[has][:, 3] <= 2 * S1 * (1 + 1e-6)).all()  # hn / ws rounds
    assert np.array_equal(bits(out[~has]), bits(cur["rgba"][~has])) and np.array_equal(bits(out_mom[~has]), bits(cur["mom"][~has]))
    assert np.array_equal(bits(out[..., 3]), bits(cur["rgba"][..., 3])), "w passes through"


def test_the_definition_brings_the_frame_closer_to_the_converged_image(oracle, golden_scenes):
    """Measured: RMSE against the 300-spp image 7.03 raw, 6.27 accumulated (45 x 37 x 7)."""
    prev, cur = oracle_pair(oracle, golden_scenes, W1, H1, S1)
    ref = oracle_frame_rgba(oracle, golden_scenes, 1, W1, H1, REF_SPP, REF_SEED)
    out, _, _ = accumulate(cur, prev, **DEFAULTS)
    raw, acc = rmse(cur["rgba"], ref), rmse(out, ref)
    print(f"RMSE against {REF_SPP} spp: raw {raw:.3f}, accumulated over one {S1}-spp history frame {acc:.3f}")
    assert acc < raw, (acc, raw)


def oracle_frame_rgba(oracle, golden_scenes, cam, W, H, spp, seed):
    view, eye = camera(golden_scenes, cam)
    osc = oscene_from(oracle, golden_scenes, "random")
    return oracle.render_segment(osc, oracle.make_frame(view, eye, SKY, W, H, spp, DEPTH, seed), 0, H, 0, W)[0].reshape(H, W, 4)


def test_history_lands_on_the_same_surface_point(oracle, golden_scenes):
    """History colour = the previous frame's reconstructed hit point, history count 1e6 (and
    max_history 1e6), so the output colour is the reprojected point: over fully covered pixels
    with history it lies within one pixel footprint, 2 z / height, of the pixel's own P in
    the median (measured: about a third of one)."""
    W, H, spp = 48, 32, 4
    prev, cur = oracle_pair(oracle, golden_scenes, W, H, spp)
    # any inverse serves a camera's own reprojection: only P is read
    P_prev = reproject(prev["feat"], prev["view"], prev["eye"], W, H, inverse3(prev["view"]), prev["eye"])[4]
    P_cur = reproject(cur["feat"], cur["view"], cur["eye"], W, H, inverse3(prev["view"]), prev["eye"])[4]
    h_rgba = np.concatenate([P_prev, np.zeros((H, W, 1), F)], axis=2).astype(F)
    h_mom = prev["mom"].copy()
    h_mom[..., 3] = F(1e6)
    out, out_mom, info = accumulate(cur, prev, history=(h_rgba, h_mom, prev["feat"], prev["ids"]),
                                    tol_normal=0.25, tol_depth=0.1, max_history=1e6)
    sel = info["has"] & (cur["feat"][:, :, 0, 3] == 1)
    assert sel.sum() >= 0.3 * W * H
    z = cur["feat"][:, :, 1, 3][sel].astype(np.float64)
    dist = np.linalg.norm(out[sel][:, :3].astype(np.float64) - P_cur[sel].astype(np.float64), axis=1)
    rel = dist / (2.0 * z / H)
    print(f"geometry 48x32x4: {int(sel.sum())} pixels, median distance {np.median(rel):.3f} of a pixel footprint")
    assert np.median(rel) < 1.0


def test_a_static_camera_returns_every_pixel_to_itself(oracle, golden_scenes):
    W, H, spp = W1, H1, S1
    prev, cur = oracle_pair(oracle, golden_scenes, W, H, spp, cams=(0, 0))
    assert not np.array_equal(bits(prev["rgba"]), bits(cur["rgba"])), "the seeds differ"
    # the general path's arithmetic misses the pixel's own place by a few 1e-6: hence the rule
    gx, gy, _, _, _ = reproject(cur["feat"], cur["view"], cur["eye"], W, H, inverse3(prev["view"]), prev["eye"])
    ys, xs = np.mgrid[0:H, 0:W]
    miss = max(float(np.abs(gx - xs).max()), float(np.abs(gy - ys).max()))
    print(f"static camera 45x37: the unruled arithmetic misses the pixel by up to {miss:.2e}")
    assert 0 < miss < 1e-4
    out, out_mom, info = accumulate(cur, prev, tol_normal=np.inf, tol_depth=np.inf, max_history=64.0)
    assert np.array_equal(info["fx"], xs.astype(F)) and np.array_equal(info["fy"], ys.astype(F))
    same_id = prev["ids"] == cur["ids"]
    assert np.array_equal(info["has"], same_id) and same_id.mean() > 0.9
    # with every id equal every pixel has history, and two frames of equal spp meet half way
    ids = np.zeros((H, W), np.uint32)
    a, b = dict(cur, ids=ids), dict(prev, ids=ids)
    out, out_mom, info = accumulate(a, b, tol_normal=np.inf, tol_depth=np.inf, max_history=64.0)
    assert info["has"].all() and info["taken"] == W * H
    h, c = prev["rgba"][..., :3], cur["rgba"][..., :3]
    assert np.array_equal(bits(out[..., :3]), bits(h + (c - h) * F(0.5)))
    assert (out_mom[..., 3] == 2 * spp).all()
