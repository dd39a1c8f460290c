"""The definitions of the sample moments and of the variance-guided filter themselves
(tests/moments.py, the numpy restatement the GPU tests compare against), checked on the CPU
against the oracle alone.

The frame is tests/test_denoise_helper.py's: the golden `random` scene at 96 x 64 x 4 spp,
depth 8, seed 3, with the per-sample colours of oracle.trace_region; the reference image is
the oracle's at 600 spp with seed 103.  Measured with this helper: 58.6 % of the pixels have
variance exactly 0 (sky-only or single-surface pixels); the RMSE against the reference is 9.096
raw, 7.287 after the plain filter at its defaults and 6.947 after the variance-guided filter
at its own (sigma_color 4, var_floor 1.0, 3 levels).
"""
import numpy as np

from denoise import DEFAULT_SIGMAS, expected_denoise, rmse
from moments import DEFAULT_VAR_FLOOR, DEFAULT_VAR_SIGMAS, expected_denoise_var, expected_moments
from test_denoise_helper import H, REF_SEED, REF_SPP, SPP, W, _inputs, oracle_inputs
from test_gpu_features import DEPTH, SEED
from test_gpu_parity import EYE, SKY, bits

_frame = {}


def frame(oracle, golden_scenes):
    """rgba, feat of test_denoise_helper's frame, its per-sample colours and their moments."""
    if not _frame:
        rgba, feat = oracle_inputs(oracle, golden_scenes, W, H, SPP)
        osc = _inputs[(W, H, SPP)][2]
        fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W, H, SPP, DEPTH, SEED)
        col = oracle.trace_region(osc, fr, 0, H, 0, W)[0]
        _frame.update(rgba=rgba, feat=feat, osc=osc, col=col, mom=expected_moments(col))
    return _frame


def test_the_mean_of_the_samples_is_the_render(oracle, golden_scenes):
    f = frame(oracle, golden_scenes)
    col = f["col"]
    acc = np.zeros((W * H, 3), np.float32)
    for s in range(SPP):
        acc = acc + col[:, s, :3]
    mean = acc * (np.float32(1.0) / np.float32(SPP))
    assert np.array_equal(bits(mean), bits(f["rgba"][:, :3]))


def test_zero_and_positive_variances_and_the_sample_order(oracle, golden_scenes):
    f = frame(oracle, golden_scenes)
    mom = f["mom"]
    assert mom.shape == (W * H, 4) and (mom[:, 3] == SPP).all() and np.isfinite(mom).all()
    zero, pos = float((mom[:, 2] == 0).mean()), float((mom[:, 2] > 0).mean())
    print(f"variance == 0 in {zero:.3f} of the pixels, > 0 in {pos:.3f}")
    assert zero > 0 and pos > 0 and zero + pos == 1.0
    assert (mom[:, 2] >= 0).all()
    rev = expected_moments(f["col"], reverse=True)
    order = int((bits(rev[:, 1]) != bits(mom[:, 1])).sum())
    print(f"the sample order changes m2 in {order} pixels")
    assert order >= 1


def test_the_definition_denoises_better_than_the_plain_filter(oracle, golden_scenes):
    f = frame(oracle, golden_scenes)
    fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W, H, REF_SPP, DEPTH, REF_SEED)
    ref, _ = oracle.render_segment(f["osc"], fr, 0, H, 0, W)
    raw = rmse(f["rgba"], ref)
    plain, _ = expected_denoise(f["rgba"], f["feat"], W, H, DEFAULT_SIGMAS, 3)
    out, out_var, _ = expected_denoise_var(f["rgba"], f["feat"], f["mom"], W, H, DEFAULT_VAR_SIGMAS, DEFAULT_VAR_FLOOR, 3)
    e_plain, e = rmse(plain, ref), rmse(out, ref)
    print(f"RMSE against {REF_SPP} spp: raw {raw:.3f}, plain filter {e_plain:.3f}, variance-guided {e:.3f}")
    assert e < 0.9 * raw, (e, raw)
    assert e < e_plain, (e, e_plain)
    # the filtered variance of the means is finite, not negative and mostly below the input's
    g0 = (f["mom"][:, 2] / f["mom"][:, 3]).reshape(H, W)
    assert np.isfinite(out_var).all() and (out_var >= 0).all() and out_var.mean() < g0.mean()
    # w passes through
    assert np.array_equal(bits(out[..., 3]), bits(f["rgba"].reshape(H, W, 4)[..., 3]))


def test_nonfinite_variances_pass_through_and_never_spread(oracle, golden_scenes):
    f = frame(oracle, golden_scenes)
    rgba = f["rgba"].reshape(H, W, 4)
    mom = f["mom"].reshape(H, W, 4).copy()
    spots = {(10, 20): np.nan, (31, 50): np.inf, (63, 95): -np.inf}  # (y, x); the last is a corner
    for (y, x), v in spots.items():
        mom[y, x, 2] = v
    out, out_var, skipped = expected_denoise_var(rgba, f["feat"], mom, W, H)
    assert np.isfinite(out).all(), "no colour turns non-finite"
    for (y, x) in spots:
        assert np.array_equal(bits(out[y, x]), bits(rgba[y, x])), (y, x)
    bad = ~np.isfinite(out_var)
    assert sorted(zip(*np.nonzero(bad))) == sorted(spots), "exactly those three variances are non-finite"
    assert skipped >= 1, skipped
    # away from the three pixels' taps (at most 2 * (1 + 2 + 4) = 14 pixels off) nothing moved
    clean, clean_var, _ = expected_denoise_var(rgba, f["feat"], f["mom"], W, H)
    far = np.ones((H, W), bool)
    for (y, x) in spots:
        far[max(y - 14, 0):y + 15, max(x - 14, 0):x + 15] = False
    assert far.any() and np.array_equal(bits(out[far]), bits(clean[far]))
    assert np.array_equal(bits(out_var[far]), bits(clean_var[far]))
    assert np.array_equal(bits(out[..., 3]), bits(rgba[..., 3]))
