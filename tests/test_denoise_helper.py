"""The denoiser's definition itself (tests/denoise.py, the numpy restatement the GPU tests
compare against), checked on the CPU against the oracle alone: it has to denoise, and
non-finite pixels have to stay where they are.

The image is the golden `random` scene through golden_scenes["view"] from the eye
[0, 1, -3], depth 8, seed 3, at 96 x 64 x 4 spp, rendered by the oracle; its features are
tests/features.py's; the reference image is the oracle's at 600 spp with seed 103.  Measured
with this helper: the RMSE against that image falls from 9.10 (raw) to 7.29 with the default
sigmas (30, 0.1, 0.25, 0.5) at 3 levels, and to 6.63 with sigma_albedo = +inf.
"""
import numpy as np

from denoise import DEFAULT_SIGMAS, expected_denoise, rmse
from test_gpu_features import DEPTH, SEED, want_random
from test_gpu_parity import EYE, SKY, bits

W, H, SPP = 96, 64, 4
REF_SPP, REF_SEED = 600, 103

_inputs = {}


def oracle_inputs(oracle, golden_scenes, W, H, spp):
    """(rgba (H * W, 4), feat (H * W, 2, 4)) of the oracle's frame, computed once."""
    key = (W, H, spp)
    if key not in _inputs:
        import simplepathtracer_amd as spt
        w = want_random(oracle, spt, golden_scenes, W, H, spp)
        s = w["scene"]
        osc = oracle.OracleScene(s.centers, s.radii, s.colors, s.materials, s.fuzz)
        fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W, H, spp, DEPTH, SEED)
        rgba, _ = oracle.render_segment(osc, fr, 0, H, 0, W)
        _inputs[key] = (rgba, w["feat"], osc)
    return _inputs[key][:2]


def test_the_definition_denoises(oracle, golden_scenes):
    rgba, feat = oracle_inputs(oracle, golden_scenes, W, H, SPP)
    osc = _inputs[(W, H, SPP)][2]
    fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W, H, REF_SPP, DEPTH, REF_SEED)
    ref, _ = oracle.render_segment(osc, fr, 0, H, 0, W)
    raw = rmse(rgba, ref)
    out, _ = expected_denoise(rgba, feat, W, H, DEFAULT_SIGMAS, 3)
    out_noalb, _ = expected_denoise(rgba, feat, W, H, (30.0, np.inf, 0.25, 0.5), 3)
    e, e_noalb = rmse(out, ref), rmse(out_noalb, ref)
    print(f"RMSE against {REF_SPP} spp: raw {raw:.3f}, filtered {e:.3f}, without the albedo term {e_noalb:.3f}")
    assert e < 0.9 * raw, (e, raw)
    assert e_noalb < 0.9 * raw, (e_noalb, raw)
    # w passes through
    assert np.array_equal(bits(out[..., 3]), bits(rgba.reshape(H, W, 4)[..., 3]))


def test_nonfinite_pixels_pass_through_and_never_spread(oracle, golden_scenes):
    rgba, feat = oracle_inputs(oracle, golden_scenes, W, H, SPP)
    rgba = rgba.reshape(H, W, 4).copy()
    spots = {(10, 20): np.nan, (31, 50): np.inf, (63, 95): -np.inf}  # (y, x); the last is a corner
    for (y, x), v in spots.items():
        rgba[y, x, :3] = v
    out, skipped = expected_denoise(rgba, feat, W, H, DEFAULT_SIGMAS, 3)
    bad = ~np.isfinite(out[..., :3]).all(axis=2)
    assert sorted(zip(*np.nonzero(bad))) == sorted(spots), "exactly those three pixels are non-finite"
    for (y, x) in spots:
        assert np.array_equal(bits(out[y, x]), bits(rgba[y, x])), (y, x)
    assert skipped >= 1, skipped
    # away from the three pixels' taps (at most 2 * (1 + 2 + 4) = 14 pixels off) nothing moved
    clean, _ = expected_denoise(oracle_inputs(oracle, golden_scenes, W, H, SPP)[0], feat, W, H, DEFAULT_SIGMAS, 3)
    far = np.ones((H, W), bool)
    for (y, x) in spots:
        far[max(y - 14, 0):y + 15, max(x - 14, 0):x + 15] = False
    assert far.any() and np.array_equal(bits(out[far]), bits(clean[far]))
