"""The contract of adaptive sampling itself (tests/adaptive.py, the numpy restatement the GPU
tests compare against), checked on the CPU against the oracle alone.

The frame is tests/test_moments_helper.py's: the golden `random` scene at 96 x 64, depth 8,
seed 3, with the per-sample colours of oracle.trace_region at 64 spp; the reference image is
the oracle's at 600 spp with seed 103.  Measured with this helper at base 8, step 8, max 64,
tol 0.08, floor 1.0: mean 35.25 spp, active tiles per pass 96, 54, 50, 49, 49, 47, 43, 35,
RMSE 2.454 against 3.071 for the uniform frame at 36 spp (and 2.364 at 64 spp).
"""
import math

import numpy as np

from adaptive import expected_adaptive, pixel_counts, tile_ids
from denoise import rmse
from moments import expected_moments
from test_denoise_helper import H, REF_SEED, REF_SPP, W
from test_gpu_features import DEPTH, SEED
from test_gpu_parity import EYE, SKY, bits, oscene_from

BASE, STEP, MAX, TOL, FLOOR = 8, 8, 64, 0.08, 1.0

_frame = {}


def frame(oracle, golden_scenes):
    """The oracle's scene, its per-sample colours at MAX spp and the contract's answer."""
    if not _frame:
        osc = oscene_from(oracle, golden_scenes, "random")
        fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W, H, MAX, DEPTH, SEED)
        col = oracle.trace_region(osc, fr, 0, H, 0, W)[0]
        rgba, mom, n_map, active = expected_adaptive(col, W, H, BASE, STEP, MAX, TOL, FLOOR)
        _frame.update(osc=osc, col=col, rgba=rgba, mom=mom, n_map=n_map, active=active)
    return _frame


def uniform(oracle, golden_scenes, osc, spp, seed=SEED):
    fr = oracle.make_frame(golden_scenes["view"], EYE, SKY, W, H, spp, DEPTH, seed)
    return oracle.render_segment(osc, fr, 0, H, 0, W)[0]


def test_each_pixel_is_the_plain_render_at_its_own_count(oracle, golden_scenes):
    f = frame(oracle, golden_scenes)
    n_pix = pixel_counts(f["n_map"], W, H)
    assert np.array_equal(f["mom"][:, 3], n_pix.astype(np.float32))
    for n in np.unique(n_pix):
        plain = uniform(oracle, golden_scenes, f["osc"], int(n))
        at = n_pix == n
        assert np.array_equal(bits(f["rgba"][at]), bits(plain[at])), f"pixels that stopped at {n} samples"


def test_an_infinite_tolerance_gives_the_moments_of_the_base_pass(oracle, golden_scenes):
    f = frame(oracle, golden_scenes)
    rgba, mom, n_map, active = expected_adaptive(f["col"], W, H, BASE, STEP, MAX, float("inf"), FLOOR)
    assert active == [len(n_map.reshape(-1))] and (n_map == BASE).all()
    assert np.array_equal(bits(mom), bits(expected_moments(f["col"][:, :BASE])))
    assert np.array_equal(bits(rgba), bits(uniform(oracle, golden_scenes, f["osc"], BASE)))
    # tol = 0: exactly the tiles with some var > 0 after the base pass run to the end
    _, mom0, n0, _ = expected_adaptive(f["col"], W, H, BASE, STEP, MAX, 0.0, FLOOR)
    tile, n_tiles = tile_ids(W, H)
    noisy = np.zeros(n_tiles, bool)
    noisy[np.unique(tile[mom[:, 2] > 0])] = True
    assert noisy.any() and not noisy.all()
    assert np.array_equal(n0.reshape(-1), np.where(noisy, MAX, BASE))


def test_fewer_samples_reach_a_lower_error_than_the_uniform_frame(oracle, golden_scenes):
    f = frame(oracle, golden_scenes)
    ref = uniform(oracle, golden_scenes, f["osc"], REF_SPP, REF_SEED)
    n_pix = pixel_counts(f["n_map"], W, H)
    mean = float(n_pix.mean())
    e = rmse(f["rgba"], ref)
    e_uniform = rmse(uniform(oracle, golden_scenes, f["osc"], math.ceil(mean)), ref)
    print(f"adaptive {BASE}/{STEP}/{MAX}, tol {TOL}: mean {mean:.2f} spp, active tiles per pass {f['active']}, "
          f"RMSE {e:.3f} against {e_uniform:.3f} uniform at {math.ceil(mean)} spp")
    assert e < 0.9 * e_uniform, (e, e_uniform)
    assert mean < MAX
    assert len(np.unique(n_pix)) >= 3, np.unique(n_pix)
    assert f["active"][0] == f["n_map"].size and all(a >= b for a, b in zip(f["active"], f["active"][1:]))


def test_a_nan_pixel_counts_as_converged(oracle, golden_scenes):
    f = frame(oracle, golden_scenes)
    tile, _ = tile_ids(W, H)
    # a tile that stopped at the base pass, one pixel's samples forced NaN: it still stops there
    quiet = int(np.nonzero(f["n_map"].reshape(-1) == BASE)[0][0])
    p = int(np.nonzero(tile == quiet)[0][5])
    col = f["col"].copy()
    col[p, :, :3] = np.nan
    rgba, mom, n_map, _ = expected_adaptive(col, W, H, BASE, STEP, MAX, TOL, FLOOR)
    assert n_map.reshape(-1)[quiet] == BASE and np.array_equal(n_map, f["n_map"])
    assert np.isnan(rgba[p, :3]).all() and np.isnan(mom[p, :3]).all() and mom[p, 3] == BASE and rgba[p, 3] == 0
    others = np.arange(W * H) != p
    assert np.array_equal(bits(rgba[others]), bits(f["rgba"][others])) and np.array_equal(bits(mom[others]), bits(f["mom"][others]))
