"""What spt_render_moments and spt_denoise_var must return: the definitions of
include/spt_hip.h "sample moments" and "variance-guided denoiser"  restated
in numpy, shared by tests/test_moments_helper.py and tests/test_gpu_moments.py.  A plain
helper module: numpy only, it never calls the device.

Every array below is float32 and every line is one numpy operation per operation of the
definition, so nothing can contract and each result is rounded once, as the kernels'.
"""
import numpy as np

from denoise import level_walk

F = np.float32
LUMA = (F(0.2126), F(0.7152), F(0.0722))
DEFAULT_VAR_SIGMAS = (4.0, 0.1, 0.25, 0.5)
DEFAULT_VAR_FLOOR = 1.0


def expected_moments(col, reverse=False):
    """col: per-sample colours of shape (pixels, spp, >= 3) (what spt_render_samples and
    oracle.trace_region give).  Returns mom of shape (pixels, 4): {m1, m2, var, spp} of the
    samples' luminance, summed from +0 in sample order (reverse: in the opposite order, for
    the tests' liveness checks)."""
    col = np.ascontiguousarray(col, F)
    n, spp = col.shape[:2]
    s1, s2 = np.zeros(n, F), np.zeros(n, F)
    with np.errstate(all="ignore"):
        for s in (range(spp - 1, -1, -1) if reverse else range(spp)):
            c = col[:, s]
            L = (c[:, 0] * LUMA[0] + c[:, 1] * LUMA[1]) + c[:, 2] * LUMA[2]
            s1 = s1 + L
            s2 = s2 + L * L
            assert L.dtype == F and s1.dtype == F and s2.dtype == F
        inv = F(1.0) / F(spp)
        m1, m2 = s1 * inv, s2 * inv
        d = m2 - m1 * m1
        var = np.where(d < 0, F(0.0), d)  # NaN stays NaN
    mom = np.stack([m1, m2, var, np.full(n, F(spp))], axis=1)
    assert mom.dtype == F
    return mom


def expected_denoise_var(rgba, feat, mom, W, H, sigmas=DEFAULT_VAR_SIGMAS, var_floor=DEFAULT_VAR_FLOOR, levels=3,
                         reverse_taps=False):
    """rgba: W * H float4 pixels, feat: 8 floats per pixel, mom: 4 floats per pixel (any
    shapes), sigmas: (color, albedo, normal, depth).  Returns (out, out_var, skipped): out of
    shape (H, W, 4), out_var (H, W), and the number of in-image taps skipped because their
    weight was not > 0, over all levels.  The levels themselves are tests/denoise.py's
    level_walk, the variance-guided form."""
    return level_walk(rgba, feat, W, H, sigmas, levels, reverse_taps, mom=mom, var_floor=var_floor)
