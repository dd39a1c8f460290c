"""What spt_render_adaptive must return: the contract of include/spt_hip.h "adaptive sampling"
 restated in numpy, shared by tests/test_adaptive_helper.py and
tests/test_gpu_adaptive.py.  A plain helper module: numpy only, it never calls the device.

Every array below is float32 and every line is one numpy operation per operation of the
contract, so nothing can contract and each result is rounded once, as the kernel's.
"""
import numpy as np

from moments import LUMA

F = np.float32


def tile_ids(W, H):
    """The 8x8 tile (row-major over ceil(W / 8) x ceil(H / 8)) of each pixel of a W x H region,
    in local row-major pixel order, and the tile count."""
    tx, ty = (W + 7) // 8, (H + 7) // 8
    y, x = np.divmod(np.arange(W * H), W)
    return (y // 8) * tx + (x // 8), tx * ty


def expected_adaptive(col, W, H, base, step, mx, tol, floor):
    """col: per-sample colours of the W x H region, shape (W * H, >= mx, >= 3), pixel-major
    in local row-major order (what oracle.trace_region and spt_render_samples give at
    spp = mx).  Returns (rgba, mom, n_map, active): rgba and mom of shape (W * H, 4), the
    per-tile sample counts of shape (ceil(H / 8), ceil(W / 8)) and the number of active tiles
    in each pass run."""
    assert base >= 1 and step >= 1 and mx >= base and col.shape[0] == W * H and col.shape[1] >= mx
    col = np.ascontiguousarray(col, F)
    npix = W * H
    tile, n_tiles = tile_ids(W, H)
    tol, floor = F(tol), F(floor)
    acc = np.zeros((npix, 3), F)
    s1, s2 = np.zeros(npix, F), np.zeros(npix, F)
    rgba, mom = np.zeros((npix, 4), F), np.zeros((npix, 4), F)
    n_tile = np.zeros(n_tiles, np.int64)
    on = np.ones(n_tiles, bool)  # active tiles
    active = []
    n = 0
    with np.errstate(all="ignore"):
        while on.any():
            take = base if n == 0 else min(step, mx - n)
            active.append(int(on.sum()))
            px = on[tile]  # pixels of the pass
            for s in range(n, n + take):
                c = col[px, s]
                acc[px] = acc[px] + c[:, :3]
                L = (c[:, 0] * LUMA[0] + c[:, 1] * LUMA[1]) + c[:, 2] * LUMA[2]
                s1[px] = s1[px] + L
                s2[px] = s2[px] + L * L
                assert L.dtype == F
            n += take
            inv = F(1.0) / F(n)
            m1, m2 = s1 * inv, s2 * inv
            d = m2 - m1 * m1
            var = np.where(d < 0, F(0.0), d)  # NaN stays NaN
            e = var * inv
            r = (m1 + floor) * tol
            thr = r * r
            unconverged = (e > thr) & px  # NaN compares false: converged
            assert e.dtype == F and thr.dtype == F
            stay = np.zeros(n_tiles, bool)
            if n < mx:
                stay[np.unique(tile[unconverged])] = True
            stop = on & ~stay
            out = stop[tile]
            rgba[out, :3] = acc[out] * inv
            mom[out] = np.stack([m1, m2, var, np.full(npix, F(n))], axis=1)[out]
            n_tile[stop] = n
            on = stay
    assert rgba.dtype == F and mom.dtype == F
    return rgba, mom, n_tile.reshape((H + 7) // 8, (W + 7) // 8), active


def pixel_counts(n_map, W, H):
    """The per-tile sample counts as one count per pixel, local row-major."""
    tile, _ = tile_ids(W, H)
    return n_map.reshape(-1)[tile]
