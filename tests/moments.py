"""What spt_render_moments and spt_denoise_var must return: the definitions of
include/spt_hip.h "sample moments" and "variance-guided denoiser"  restated
in numpy, shared by tests/test_moments_helper.py and tests/test_gpu_moments.py.  A plain
helper module: numpy only, it never calls the device.

Every array below is float32 and every line is one numpy operation per operation of the
definition, so nothing can contract and each result is rounded once, as the kernels'.
"""
import numpy as np

from denoise import H_TAPS

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
    weight was not > 0, over all levels."""
    rgba = np.ascontiguousarray(rgba, F).reshape(H, W, 4)
    feat = np.ascontiguousarray(feat, F).reshape(H, W, 2, 4)
    mom = np.ascontiguousarray(mom, F).reshape(H, W, 4)
    assert 1 <= levels <= 8
    vf = F(var_floor)
    with np.errstate(all="ignore"):
        kc, ka, kn, kz = (F(1.0) / (F(s) * F(s)) for s in sigmas)
        a = feat[:, :, 0, :3]
        n = feat[:, :, 1, :3]
        cov, dep = feat[:, :, 0, 3], feat[:, :, 1, 3]
        z = np.where(cov > 0, dep / np.where(cov > 0, cov, F(1.0)), F(0.0)).astype(F)
        g = mom[:, :, 2] / mom[:, :, 3]
        g = np.where(np.isfinite(g), g, F(np.nan)).astype(F)  # a quotient that is not finite is NaN
        ys, xs = np.mgrid[0:H, 0:W]
        u = rgba[:, :, :3].copy()
        skipped = 0
        order = [(j, i) for j in range(-2, 3) for i in range(-2, 3)]
        if reverse_taps:
            order.reverse()
        for k in range(levels):
            s = 1 << k
            acc = np.zeros((H, W, 3), F)
            ws = np.zeros((H, W), F)
            gacc = np.zeros((H, W), F)
            for j, i in order:
                xq, yq = xs + i * s, ys + j * s
                inside = (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
                xc, yc = np.clip(xq, 0, W - 1), np.clip(yq, 0, H - 1)
                uq = u[yc, xc]
                gq = g[yc, xc]
                du = uq - u
                dc = (du[..., 0] * du[..., 0] + du[..., 1] * du[..., 1]) + du[..., 2] * du[..., 2]
                da = a[yc, xc] - a
                d_a = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                dn = n[yc, xc] - n
                d_n = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                dz = z[yc, xc] - z
                d_z = dz * dz
                vn = vf + (g + gq)
                X = ((dc * kc) / vn + d_a * ka) + (d_n * kn + d_z * kz)
                w = (H_TAPS[abs(i)] * H_TAPS[abs(j)]) / (F(1.0) + X)
                take = inside & (w > 0)
                skipped += int((inside & ~take).sum())
                for c in range(3):
                    acc[..., c] = np.where(take, acc[..., c] + w * uq[..., c], acc[..., c])
                ws = np.where(take, ws + w, ws)
                gacc = np.where(take, gacc + (w * w) * gq, gacc)
                assert X.dtype == F and w.dtype == F and acc.dtype == F and ws.dtype == F and gacc.dtype == F
            live = ws > 0
            nxt = u.copy()  # no weight at all: colour and g pass through, bits and all
            safe = np.where(live, ws, F(1.0))
            for c in range(3):
                nxt[..., c] = np.where(live, acc[..., c] / safe, u[..., c])
            g = np.where(live, gacc / (safe * safe), g).astype(F)
            u = nxt
    out = rgba.copy()
    out[:, :, :3] = u
    assert out.dtype == F and g.dtype == F
    return out, g, skipped
