"""What spt_denoise must return: the definition of include/spt_hip.h "denoiser" (DESIGN.md
§4.11) restated in numpy, shared by tests/test_denoise_helper.py and
tests/test_gpu_denoise.py.  A plain helper module: numpy only (the bytes go through the
oracle's spo_write_pixel), it never calls the device.

Every array below is float32 and every line is one numpy operation per operation of the
definition, so nothing can contract and each result is rounded once, as the kernel's.
"""
import ctypes

import numpy as np

F = np.float32
H_TAPS = (F(0.375), F(0.25), F(0.0625))
DEFAULT_SIGMAS = (30.0, 0.1, 0.25, 0.5)


def level_walk(rgba, feat, W, H, sigmas, levels, reverse_taps=False, mom=None, var_floor=None):
    """The levels of both filters, the one place the edge rule, the tap order and the
    pass-through rule are written.  mom None: the plain form, the colour factor times 4^k at
    level k.  mom given (4 floats per pixel, with var_floor): the variance-guided form, g =
    mom.z / mom.w rides along, the colour term is divided by var_floor + (g_p + g_q) and the
    colour factor stays.  Returns (out, g, skipped): out of shape (H, W, 4), g of shape (H, W)
    or None, and the number of in-image taps skipped because their weight was not > 0."""
    rgba = np.ascontiguousarray(rgba, F).reshape(H, W, 4)
    feat = np.ascontiguousarray(feat, F).reshape(H, W, 2, 4)
    var = mom is not None
    assert 1 <= levels <= 8
    with np.errstate(all="ignore"):
        kc, ka, kn, kz = (F(1.0) / (F(s) * F(s)) for s in sigmas)
        a = feat[:, :, 0, :3]
        n = feat[:, :, 1, :3]
        cov, dep = feat[:, :, 0, 3], feat[:, :, 1, 3]
        z = np.where(cov > 0, dep / np.where(cov > 0, cov, F(1.0)), F(0.0)).astype(F)
        g = None
        if var:
            mom = np.ascontiguousarray(mom, F).reshape(H, W, 4)
            vf = F(var_floor)
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
            kck = kc if var else kc * F(4 ** k)
            acc = np.zeros((H, W, 3), F)
            ws = np.zeros((H, W), F)
            gacc = np.zeros((H, W), F)  # the variance form's
            for j, i in order:
                xq, yq = xs + i * s, ys + j * s
                inside = (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
                xc, yc = np.clip(xq, 0, W - 1), np.clip(yq, 0, H - 1)
                uq = u[yc, xc]
                du = uq - u
                dc = (du[..., 0] * du[..., 0] + du[..., 1] * du[..., 1]) + du[..., 2] * du[..., 2]
                da = a[yc, xc] - a
                d_a = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                dn = n[yc, xc] - n
                d_n = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                dz = z[yc, xc] - z
                d_z = dz * dz
                tc = dc * kck
                if var:
                    gq = g[yc, xc]
                    vn = vf + (g + gq)
                    tc = tc / vn
                X = (tc + d_a * ka) + (d_n * kn + d_z * kz)
                w = (H_TAPS[abs(i)] * H_TAPS[abs(j)]) / (F(1.0) + X)
                take = inside & (w > 0)
                skipped += int((inside & ~take).sum())
                for c in range(3):
                    acc[..., c] = np.where(take, acc[..., c] + w * uq[..., c], acc[..., c])
                ws = np.where(take, ws + w, ws)
                if var:
                    gacc = np.where(take, gacc + (w * w) * gq, gacc)
                assert X.dtype == F and w.dtype == F and acc.dtype == F and ws.dtype == F and gacc.dtype == F
            live = ws > 0
            nxt = u.copy()  # no weight at all: the pixel (and g) passes through, bits and all
            safe = np.where(live, ws, F(1.0))
            for c in range(3):
                nxt[..., c] = np.where(live, acc[..., c] / safe, u[..., c])
            if var:
                g = np.where(live, gacc / (safe * safe), g).astype(F)
            u = nxt
    out = rgba.copy()
    out[:, :, :3] = u
    assert out.dtype == F and (g is None or g.dtype == F)
    return out, g, skipped


def expected_denoise(rgba, feat, W, H, sigmas=DEFAULT_SIGMAS, levels=3, reverse_taps=False):
    """rgba: W * H float4 pixels (any shape), feat: 8 floats per pixel in spt_render_features'
    layout, sigmas: (color, albedo, normal, depth), each > 0 (inf allowed).  Returns
    (out, skipped): out of shape (H, W, 4) and the number of in-image taps skipped because
    their weight was not > 0, over all levels.  reverse_taps visits the 25 taps in the
    opposite order (j = 2 .. -2, i = 2 .. -2): the same sums in another order, for the tests'
    liveness checks."""
    out, _, skipped = level_walk(rgba, feat, W, H, sigmas, levels, reverse_taps)
    return out, skipped


def expected_bytes(oracle, out, W, H):
    """`out` as a g_data frame of its own W x H (W * H * 3 bytes): pixel (x, y) at
    W*H*3 - ((W - x)*3 + y*W*3), each pixel's bytes the oracle's spo_write_pixel."""
    out = np.ascontiguousarray(out, F).reshape(H * W, 4)
    g = np.zeros(W * H * 3, np.uint8)
    L = oracle.lib()
    b = np.zeros(3, np.uint8)
    bp = b.ctypes.data_as(ctypes.c_void_p)
    for y in range(H):
        for x in range(W):
            L.spo_write_pixel(ctypes.c_void_p(out.ctypes.data + 16 * (y * W + x)), bp)
            at = W * H * 3 - ((W - x) * 3 + y * W * 3)
            g[at:at + 3] = b
    return g


def rmse(a, b):
    """Root mean square error over the rgb lanes, in float64."""
    d = np.asarray(a, np.float64)[..., :3].reshape(-1, 3) - np.asarray(b, np.float64)[..., :3].reshape(-1, 3)
    return float(np.sqrt((d * d).mean()))
