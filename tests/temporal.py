"""What spt_temporal must return: the definition of include/spt_hip.h "temporal accumulation"
 restated in numpy, shared by tests/test_temporal_helper.py and
tests/test_gpu_temporal.py.  A plain helper module: numpy only, it never calls the device.

Every array below is float32 and every line is one numpy operation per operation of the
definition, so nothing can contract and each result is rounded once, as the kernel's.  Minv,
the inverse of the previous camera's 3x3 block, is passed in (spt_temporal_inverse's on the
GPU's side; inverse3 below where no library is at hand).
"""
import numpy as np

F = np.float32
INF = float("inf")
DEFAULTS = dict(tol_normal=0.25, tol_depth=0.1, max_history=64.0)
RULES = ("outside", "ids", "normal", "depth")


def inverse3(view):
    """np.linalg.inv of view's upper-left 3x3 in float64, rounded to float32: (3, 3)."""
    m = np.asarray(view, F).reshape(4, 4)[:3, :3].astype(np.float64)
    return np.linalg.inv(m).astype(F)


def yawed(view, degrees):
    """`view` turned about the world's y axis by `degrees`: the 16 floats of a camera that
    sees what `view` sees, rotated (computed in float64, rounded once)."""
    v = np.asarray(view, F).reshape(4, 4).astype(np.float64)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    out = v.copy()
    out[:3, :3] = ry @ v[:3, :3]
    return np.ascontiguousarray(out.astype(F).reshape(16))


def cameras_equal(view, eye, prev_view, prev_eye):
    """The static rule's condition: the nine used entries and the eyes' xyz compare equal."""
    a, b = np.asarray(view, F).reshape(4, 4)[:3, :3], np.asarray(prev_view, F).reshape(4, 4)[:3, :3]
    return bool((a == b).all() and (np.asarray(eye, F).reshape(-1)[:3] == np.asarray(prev_eye, F).reshape(-1)[:3]).all())


def _mean_depth(feat):
    cov, dep = feat[:, :, 0, 3], feat[:, :, 1, 3]
    hit = cov > 0
    z = np.where(hit, dep / np.where(hit, cov, F(1.0)), F(0.0))
    assert z.dtype == F
    return z, hit


def reproject(feat, view, eye, W, H, minv, prev_eye, static=False):
    """The geometry of the definition for every pixel: (fx, fy, front, L, P), all (H, W) but
    P (H, W, 3), the reconstructed hit point (E + d * z; the sky's is not used)."""
    feat = np.ascontiguousarray(feat, F).reshape(H, W, 2, 4)
    M = np.asarray(view, F).reshape(16)
    E, Ep = np.asarray(eye, F).reshape(-1)[:3], np.asarray(prev_eye, F).reshape(-1)[:3]
    Mi = np.asarray(minv, F).reshape(9)
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(F), ys.astype(F)
    fw, fh = F(W), F(H)
    with np.errstate(all="ignore"):
        z, hit = _mean_depth(feat)
        vx = F(-1.0) + F(2.0) * (xf / fh)
        vy = F(-1.0) + F(2.0) * (yf / fw)
        r = [(M[4 * i] * vx + M[4 * i + 1] * vy) + M[4 * i + 2] for i in range(3)]
        ln = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        d = [r[i] / ln for i in range(3)]
        P = [E[i] + d[i] * z for i in range(3)]
        wh = [P[i] - Ep[i] for i in range(3)]
        L = np.where(hit, np.sqrt((wh[0] * wh[0] + wh[1] * wh[1]) + wh[2] * wh[2]), F(0.0))
        w = [np.where(hit, wh[i], d[i]) for i in range(3)]
        q = [(Mi[3 * i] * w[0] + Mi[3 * i + 1] * w[1]) + Mi[3 * i + 2] * w[2] for i in range(3)]
        a, b = q[0] / q[2], q[1] / q[2]
        fx = ((a + F(1.0)) * F(0.5)) * fh
        fy = ((b + F(1.0)) * F(0.5)) * fw
        front = q[2] > 0
    if static:
        fx, fy, front = xf, yf, np.ones((H, W), bool)
    for v in (vx, ln, L, fx, fy, *d, *P, *q):
        assert v.dtype == F
    return fx, fy, front, L, np.stack(P, axis=2)


def expected_temporal(rgba, mom, feat, ids, view, eye, W, H, history=None, prev_view=None, prev_eye=None, minv=None,
                      tol_normal=0.25, tol_depth=0.1, max_history=64.0):
    """This frame's rgba (4), mom (4), feat (8 floats per pixel) and ids (any shapes), its
    camera, and `history` = (rgba, mom, feat, ids) of the previous frame with prev_view,
    prev_eye and minv (None: no history).  Returns (out_rgba (H, W, 4), out_mom (H, W, 4),
    info); info has

        history   the share of pixels that found history (ws > 0)
        has       (H, W) bool, those pixels
        taken     the taps taken
        alone     {rule: taps that rule rejects and every other test accepts}, rules
                  "outside", "ids", "normal", "depth"; over the taps with wt > 0 of pixels that
                  seek history, and ("outside" apart: such a tap has no pixel to test) over tap
                  pixels that are valid (hist_mom.w > 0, finite colour and moments)
        fx, fy    (H, W) the reprojected coordinates
        sought    (H, W) bool, the pixels that seek history
    """
    rgba = np.ascontiguousarray(rgba, F).reshape(H, W, 4)
    mom = np.ascontiguousarray(mom, F).reshape(H, W, 4)
    feat = np.ascontiguousarray(feat, F).reshape(H, W, 2, 4)
    ids = np.ascontiguousarray(ids, np.uint32).reshape(H, W)
    out, out_mom = rgba.copy(), mom.copy()
    none = np.zeros((H, W), bool)
    info = dict(history=0.0, has=none, taken=0, alone={r: 0 for r in RULES}, fx=None, fy=None, sought=none)
    if history is None:
        return out, out_mom, info
    h_rgba = np.ascontiguousarray(history[0], F).reshape(H, W, 4)
    h_mom = np.ascontiguousarray(history[1], F).reshape(H, W, 4)
    h_feat = np.ascontiguousarray(history[2], F).reshape(H, W, 2, 4)
    h_ids = np.ascontiguousarray(history[3], np.uint32).reshape(H, W)
    tn, td, mh = F(tol_normal), F(tol_depth), F(max_history)
    static = cameras_equal(view, eye, prev_view, prev_eye)
    fx, fy, front, L, _ = reproject(feat, view, eye, W, H, minv, prev_eye, static)
    with np.errstate(all="ignore"):
        cur_ok = (np.isfinite(rgba[..., :3]).all(axis=2) & np.isfinite(mom).all(axis=2) &
                  np.isfinite(feat).all(axis=(2, 3)) & (mom[..., 3] > 0))
        sought = cur_ok & front & (fx > F(-1.0)) & (fx < F(W)) & (fy > F(-1.0)) & (fy < F(H))
        hit = feat[:, :, 0, 3] > 0
        zq, _ = _mean_depth(h_feat)
        nrm, h_nrm = feat[:, :, 1, :3], h_feat[:, :, 1, :3]
        x0 = np.where(sought, np.floor(fx), F(0.0))
        y0 = np.where(sought, np.floor(fy), F(0.0))
        tx, ty = np.where(sought, fx, F(0.0)) - x0, np.where(sought, fy, F(0.0)) - y0
        xi0, yi0 = x0.astype(np.int64), y0.astype(np.int64)
        lim = td * L
        lim2 = lim * lim
        ws = np.zeros((H, W), F)
        hc = np.zeros((H, W, 3), F)
        h1, h2, hn = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
        taken, alone = 0, {r: 0 for r in RULES}
        for j in (0, 1):
            for i in (0, 1):
                xi, yj = xi0 + i, yi0 + j
                inside = (xi >= 0) & (xi < W) & (yj >= 0) & (yj < H)
                xc, yc = np.clip(xi, 0, W - 1), np.clip(yj, 0, H - 1)
                wt = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
                tc, tm = h_rgba[yc, xc], h_mom[yc, xc]
                valid = (tm[..., 3] > 0) & np.isfinite(tc[..., :3]).all(axis=2) & np.isfinite(tm[..., [0, 1, 3]]).all(axis=2)
                id_ok = h_ids[yc, xc] == ids
                dn = h_nrm[yc, xc] - nrm
                dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                n_ok = (dn2 <= tn) if tn != INF else np.ones((H, W), bool)
                dz = zq[yc, xc] - L
                d_ok = ~hit | (dz * dz <= lim2) if td != INF else np.ones((H, W), bool)
                live = sought & (wt > 0)
                take = live & inside & valid & id_ok & n_ok & d_ok
                taken += int(take.sum())
                alone["outside"] += int((live & ~inside).sum())
                alone["ids"] += int((live & inside & valid & ~id_ok & n_ok & d_ok).sum())
                alone["normal"] += int((live & inside & valid & id_ok & ~n_ok & d_ok).sum())
                alone["depth"] += int((live & inside & valid & id_ok & n_ok & ~d_ok).sum())
                ws = np.where(take, ws + wt, ws)
                for c in range(3):
                    hc[..., c] = np.where(take, hc[..., c] + wt * tc[..., c], hc[..., c])
                h1 = np.where(take, h1 + wt * tm[..., 0], h1)
                h2 = np.where(take, h2 + wt * tm[..., 1], h2)
                hn = np.where(take, hn + wt * tm[..., 3], hn)
                for v in (wt, dn2, dz, ws, hc, h1, h2, hn):
                    assert v.dtype == F
        has = ws > 0
        safe = np.where(has, ws, F(1.0))
        nh = np.fmin(hn / safe, mh)
        nc = mom[..., 3]
        nn = nh + nc
        alpha = nc / nn
        for c in range(3):
            h = hc[..., c] / safe
            out[..., c] = np.where(has, h + (rgba[..., c] - h) * alpha, rgba[..., c])
        h1, h2 = h1 / safe, h2 / safe
        m1 = h1 + (mom[..., 0] - h1) * alpha
        m2 = h2 + (mom[..., 1] - h2) * alpha
        dd = m2 - m1 * m1
        var = np.where(dd < 0, F(0.0), dd)
        acc = np.stack([m1, m2, var, nn], axis=2)
        assert acc.dtype == F and alpha.dtype == F and out.dtype == F
        out_mom = np.where(has[..., None], acc, mom)
    info.update(history=float(has.mean()), has=has, taken=taken, alone=alone, fx=fx, fy=fy, sought=sought)
    return out, out_mom, info
