"""What spt_temporal_motion must return: the definition of include/spt_hip.h "temporal
accumulation under moving spheres"  restated in numpy, shared by
tests/test_temporal_motion_helper.py and tests/test_gpu_temporal_motion.py.  A plain helper
module: numpy only, it never calls the device.

The contract is tests/temporal.py's with other w, L and static rule on the pixels whose sphere
moved, so this module computes only that geometry (reproject_motion: one float32 numpy
operation per operation of the definition, as there) and hands it to temporal.py's own
expected_temporal for the taps, the tests and the blend: while that function runs, the
module's `reproject` is replaced by one that returns the geometry computed here.
"""
import contextlib

import numpy as np

import temporal
from temporal import cameras_equal, reproject

F = np.float32


def motion_table(centers, radii, prev_centers, prev_radii):
    """(n, 8) float32: {C.xyz, r, Cp.xyz, rp} per sphere, as the call reads it."""
    n = len(radii)
    out = np.zeros((n, 8), F)
    out[:, 0:3], out[:, 3] = np.asarray(centers, F).reshape(n, -1)[:, :3], np.asarray(radii, F)
    out[:, 4:7], out[:, 7] = np.asarray(prev_centers, F).reshape(n, -1)[:, :3], np.asarray(prev_radii, F)
    return out


def reproject_motion(feat, ids, view, eye, W, H, minv, prev_eye, motion, static):
    """(fx, fy, front, L, P, mv): temporal.reproject's geometry under the motion rule, and the
    (H, W) mask of the pixels it applies to.  front is False where Pp is not finite."""
    feat = np.ascontiguousarray(feat, F).reshape(H, W, 2, 4)
    ids = np.ascontiguousarray(ids, np.uint32).reshape(H, W)
    motion = np.ascontiguousarray(motion, F).reshape(-1, 8)
    n = len(motion)
    fx, fy, front, L, P = reproject(feat, view, eye, W, H, minv, prev_eye, False)
    hit = feat[:, :, 0, 3] > 0
    ys, xs = np.mgrid[0:H, 0:W]
    in_table = ids < n
    mv = np.zeros((H, W), bool)
    if n:
        with np.errstate(all="ignore"):
            rec = motion[np.where(in_table, ids, 0)]  # no record is read for id >= n
            C, r, Cp, rp = rec[..., 0:3], rec[..., 3], rec[..., 4:7], rec[..., 7]
            unmoved = (C[..., 0] == Cp[..., 0]) & (C[..., 1] == Cp[..., 1]) & (C[..., 2] == Cp[..., 2]) & (r == rp)
            mv = hit & in_table & ~unmoved
            Ep = np.asarray(prev_eye, F).reshape(-1)[:3]
            Mi = np.asarray(minv, F).reshape(9)
            s = rp / r
            u = [P[..., i] - C[..., i] for i in range(3)]
            us = [u[i] * s for i in range(3)]
            Pp = [Cp[..., i] + us[i] for i in range(3)]
            finite = np.isfinite(Pp[0]) & np.isfinite(Pp[1]) & np.isfinite(Pp[2])
            w = [Pp[i] - Ep[i] for i in range(3)]
            Lm = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
            q = [(Mi[3 * i] * w[0] + Mi[3 * i + 1] * w[1]) + Mi[3 * i + 2] * w[2] for i in range(3)]
            a, b = q[0] / q[2], q[1] / q[2]
            fxm = ((a + F(1.0)) * F(0.5)) * F(H)
            fym = ((b + F(1.0)) * F(0.5)) * F(W)
            for v in (s, Lm, fxm, fym, *us, *Pp, *w, *q):
                assert v.dtype == F
            fx, fy, L = np.where(mv, fxm, fx), np.where(mv, fym, fy), np.where(mv, Lm, L)
            front = np.where(mv, (q[2] > 0) & finite, front)
    if static:  # per pixel: the cameras compare equal and the pixel's sphere did not move
        fx, fy = np.where(mv, fx, xs.astype(F)), np.where(mv, fy, ys.astype(F))
        front = np.where(mv, front, True)
    assert fx.dtype == F and fy.dtype == F and L.dtype == F
    return fx, fy, front, L, P, mv


@contextlib.contextmanager
def _geometry(geo):
    """temporal.expected_temporal with `geo` as its reprojection."""
    saved = temporal.reproject
    temporal.reproject = lambda *a, **k: geo
    try:
        yield
    finally:
        temporal.reproject = saved


def expected_temporal_motion(rgba, mom, feat, ids, view, eye, W, H, motion, history=None, prev_view=None, prev_eye=None,
                             minv=None, tol_normal=0.25, tol_depth=0.1, max_history=64.0):
    """temporal.expected_temporal's arguments and `motion`, the (n, 8) table ((0, 8) or None:
    no sphere is in it).  Returns (out_rgba, out_mom, info), info expected_temporal's with
    "mv", the (H, W) mask of the pixels the motion rule applies to."""
    motion = np.zeros((0, 8), F) if motion is None else np.ascontiguousarray(motion, F).reshape(-1, 8)
    kw = dict(tol_normal=tol_normal, tol_depth=tol_depth, max_history=max_history)
    if history is None:
        out, out_mom, info = temporal.expected_temporal(rgba, mom, feat, ids, view, eye, W, H, **kw)
        info["mv"] = np.zeros((H, W), bool)
        return out, out_mom, info
    static = cameras_equal(view, eye, prev_view, prev_eye)
    geo = reproject_motion(feat, ids, view, eye, W, H, minv, prev_eye, motion, static)
    with _geometry(geo[:5]):
        out, out_mom, info = temporal.expected_temporal(rgba, mom, feat, ids, view, eye, W, H, history, prev_view, prev_eye,
                                                        minv, **kw)
    info["mv"] = geo[5]
    return out, out_mom, info
