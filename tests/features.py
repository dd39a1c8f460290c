"""What spt_render_features must return, from the oracle alone: the expected feature
buffers of a region (include/spt_hip.h "feature buffers"), shared by the
GPU tests (tests/test_gpu_features.py).  A plain helper module: numpy and pyoracle only, it
never calls the device.

Per pixel (x, y) and sample s = 0 .. spp - 1, in this order: the ray is spo_primary_ray on
the keyed stream spo_sample_key(seed, y * W + x, s) (what sample_state gives at 0 draws),
its winner pyoracle.primary_winners', the hit record cast_rays.restate_hits' from the eye.
Every per-sample value and every sum is float32, one numpy operation per operation of the
definition (no operation here can contract).
"""
import ctypes

import numpy as np

from cast_rays import restate_hits

SKYBOX, REFLECTIVE, REFRACTIVE, DIFFUSE = 0, 1, 2, 3


def expected_features(oracle, osc, frame, scene_arrays, region):
    """scene_arrays: (centers (n, 4), radii, colors (n, 4), materials, fuzz) or an object
    with those attributes; region: (yB, yE, xB, xE) of `frame`.  Returns a dict:

        feat  (pixels, 2, 4) float32   [[alb r, g, b, cov], [nrm x, y, z, dep]]
        ids   (pixels,) uint32         sample 0's sphere (n = the sky)
        idx   (pixels, spp) uint32     every sample's sphere
        vals  (pixels, spp, 8) float32 the per-sample values, in feat's lane order
        mat   (pixels, spp) int        the material byte of the sphere hit, -1 on a miss

    in region-local row-major pixel order."""
    f = np.float32
    if hasattr(scene_arrays, "centers"):
        sa = scene_arrays
        scene_arrays = (sa.centers, sa.radii, sa.colors, sa.materials, sa.fuzz)
    centers, radii, colors, materials = (np.asarray(a) for a in scene_arrays[:4])
    n = len(radii)
    centers = np.asarray(centers, f).reshape(n, 4)
    colors = np.asarray(colors, f).reshape(n, 4)
    materials = np.asarray(materials, np.uint8).reshape(n)
    yB, yE, xB, xE = region
    W, S, seed = frame.width, frame.spp, frame.seed
    ys, xs = np.mgrid[yB:yE, xB:xE]
    xs, ys = xs.ravel(), ys.ravel()
    npix = len(xs)
    # (pixel, sample) pairs, samples fastest
    px, py = np.repeat(xs, S), np.repeat(ys, S)
    ps = np.tile(np.arange(S), npix)
    xys = np.stack([px, py, ps], axis=1).astype(np.uint32)
    idx = oracle.primary_winners(osc, frame, xys)
    L = oracle.lib()
    d = np.zeros((npix * S, 4), f)
    fr = ctypes.byref(frame)
    for i in range(npix * S):
        st = ctypes.c_uint64(L.spo_sample_key(seed, int(py[i]) * W + int(px[i]), int(ps[i])))
        L.spo_primary_ray(fr, int(px[i]), int(py[i]), ctypes.byref(st), d.ctypes.data + 16 * i)
    hit = idx < n
    o = np.tile(np.asarray(list(frame.eye), f), (npix * S, 1))
    t, _, nrm = restate_hits(centers, radii, idx[hit], o[hit], d[hit])
    vals = np.zeros((npix * S, 8), f)
    # the sky term, (sky_c * (d.y + 1.0f)) * 0.5f per channel
    sky = np.asarray(list(frame.sky), f)[:3]
    with np.errstate(all="ignore"):
        k = d[:, 1] + f(1.0)
        vals[:, :3] = (sky[None, :] * k[:, None]) * f(0.5)
    mat = np.full(npix * S, -1, np.int64)
    mat[hit] = materials[idx[hit]]
    dif = mat == DIFFUSE
    vals[dif, :3] = colors[idx[dif], :3]
    vals[(mat == REFLECTIVE) | (mat == REFRACTIVE), :3] = f(1.0)
    vals[hit, 3] = f(1.0)
    vals[hit, 4:7] = nrm
    vals[hit, 7] = t
    vals = vals.reshape(npix, S, 8)
    acc = np.zeros((npix, 8), f)
    with np.errstate(all="ignore"):
        for s in range(S):
            acc = acc + vals[:, s]
        acc = acc * (f(1.0) / f(S))
    assert acc.dtype == f and vals.dtype == f
    idx = idx.reshape(npix, S)
    return dict(feat=acc.reshape(npix, 2, 4), ids=idx[:, 0].copy(), idx=idx, vals=vals, mat=mat.reshape(npix, S))
