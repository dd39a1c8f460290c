#!/usr/bin/env python3
"""Time of config 2's feature frame (spt_render_features_async) beside the render of the same
frame and the host-composed route it replaces, in one process.

    python tools/features_probe.py [--spp 100] [--repeats 3] [--hits-spp 4]

The frame is config 2's: 1200 x 800 at 100 spp, the 149-sphere scene, default camera.

    (a) features        spt_render_features_async, feat and ids, whole frame, device pointers
    (b) features_walk   the same on a context created with SPT_PRIM_LISTS=0: every primary
                        batch walks the tree instead of testing its block's candidate list
    (c) render          spt_render_rows_async of the same frame (render + fold launches)
    (d) primary_hits    spt_primary_hits with hit records over every (x, y, s) triple of the
                        frame at --hits-spp samples: host arrays in and out, blocking, wall
                        clock.  It grows with the sample count: scale by spp / hits-spp
                        (plus the per-pixel sums, left to the caller) to compare with (a).

(a)-(c) per repeat: two warm-up launches, then launches timed with device events on a
stream of the caller's until at least 0.5 s of them have run.  (a) and (b) are compared
bit for bit.  One JSON line on stdout.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, DEPTH, SEED = 1200, 800, 50, 1
MIN_TIMED_S = 0.5


def timed(torch, stream, launch):
    """Seconds per launch over >= MIN_TIMED_S of launches (device events), after two warm-ups."""
    def span(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(k):
            launch()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    launch()
    launch()
    stream.synchronize()
    k, s = 1, span(1)
    while s < MIN_TIMED_S:  # (a lone launch is slower than its share of a queue of them)
        k = max(k + 1, math.ceil(1.2 * k * MIN_TIMED_S / max(s, 1e-6)))
        s = span(k)
    return s / k


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--spp", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hits-spp", type=int, default=4)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("features_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    scene = spt.generate_spheres(1)

    def context(lists):
        old = os.environ.get("SPT_PRIM_LISTS")
        if not lists:
            os.environ["SPT_PRIM_LISTS"] = "0"  # read when the context is created
        try:
            ctx = spt.Context(0)
        finally:
            if not lists:
                os.environ.pop("SPT_PRIM_LISTS")
                if old is not None:
                    os.environ["SPT_PRIM_LISTS"] = old
        ctx.set_scene(scene)
        ctx.set_camera(spt.camera_basis(), spt.scene.DEFAULT_EYE, spt.INIT_COLOR)
        ctx.set_params(W, H, args.spp, DEPTH, SEED)
        assert (ctx.stats()["prim_list_blocks"] > 0) == lists
        return ctx

    ctx, ctx_walk = context(True), context(False)
    npix = W * H
    feat = torch.zeros((npix, 2, 4), dtype=torch.float32, device=dev)
    feat_walk = torch.zeros_like(feat)
    ids = torch.zeros(npix, dtype=torch.int32, device=dev)
    ids_walk = torch.zeros_like(ids)
    frame = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def features(c, f, i):
        c.render_features_async(0, H, 1, 1, 0, 0, W, f.data_ptr(), i.data_ptr(), stream.cuda_stream)

    def render():
        ctx.render_rows_async(0, 0, H, 1, 1, 0, 0, W, d_rgba=frame.data_ptr(), stream=stream.cuda_stream)

    ys, xs = np.mgrid[0:H, 0:W]
    xys = np.stack([np.repeat(xs.ravel(), args.hits_spp), np.repeat(ys.ravel(), args.hits_spp),
                    np.tile(np.arange(args.hits_spp), npix)], axis=1).astype(np.uint32)
    reps = []
    for _ in range(args.repeats):
        t_a = timed(torch, stream, lambda: features(ctx, feat, ids))
        t_b = timed(torch, stream, lambda: features(ctx_walk, feat_walk, ids_walk))
        t_c = timed(torch, stream, render)
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.primary_hits(xys, hits=True)
        t_d = time.perf_counter() - t0
        reps.append({"features_ms": round(t_a * 1e3, 3), "features_walk_ms": round(t_b * 1e3, 3),
                     "render_ms": round(t_c * 1e3, 3), "primary_hits_ms": round(t_d * 1e3, 1)})
    same = bool(torch.equal(feat.view(torch.int32), feat_walk.view(torch.int32)) and torch.equal(ids, ids_walk))
    cov = float(feat[:, 0, 3].mean())
    ctx.close()
    ctx_walk.close()

    def spread(key):
        v = [r[key] for r in reps]
        return {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)}

    rays = npix * args.spp
    a = spread("features_ms")
    print(json.dumps({"scene": "c2", "spheres": scene.n, "frame": f"{W}x{H}x{args.spp} spp", "primary_rays": rays,
                      "features_ms": a, "features_grays_s": round(rays / a["median"] / 1e6, 2),
                      "features_walk_ms": spread("features_walk_ms"), "render_ms": spread("render_ms"),
                      "primary_hits_spp": args.hits_spp, "primary_hits_ms": spread("primary_hits_ms"),
                      "primary_hits_bytes": {"up": 12 * npix * args.hits_spp, "down": 36 * npix * args.hits_spp},
                      "features_bytes_down": 36 * npix, "lists_equal_walk": same, "mean_coverage": round(cov, 4),
                      "repeats": reps}), flush=True)


if __name__ == "__main__":
    main()
