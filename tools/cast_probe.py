#!/usr/bin/env python3
"""Rate of the standalone ray-query kernels (spt_cast_rays_async) beside the render's own
cast rate on the same scene, in the same process.

    python tools/cast_probe.py [--scene c2|stress10k|both] [--rays 4194304] [--repeats 3]

Per scene and repeat: 2^22 rays, half from sphere surfaces into the outward or inward
hemisphere and half from the default eye toward points near sphere centres (kinds A and B
of tests/test_gpu_cast.py), resident on the device; two warm-up launches, then launches
timed with device events until at least 0.5 s of them have run: the index alone, with
the hit records, and the same rays sorted by kind and sphere (coherent waves).  The
yardstick is the render of the same scene (config 2: 1200 x 800 x 100 spp, depth 50; the
stress scene: 1200 x 800 x 16 spp) timed by the library's own events: stats.casts /
stats.render_ms.  The render overlaps its casts with shading and the sampler, so its
rate is a yardstick, not a bound.  One JSON line per scene on stdout.  Needs a GPU; there
is no fallback.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"c2": ("random", 100), "stress10k": ("stress10k", 16)}  # scene, spp of the yardstick render
W, H, DEPTH = 1200, 800, 50
MIN_TIMED_S = 0.5


def make_scene(spt, name):
    return spt.generate_spheres(1) if name == "random" else spt.generate_stress(1, 10000)


def unit(rng, n):
    v = rng.normal(size=(n, 3)).astype(np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def mixed_rays(scene, eye, n, seed=1):
    """Kinds A and B, interleaved at random: (o, d) float32 (n, 4), w = 0, and the order
    that sorts them by kind and sphere."""
    rng = np.random.default_rng(seed)
    C, R = scene.centers[:, :3].astype(np.float32), scene.radii.astype(np.float32)
    j = rng.integers(0, len(R), n)
    nrm, dd = unit(rng, n), unit(rng, n)
    dd = np.where((np.sum(dd * nrm, axis=1) > 0)[:, None], dd, -dd)
    dd = np.where((rng.random(n) < 0.5)[:, None], dd, -dd)
    oa = C[j] + R[j, None] * nrm
    u = unit(rng, n) * np.cbrt(rng.random(n, dtype=np.float32))[:, None]
    t = C[j] + np.float32(1.2) * R[j, None] * u - eye
    db = t / np.linalg.norm(t, axis=1, keepdims=True)
    a = (rng.random(n) < 0.5)[:, None]
    o4, d4 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    o4[:, :3] = np.where(a, oa, eye)
    d4[:, :3] = np.where(a, dd, db)
    # the same rays grouped by kind and by the sphere they start on / aim at: coherent waves
    return o4, d4, np.lexsort((j, a[:, 0]))


def timed_casts(torch, ctx, to, td, ti, th, stream):
    """Mrays/s over >= MIN_TIMED_S of launches (device events), after two warm-up launches."""
    n = to.shape[0]

    def launch(k):
        for _ in range(k):
            ctx.cast_rays_async(to.data_ptr(), td.data_ptr(), n, ti.data_ptr(), th.data_ptr() if th is not None else 0,
                                stream.cuda_stream)

    def span(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        launch(k)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    launch(2)
    stream.synchronize()
    k, s = 1, span(1)
    while s < MIN_TIMED_S:  # (a lone launch is slower than its share of a queue of them)
        k = max(k + 1, math.ceil(1.2 * k * MIN_TIMED_S / max(s, 1e-6)))
        s = span(k)
    return n * k / s / 1e6, k, s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="both", choices=["c2", "stress10k", "both"])
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("cast_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    eye = np.asarray(spt.scene.DEFAULT_EYE, np.float32)[:3]
    for key in (("c2", "stress10k") if args.scene == "both" else (args.scene,)):
        name, spp = SCENES[key]
        scene = make_scene(spt, name)
        o, d, order = mixed_rays(scene, eye, args.rays)
        ctx = spt.Context(0)
        ctx.set_scene(scene)
        ctx.set_camera(spt.camera_basis(), spt.scene.DEFAULT_EYE, spt.INIT_COLOR)
        ctx.set_params(W, H, spp, DEPTH, 1)
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        so, sd = torch.from_numpy(o[order]).to(dev), torch.from_numpy(d[order]).to(dev)
        ti = torch.zeros(args.rays, dtype=torch.int32, device=dev)
        th = torch.zeros((args.rays, 2, 4), dtype=torch.float32, device=dev)
        frame = torch.zeros((W * H, 4), dtype=torch.float32, device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        reps = []
        for _ in range(args.repeats):
            idx_rate, k, s = timed_casts(torch, ctx, to, td, ti, None, stream)
            hit_rate, _, _ = timed_casts(torch, ctx, to, td, ti, th, stream)
            sorted_rate, _, _ = timed_casts(torch, ctx, so, sd, ti, None, stream)
            # the yardstick: one warm frame, then one timed by the library's events
            for timed in (False, True):
                ctx.reset_stats()
                ctx.render_rows_async(0, 0, H, 1, 1, 0, 0, W, d_rgba=frame.data_ptr(), stream=stream.cuda_stream)
                ctx.synchronize()
            st = ctx.stats()
            reps.append({"cast_mrays_s": round(idx_rate, 1), "cast_hits_mrays_s": round(hit_rate, 1),
                         "cast_sorted_mrays_s": round(sorted_rate, 1),
                         "launches_timed": k, "timed_s": round(s, 3),
                         "render_mrays_s": round(st["casts"] / st["render_ms"] / 1e3, 1),
                         "render_ms": round(st["render_ms"], 3), "render_casts": st["casts"]})
        hits = float((ti.cpu().numpy().view(np.uint32) < scene.n).mean())
        ctx.close()

        def spread(k):
            v = [r[k] for r in reps]
            return {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)}

        print(json.dumps({"scene": key, "spheres": scene.n, "rays": args.rays, "hit_share": round(hits, 3),
                          "render": f"{W}x{H}x{spp} spp, depth {DEPTH}",
                          "cast_mrays_s": spread("cast_mrays_s"), "cast_hits_mrays_s": spread("cast_hits_mrays_s"),
                          "cast_sorted_mrays_s": spread("cast_sorted_mrays_s"),
                          "render_mrays_s": spread("render_mrays_s"), "repeats": reps}), flush=True)


if __name__ == "__main__":
    main()
