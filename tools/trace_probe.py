#!/usr/bin/env python3
"""Rate of the standalone path-query kernels (spt_trace_rays_async) on config 2's own paths,
beside the render of the same paths in the same process.

    python tools/trace_probe.py [--spp 100] [--repeats 3]

The paths are the render's: for every sample of every pixel of the 1200 x 800 frame the
primary ray the render itself forms (spt_primary_hits' dirs), from the eye, on the
sample's keyed stream two draws in (sample_state(seed, y * W + x, s, 2)), at depth 50.
They lie on the device in the render's own order, [sample][8 x 8 tile][pixel of the tile],
so a wave's first 64 rays are one sample of one tile, as a render's primary batch.  One
sample is one path, so paths/s compares directly with the render's samples/s.

Per repeat: two warm-up launches, then launches timed with device events until at least
0.5 s of them have run (trace + decode kernels, as spt_trace_rays_async enqueues them),
without and with the info words; then the yardstick, one warm frame and one timed by the
library's own events (stats.render_ms: the render kernel alone, without its fold).  One
JSON line on stdout.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, DEPTH, SEED = 1200, 800, 50, 1
MIN_TIMED_S = 0.5


def tile_order():
    """(x, y) of the frame's pixels, 8 x 8 tiles row-major, row-major inside a tile."""
    ty, tx, py, px = np.meshgrid(np.arange(H // 8), np.arange(W // 8), np.arange(8), np.arange(8), indexing="ij")
    return (tx * 8 + px).ravel().astype(np.uint32), (ty * 8 + py).ravel().astype(np.uint32)


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
    return s / k, k


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--spp", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("trace_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    scene = spt.generate_spheres(1)
    ctx = spt.Context(0)
    ctx.set_scene(scene)
    ctx.set_camera(spt.camera_basis(), spt.scene.DEFAULT_EYE, spt.INIT_COLOR)
    ctx.set_params(W, H, args.spp, DEPTH, SEED)

    x, y = tile_order()
    npix, n = W * H, W * H * args.spp
    td = torch.empty((n, 4), dtype=torch.float32, device=dev)
    ts = torch.empty(n, dtype=torch.int64, device=dev)
    to = torch.from_numpy(np.asarray(spt.scene.DEFAULT_EYE, np.float32)).to(dev).repeat(n, 1)
    for s in range(args.spp):
        xys = np.stack([x, y, np.full(npix, s, np.uint32)], axis=1)
        _, dirs = ctx.primary_hits(xys, dirs=True)
        td[s * npix:(s + 1) * npix] = torch.from_numpy(dirs).to(dev)
        ts[s * npix:(s + 1) * npix] = torch.from_numpy(spt.sample_state(SEED, y * W + x, s, 2).view(np.int64)).to(dev)
    rgba = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    info = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    frame = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def launch(with_info):
        ctx.trace_rays_async(to.data_ptr(), td.data_ptr(), ts.data_ptr(), n, DEPTH, rgba.data_ptr(),
                             info.data_ptr() if with_info else 0, stream.cuda_stream)

    reps = []
    for _ in range(args.repeats):
        t_plain, k = timed(torch, stream, lambda: launch(False))
        t_info, _ = timed(torch, stream, lambda: launch(True))
        for _timed in (False, True):  # the yardstick: one warm frame, then one timed
            ctx.reset_stats()
            ctx.render_rows_async(0, 0, H, 1, 1, 0, 0, W, d_rgba=frame.data_ptr(), stream=stream.cuda_stream)
            ctx.synchronize()
        st = ctx.stats()
        reps.append({"trace_ms": round(t_plain * 1e3, 3), "trace_mpaths_s": round(n / t_plain / 1e6, 1),
                     "trace_info_ms": round(t_info * 1e3, 3), "trace_info_mpaths_s": round(n / t_info / 1e6, 1),
                     "launches_timed": k, "render_ms": round(st["render_ms"], 3),
                     "render_msamples_s": round(st["samples"] / st["render_ms"] / 1e3, 1), "render_casts": st["casts"]})
    # the traced paths are the render's: their casts are its casts, their mean its frame
    inf = info.cpu().numpy().view(np.uint32)
    casts = int(inf[:, 0].sum(dtype=np.uint64))
    acc = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    for s in range(args.spp):  # RenderSegment's sum in sample order, then * 1 / spp
        acc += rgba[s * npix:(s + 1) * npix]
    mean = (acc * np.float32(1.0 / args.spp)).cpu().numpy()
    order = (y.astype(np.int64) * W + x)
    same = bool(np.array_equal(mean[:, :3].view(np.uint32), frame.cpu().numpy()[order, :3].view(np.uint32)))
    ctx.close()

    def spread(key):
        v = [r[key] for r in reps]
        return {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)}

    print(json.dumps({"scene": "c2", "spheres": scene.n, "paths": n, "frame": f"{W}x{H}x{args.spp} spp, depth {DEPTH}",
                      "bytes_per_path": {"read": 40, "written": 16, "info": 8},
                      "trace_mpaths_s": spread("trace_mpaths_s"), "trace_info_mpaths_s": spread("trace_info_mpaths_s"),
                      "render_msamples_s": spread("render_msamples_s"), "trace_casts": casts,
                      "casts_equal_render": casts == reps[-1]["render_casts"], "mean_equals_frame": same,
                      "repeats": reps}), flush=True)


if __name__ == "__main__":
    main()
