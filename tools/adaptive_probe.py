#!/usr/bin/env python3
"""Device and wall time of adaptive sampling (spt_render_adaptive_dev) on config 2's frame,
pass by pass, beside plain renders of the same frame, in one process.

    python tools/adaptive_probe.py [--base 16] [--step 16] [--max 100] [--tol 0.08] [--floor 1.0] [--repeats 3]

The frame is config 2's, 1200 x 800, depth 50, the 149-sphere scene, default camera.

    (a) adaptive        the call at the given parameters: wall time per call (it waits on the
                        stream once per pass), spt_stats' render and fold time over the call's
                        own launches, mean spp, tiles active per pass (from mom.w)
    (b) passes          the same call cut off after pass k (max_spp = the samples pass k ends
                        at), k = 0, 1, ...: the keyed samples make its passes the full call's
                        first k + 1, so pass k's own time is the difference of consecutive
                        totals -- wall, render kernel and fold kernel; what is left of the
                        wall time is the plan kernel, the host's wait and the launch gaps
    (c) plain           spt_render_rows_async of the frame at max_spp, at ceil(mean spp) and
                        at base_spp (render + fold), and spt_render_moments_async at base_spp
                        (render + fold + moments: what pass 0 replaces)

Per repeat: two warm-up calls, then calls timed until at least 0.5 s of them have run
(tools/denoise_probe.py's `timed`).  One JSON line on stdout.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from denoise_probe import timed  # noqa: E402

W, H, DEPTH, SEED = 1200, 800, 50, 1


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", type=int, default=16)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--max", type=int, default=100)
    ap.add_argument("--tol", type=float, default=0.08)
    ap.add_argument("--floor", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("adaptive_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    scene = spt.generate_spheres(1)
    ctx = spt.Context(0)
    ctx.set_scene(scene)
    ctx.set_camera(spt.camera_basis(), spt.scene.DEFAULT_EYE, spt.INIT_COLOR)
    ctx.set_params(W, H, args.base, DEPTH, SEED)
    npix = W * H
    frame = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    mom = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def adaptive(mx):
        return ctx.render_adaptive_dev(0, H, 0, W, args.base, args.step, mx, args.tol, args.floor, rgba=frame, mom=mom,
                                       stream=stream.cuda_stream)

    def measure(launch):
        """median over the repeats of (wall ms, render kernel ms, fold kernel ms) per call"""
        reps = []
        for _ in range(args.repeats):
            ctx.synchronize()
            ctx.reset_stats()
            t = timed(torch, stream, launch)
            ctx.synchronize()
            st = ctx.stats()
            calls = st["launches"] / per_call["launches"] if per_call["launches"] else 1
            reps.append((t * 1e3, st["render_ms"] / calls, st["fold_ms"] / calls))
        return [round(median([r[k] for r in reps]), 4) for k in range(3)]

    def rays(launch):
        """(samples, rays cast) of one call, from spt_stats' device counters"""
        ctx.synchronize()
        ctx.reset_stats()
        launch()
        stream.synchronize()
        ctx.synchronize()
        st = ctx.stats()
        return {"samples": st["samples"], "casts": st["casts"], "casts_per_sample": round(st["casts"] / max(st["samples"], 1), 3)}

    # (a) the full call, and the spp map it leaves
    info = adaptive(args.max)
    stream.synchronize()
    n_pix = mom.cpu().numpy()[:, 3].astype(np.int64).reshape(H, W)
    tiles = n_pix[::8, ::8]
    ends = [args.base]
    while ends[-1] < args.max:
        ends.append(min(ends[-1] + args.step, args.max))
    active = [int((tiles >= e).sum()) for e in ends[:info["passes"]]]
    mean_spp = float(n_pix.mean())
    per_call = {"launches": info["passes"]}
    wall, render_ms, fold_ms = measure(lambda: adaptive(args.max))
    res = {"scene": "c2", "spheres": scene.n, "frame": f"{W}x{H}", "depth": DEPTH,
           "params": {"base": args.base, "step": args.step, "max": args.max, "tol": args.tol, "floor": args.floor},
           "adaptive": {"wall_ms": wall, "render_kernel_ms": render_ms, "fold_kernel_ms": fold_ms,
                        "other_ms": round(wall - render_ms - fold_ms, 4), "passes": info["passes"], "samples": info["samples"],
                        "mean_spp": round(mean_spp, 3), "tiles": int(tiles.size), "active_tiles": active,
                        "work": rays(lambda: adaptive(args.max))}}

    # (b) pass by pass: the call cut off after pass k
    res["passes"] = []
    prev, prev_casts = (0.0, 0.0, 0.0), 0
    for k in range(info["passes"]):
        per_call = {"launches": k + 1}
        tot = measure(lambda: adaptive(ends[k]))
        casts = rays(lambda: adaptive(ends[k]))["casts"]
        take = ends[k] - (ends[k - 1] if k else 0)
        words = active[k] * 64 * take  # (edge tiles hold fewer: an upper bound)
        own = [round(a - b, 4) for a, b in zip(tot, prev)]
        res["passes"].append({"pass": k, "n_end": ends[k], "take": take, "active_tiles": active[k], "total_ms": tot,
                              "wall_ms": own[0], "render_kernel_ms": own[1], "fold_kernel_ms": own[2],
                              "other_ms": round(own[0] - own[1] - own[2], 4),
                              "fold_ns_per_word": round(own[2] * 1e6 / words, 4) if words else None,
                              "casts": casts - prev_casts, "casts_per_sample": round((casts - prev_casts) / words, 3)})
        prev, prev_casts = tot, casts

    # (c) plain renders of the same frame
    res["plain"] = {}
    per_call = {"launches": 1}
    for name, spp in (("max", args.max), ("mean", math.ceil(mean_spp)), ("base", args.base)):
        ctx.set_params(W, H, spp, DEPTH, SEED)
        w_, r_, f_ = measure(lambda: ctx.render_rows_async(0, 0, H, 1, 1, 0, 0, W, d_rgba=frame.data_ptr(),
                                                           stream=stream.cuda_stream))
        res["plain"][name] = {"spp": spp, "wall_ms": w_, "render_kernel_ms": r_, "fold_kernel_ms": f_,
                              "fold_ns_per_word": round(f_ * 1e6 / (npix * spp), 4),
                              "work": rays(lambda: ctx.render_rows_async(0, 0, H, 1, 1, 0, 0, W, d_rgba=frame.data_ptr(),
                                                                         stream=stream.cuda_stream))}
    ctx.set_params(W, H, args.base, DEPTH, SEED)
    w_, r_, f_ = measure(lambda: ctx.render_moments_async(0, H, 1, 1, 0, 0, W, frame.data_ptr(), 0, mom.data_ptr(),
                                                          stream.cuda_stream))
    res["plain"]["moments_base"] = {"spp": args.base, "wall_ms": w_, "render_kernel_ms": r_, "fold_kernel_ms": f_,
                                    "fold_plus_moments_ms": round(w_ - r_, 4),
                                    "fold_plus_moments_ns_per_word": round((w_ - r_) * 1e6 / (npix * args.base), 4)}
    p0 = res["passes"][0]
    res["ratios"] = {
        "pass0_wall_over_plain_base_wall": round(p0["wall_ms"] / res["plain"]["base"]["wall_ms"], 3),
        "pass0_render_kernel_over_plain_base": round(p0["render_kernel_ms"] / res["plain"]["base"]["render_kernel_ms"], 3),
        "adaptive_fold_over_fold_plus_moments": round(p0["fold_kernel_ms"] / res["plain"]["moments_base"]["fold_plus_moments_ms"], 3),
        "adaptive_wall_over_plain_max": round(wall / res["plain"]["max"]["wall_ms"], 3),
        "adaptive_wall_over_plain_mean": round(wall / res["plain"]["mean"]["wall_ms"], 3),
    }
    ctx.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
