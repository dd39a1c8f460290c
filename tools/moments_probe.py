#!/usr/bin/env python3
"""Device time of the sample-moments pass (spt_render_moments_async) and of the
variance-guided filter (spt_denoise_var_async) per level on config 2's frame, beside the
fold of the same run and the plain filter, in one process.

    python tools/moments_probe.py [--spp 4,100] [--levels 3] [--repeats 3]

The frame is config 2's, 1200 x 800, the 149-sphere scene, default camera.  Per sample count:

    (a) render          spt_render_rows_async of the frame (render + fold)
    (b) moments         spt_render_moments_async of the frame (render + fold + moments pass):
                        the moments pass's own time is (b) - (a); `fold_ms` is spt_stats'
                        fold time per launch over the very launches of (b)
    (c) denoise_var L   spt_denoise_var_async at L = 1 .. --levels levels (first sample count
    (d) denoise L       only: the filters' time does not depend on it); a call launches its
                        levels back to back, so level k's own time is the difference of
                        consecutive totals

Per repeat: two warm-up calls, then calls timed with device events on a stream of the
caller's until at least 0.5 s of them have run.  The moments pass moves 4 B per sample in and
16 B per pixel out: `moments_gbs` is that over its time.  One JSON line on stdout.  Needs a
GPU; there is no fallback.
"""
import argparse
import json
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
    ap.add_argument("--spp", default="4,100")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("moments_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    scene = spt.generate_spheres(1)
    ctx = spt.Context(0)
    ctx.set_scene(scene)
    ctx.set_camera(spt.camera_basis(), spt.scene.DEFAULT_EYE, spt.INIT_COLOR)
    npix = W * H
    frame = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    mom = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    feat = torch.zeros((npix, 2, 4), dtype=torch.float32, device=dev)
    out = torch.zeros_like(frame)
    var = torch.zeros(npix, dtype=torch.float32, device=dev)
    scratch = torch.zeros(max(spt.denoise_scratch_bytes(W, H, args.levels) // 4, 1), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def render():
        ctx.render_rows_async(0, 0, H, 1, 1, 0, 0, W, d_rgba=frame.data_ptr(), stream=stream.cuda_stream)

    def moments():
        ctx.render_moments_async(0, H, 1, 1, 0, 0, W, frame.data_ptr(), 0, mom.data_ptr(), stream.cuda_stream)

    def denoise_var(levels):
        ctx.denoise_variance_async(W, H, frame.data_ptr(), feat.data_ptr(), mom.data_ptr(), levels=levels,
                                   d_out=out.data_ptr(), d_out_var=var.data_ptr(), d_scratch=scratch.data_ptr(),
                                   stream=stream.cuda_stream)

    def denoise(levels):
        ctx.denoise_async(W, H, frame.data_ptr(), feat.data_ptr(), levels=levels, d_out=out.data_ptr(),
                          d_scratch=scratch.data_ptr(), stream=stream.cuda_stream)

    res = {"scene": "c2", "spheres": scene.n, "frame": f"{W}x{H}", "by_spp": []}
    for n, spp in enumerate(int(s) for s in args.spp.split(",")):
        ctx.set_params(W, H, spp, DEPTH, SEED)
        reps = []
        for _ in range(args.repeats):
            t_a = timed(torch, stream, render)
            ctx.synchronize()
            ctx.reset_stats()
            t_b = timed(torch, stream, moments)
            ctx.synchronize()
            st = ctx.stats()
            reps.append({"render_ms": round(t_a * 1e3, 4), "moments_call_ms": round(t_b * 1e3, 4),
                         "fold_ms": round(st["fold_ms"] / max(st["launches"], 1), 4),
                         "render_kernel_ms": round(st["render_ms"] / max(st["launches"], 1), 4)})
        t_pass = median([r["moments_call_ms"] - r["render_ms"] for r in reps])
        nbytes = 4 * npix * spp + 16 * npix
        entry = {"spp": spp, "render_ms": median([r["render_ms"] for r in reps]),
                 "moments_call_ms": median([r["moments_call_ms"] for r in reps]),
                 "moments_pass_ms": round(t_pass, 4), "moments_bytes": nbytes,
                 "moments_gbs": round(nbytes / (t_pass * 1e-3) / 1e9, 1) if t_pass > 0 else None,
                 "fold_ms": median([r["fold_ms"] for r in reps]), "repeats": reps}
        if n == 0:
            # the blocking form gives the same answer, and the filters run on this frame
            moments()
            stream.synchronize()
            h_rgba, h_mom = ctx.render_moments(0, H, 0, W)
            entry["async_equals_blocking"] = bool(np.array_equal(mom.cpu().numpy().view(np.uint32), h_mom.view(np.uint32)) and
                                                  np.array_equal(frame.cpu().numpy().view(np.uint32), h_rgba.view(np.uint32)))
            entry["variance_zero_share"] = round(float((h_mom[:, 2] == 0).mean()), 4)
            ctx.render_features_async(0, H, 1, 1, 0, 0, W, feat.data_ptr(), 0, stream.cuda_stream)
            stream.synchronize()
            freps = []
            for _ in range(args.repeats):
                freps.append({"denoise_var_ms": [round(timed(torch, stream, lambda k=k: denoise_var(k)) * 1e3, 4)
                                                 for k in range(1, args.levels + 1)],
                              "denoise_ms": [round(timed(torch, stream, lambda k=k: denoise(k)) * 1e3, 4)
                                             for k in range(1, args.levels + 1)]})
            for key in ("denoise_var_ms", "denoise_ms"):
                total = [median([r[key][k] for r in freps]) for k in range(args.levels)]
                res[key.replace("_ms", "_total_ms")] = total
                res[key.replace("_ms", "_level_ms")] = [round(total[k] - (total[k - 1] if k else 0.0), 4)
                                                        for k in range(args.levels)]
            res["filter_repeats"] = freps
        res["by_spp"].append(entry)
    ctx.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
