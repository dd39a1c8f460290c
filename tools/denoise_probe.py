#!/usr/bin/env python3
"""Device time of the denoiser (spt_denoise_async) per level on config 2's frame, beside the
feature buffers and the render of the same frame, in one process.

    python tools/denoise_probe.py [--spp 8] [--levels 5] [--repeats 3]

The frame is config 2's, 1200 x 800, the 149-sphere scene, default camera, rendered at --spp
samples (a preview: what the filter is for); its feature buffers are spt_render_features'.

    (a) denoise L       spt_denoise_async at L = 1 .. --levels levels, float output, device
                        pointers.  A call launches its levels back to back on the stream, so
                        level k's own time is the difference (a)[k + 1] - (a)[k].
    (b) features        spt_render_features_async of the same frame
    (c) render          spt_render_rows_async of the same frame

Per repeat: two warm-up calls, then calls timed with device events on a stream of the
caller's until at least 0.5 s of them have run.  A level moves at least 48 B read and 16 B
written per pixel (61.4 MB here): `gbs` is that over the level's time, `of_peak` its share of
the 8.0 TB/s HBM3E peak.  The 3-level answer is compared bit for bit with the blocking form's.
One JSON line on stdout.  Needs a GPU; there is no fallback.
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
LEVEL_BYTES = 64 * W * H  # the least a level moves: rgba + feat in, rgba out
HBM_PEAK = 8.0e12


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
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("denoise_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    scene = spt.generate_spheres(1)
    ctx = spt.Context(0)
    ctx.set_scene(scene)
    ctx.set_camera(spt.camera_basis(), spt.scene.DEFAULT_EYE, spt.INIT_COLOR)
    ctx.set_params(W, H, args.spp, DEPTH, SEED)
    npix = W * H
    frame = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    feat = torch.zeros((npix, 2, 4), dtype=torch.float32, device=dev)
    out = torch.zeros_like(frame)
    scratch = torch.zeros(max(spt.denoise_scratch_bytes(W, H, args.levels) // 4, 1), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def render():
        ctx.render_rows_async(0, 0, H, 1, 1, 0, 0, W, d_rgba=frame.data_ptr(), stream=stream.cuda_stream)

    def features():
        ctx.render_features_async(0, H, 1, 1, 0, 0, W, feat.data_ptr(), 0, stream.cuda_stream)

    def denoise(levels):
        ctx.denoise_async(W, H, frame.data_ptr(), feat.data_ptr(), levels=levels, d_out=out.data_ptr(),
                          d_scratch=scratch.data_ptr(), stream=stream.cuda_stream)

    reps = []
    for _ in range(args.repeats):
        t_c = timed(torch, stream, render)
        t_b = timed(torch, stream, features)
        t_a = [timed(torch, stream, lambda n=n: denoise(n)) for n in range(1, args.levels + 1)]
        reps.append({"render_ms": round(t_c * 1e3, 3), "features_ms": round(t_b * 1e3, 3),
                     "denoise_ms": [round(t * 1e3, 4) for t in t_a]})
    denoise(min(3, args.levels))
    stream.synchronize()
    h_frame, h_feat = frame.cpu().numpy().reshape(H, W, 4), feat.cpu().numpy()
    same = bool(np.array_equal(out.cpu().numpy().reshape(H, W, 4).view(np.uint32),
                               ctx.denoise(h_frame, h_feat, levels=min(3, args.levels)).view(np.uint32)))
    moved = float((out.cpu().numpy()[:, :3] != h_frame.reshape(-1, 4)[:, :3]).any(axis=1).mean())
    ctx.close()

    def median(v):
        return sorted(v)[len(v) // 2]

    total = [median([r["denoise_ms"][k] for r in reps]) for k in range(args.levels)]
    per_level = [round(total[k] - (total[k - 1] if k else 0.0), 4) for k in range(args.levels)]
    print(json.dumps({"scene": "c2", "spheres": scene.n, "frame": f"{W}x{H}x{args.spp} spp", "level_bytes": LEVEL_BYTES,
                      "denoise_total_ms": total, "level_ms": per_level,
                      "level_gbs": [round(LEVEL_BYTES / (t * 1e-3) / 1e9, 1) if t > 0 else None for t in per_level],
                      "level_of_peak": [round(LEVEL_BYTES / (t * 1e-3) / HBM_PEAK, 3) if t > 0 else None for t in per_level],
                      "features_ms": median([r["features_ms"] for r in reps]),
                      "render_ms": median([r["render_ms"] for r in reps]),
                      "async_equals_blocking": same, "pixels_changed": round(moved, 4), "repeats": reps}), flush=True)


if __name__ == "__main__":
    main()
