#!/usr/bin/env python3
"""Device time of the temporal accumulation (spt_temporal_async) on config 2's frame, for a
camera that stands still and one that moves, beside a device-to-device copy of the bytes the
call must move, in one process.

    python tools/temporal_probe.py [--spp 4] [--repeats 3]

The frames are config 2's, 1200 x 800, the 149-sphere scene at --spp samples (a preview: what
the accumulation is for): frame A from the default camera, frame B from an eye moved by
[0.15, 0.05, 0.1] that looks about 2 degrees to the side, each with its moments, feature
buffers and ids, all device-resident.

    (a) static          B against a history B seen by the same camera: the static rule, every
                        pixel's four taps collapse onto its own place
    (b) moved           B against the history A: the general path
    (c) no history      B alone: the outputs are copies
    (d) copy            one hipMemcpyAsync device to device that moves what a call must move:
                        68 B in, 68 B of history in and 32 B out per pixel, 168 B, as 84 B read
                        and 84 B written per pixel -- the floor

Per repeat: two warm-up calls, then calls timed with device events on a stream of the caller's
until at least 0.5 s of them have run.  `gbs` is 168 B per pixel over the call's time (100 B for
(c)), `of_copy` the call's time over the copy's.  The moved answer is compared bit for bit with
the blocking form's.  One JSON line on stdout.  Needs a GPU; there is no fallback.
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
CALL_BYTES = 168 * W * H  # rgba, mom, feat, ids in (68), the history's same (68), two float4 out (32)
EYE_B, LOOK_B = (0.15, 1.05, -2.9, 0.0), (0.255, 1.05, 0.1, 0.0)  # atan(0.105 / 3) = 2 degrees


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
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("temporal_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    scene = spt.generate_spheres(1)
    ctx = spt.Context(0)
    ctx.set_scene(scene)
    npix = W * H
    cams = [(spt.camera_basis(), np.asarray(spt.scene.DEFAULT_EYE, np.float32)),
            (spt.camera_basis(EYE_B, LOOK_B), np.asarray(EYE_B, np.float32))]
    frames = []
    for k, (view, eye) in enumerate(cams):
        ctx.set_camera(view, eye, spt.INIT_COLOR)
        ctx.set_params(W, H, args.spp, DEPTH, SEED + k)
        f = dict(rgba=torch.zeros((npix, 4), dtype=torch.float32, device=dev), mom=torch.zeros((npix, 4), dtype=torch.float32, device=dev),
                 feat=torch.zeros((npix, 2, 4), dtype=torch.float32, device=dev), ids=torch.zeros(npix, dtype=torch.int32, device=dev))
        torch.cuda.synchronize(dev)
        ctx.render_moments_async(0, H, 1, 1, 0, 0, W, d_rgba=f["rgba"].data_ptr(), d_mom=f["mom"].data_ptr(), stream=stream.cuda_stream)
        ctx.render_features_async(0, H, 1, 1, 0, 0, W, f["feat"].data_ptr(), f["ids"].data_ptr(), stream.cuda_stream)
        stream.synchronize()
        frames.append(f)
    a, b = frames
    out = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    out_mom = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    src = torch.zeros(npix * 84, dtype=torch.uint8, device=dev)
    dst = torch.zeros_like(src)
    torch.cuda.synchronize(dev)

    def ptrs(f):
        return tuple(f[k].data_ptr() for k in ("rgba", "mom", "feat", "ids"))

    def temporal(hist, prev_cam):
        ctx.temporal_async(W, H, *ptrs(b), cams[1][0], cams[1][1], ptrs(hist) if hist is not None else None,
                           prev_cam[0] if hist is not None else None, prev_cam[1] if hist is not None else None,
                           d_out_rgba=out.data_ptr(), d_out_mom=out_mom.data_ptr(), stream=stream.cuda_stream)

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src, non_blocking=True)

    reps = []
    for _ in range(args.repeats):
        t = {"static_ms": timed(torch, stream, lambda: temporal(b, cams[1])),
             "moved_ms": timed(torch, stream, lambda: temporal(a, cams[0])),
             "no_history_ms": timed(torch, stream, lambda: temporal(None, None)),
             "copy_ms": timed(torch, stream, copy)}
        reps.append({k: round(v * 1e3, 4) for k, v in t.items()})
    temporal(a, cams[0])
    stream.synchronize()
    h = {k: [f[k].cpu().numpy() for f in frames] for k in ("rgba", "mom", "feat", "ids")}
    blocking = ctx.temporal(h["rgba"][1].reshape(H, W, 4), h["mom"][1], h["feat"][1], h["ids"][1].view(np.uint32), cams[1][0],
                            cams[1][1], (h["rgba"][0], h["mom"][0], h["feat"][0], h["ids"][0].view(np.uint32)), cams[0][0],
                            cams[0][1])
    got_mom = out_mom.cpu().numpy()
    same = bool(np.array_equal(out.cpu().numpy().view(np.uint32), blocking[0].reshape(-1, 4).view(np.uint32)) and
                np.array_equal(got_mom.view(np.uint32), blocking[1].reshape(-1, 4).view(np.uint32)))
    history = float((got_mom[:, 3] > h["mom"][1][:, 3]).mean())
    ctx.close()

    def median(key):
        v = sorted(r[key] for r in reps)
        return v[len(v) // 2]

    ms = {k: median(k) for k in ("static_ms", "moved_ms", "no_history_ms", "copy_ms")}
    res = {"scene": "c2", "spheres": scene.n, "frame": f"{W}x{H}x{args.spp} spp", "call_bytes": CALL_BYTES, **ms}
    for k, nbytes in (("static", CALL_BYTES), ("moved", CALL_BYTES), ("no_history", 100 * npix), ("copy", CALL_BYTES)):
        res[f"{k}_gbs"] = round(nbytes / (ms[f"{k}_ms"] * 1e-3) / 1e9, 1)
    for k in ("static", "moved"):
        res[f"{k}_of_copy"] = round(ms[f"{k}_ms"] / ms["copy_ms"], 3)
    res.update(history_share_moved=round(history, 4), async_equals_blocking=same, repeats=reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
