#!/usr/bin/env python3
"""Device time of the temporal accumulation under moving spheres (spt_temporal_motion_async)
beside the plain call on the same frames, and the wall time of a TemporalAccumulator frame with
the history resident on the device and without, in one process.

    python tools/temporal_motion_probe.py [--spp 4] [--repeats 3] [--frames 6]

The frames are tools/temporal_probe.py's: config 2's, 1200 x 800, the 149-sphere scene at
--spp samples; frame A from the default camera, frame B from an eye moved by [0.15, 0.05, 0.1]
that looks about 2 degrees to the side -- B of a scene in which every third sphere (1, 4, 7,
...: not the ground) has moved by [0.05, 0, 0.03], a few pixels at the scene's depths.  All
device-resident.

    (a) plain moved     spt_temporal_async, B against the history A: the yardstick
    (b) unmoved table   spt_temporal_motion_async with a table in which nothing moved: the
                        records are gathered, every pixel takes the plain path
    (c) a third moved   spt_temporal_motion_async with the table of the scene's motion

Timing as tools/temporal_probe.py: per repeat two warm-up calls, then calls timed with device
events on a stream of the caller's until at least 0.5 s of them have run; medians of the
repeats.  (b)'s answer is compared bit for bit with (a)'s, (c)'s with the blocking form's.

The accumulator: --frames frames of the camera swinging between the two eyes over the two
scenes in turn, TemporalAccumulator(resident=False) then (resident=True), wall time per frame
(the first frame of each, which allocates, left out; median of the rest), and of set_scene
alone, which every frame with a scene pays on the host.  One JSON line on stdout.  Needs a GPU;
there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from temporal_probe import DEPTH, EYE_B, H, LOOK_B, SEED, W, timed  # noqa: E402

SHIFT = (0.05, 0.0, 0.03)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=6)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("temporal_motion_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    scene_a = spt.generate_spheres(1)
    centers = scene_a.centers.copy()
    centers[1::3, :3] += np.asarray(SHIFT, np.float32)
    scene_b = spt.Scene(centers, scene_a.radii, scene_a.colors, scene_a.materials, scene_a.fuzz)
    ctx = spt.Context(0)
    npix = W * H
    cams = [(spt.camera_basis(), np.asarray(spt.scene.DEFAULT_EYE, np.float32)),
            (spt.camera_basis(EYE_B, LOOK_B), np.asarray(EYE_B, np.float32))]
    frames = []
    for k, ((view, eye), scene) in enumerate(zip(cams, (scene_a, scene_b))):
        ctx.set_scene(scene)
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
    tables = {"unmoved": spt.sphere_motion(scene_b, scene_b), "third": spt.sphere_motion(scene_b, scene_a)}
    d_tables = {k: torch.from_numpy(v).to(dev) for k, v in tables.items()}
    out = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    out_mom = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def ptrs(f):
        return tuple(f[k].data_ptr() for k in ("rgba", "mom", "feat", "ids"))

    def temporal(table):
        kw = {} if table is None else dict(d_motion=d_tables[table].data_ptr(), n_spheres=scene_b.n)
        ctx.temporal_async(W, H, *ptrs(b), cams[1][0], cams[1][1], ptrs(a), cams[0][0], cams[0][1], d_out_rgba=out.data_ptr(),
                           d_out_mom=out_mom.data_ptr(), stream=stream.cuda_stream, **kw)

    def answer(table):
        temporal(table)
        stream.synchronize()
        return out.cpu().numpy().view(np.uint32), out_mom.cpu().numpy().view(np.uint32)

    reps = []
    for _ in range(args.repeats):
        t = {"plain_moved_ms": timed(torch, stream, lambda: temporal(None)),
             "unmoved_table_ms": timed(torch, stream, lambda: temporal("unmoved")),
             "third_moved_ms": timed(torch, stream, lambda: temporal("third"))}
        reps.append({k: round(v * 1e3, 4) for k, v in t.items()})
    plain, unmoved, third = answer(None), answer("unmoved"), answer("third")
    h = {k: [f[k].cpu().numpy() for f in frames] for k in ("rgba", "mom", "feat", "ids")}
    blocking = ctx.temporal(h["rgba"][1].reshape(H, W, 4), h["mom"][1], h["feat"][1], h["ids"][1].view(np.uint32), cams[1][0],
                            cams[1][1], (h["rgba"][0], h["mom"][0], h["feat"][0], h["ids"][0].view(np.uint32)), cams[0][0],
                            cams[0][1], motion=tables["third"])
    eq = lambda x, y: bool(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]))  # noqa: E731
    blocking = (blocking[0].reshape(-1, 4).view(np.uint32), blocking[1].reshape(-1, 4).view(np.uint32))
    moved_ids = np.flatnonzero((tables["third"][:, :4] != tables["third"][:, 4:]).any(axis=1))
    on_moved = np.isin(h["ids"][1].view(np.uint32), moved_ids) & (h["feat"][1][:, 0, 3] > 0)
    n_cur = h["mom"][1][:, 3]
    hist = {"plain": float((plain[1].view(np.float32)[:, 3] > n_cur)[on_moved].mean()),
            "motion": float((third[1].view(np.float32)[:, 3] > n_cur)[on_moved].mean())}

    # the accumulator, frame by frame, and set_scene alone
    wall = {}
    for resident in (False, True):
        acc = spt.TemporalAccumulator(ctx, W, H, args.spp, DEPTH, seed=SEED, resident=resident)
        ts = []
        for k in range(args.frames + 1):
            t0 = time.perf_counter()
            acc.frame(*cams[k & 1], scene=(scene_a, scene_b)[k & 1])
            ts.append(time.perf_counter() - t0)
        wall["resident" if resident else "host"] = [round(t * 1e3, 3) for t in ts[1:]]
    ts = []
    for k in range(args.frames + 1):
        t0 = time.perf_counter()
        ctx.set_scene((scene_a, scene_b)[k & 1])
        ts.append(time.perf_counter() - t0)
    wall["set_scene"] = [round(t * 1e3, 3) for t in ts[1:]]
    ctx.close()

    ms = {k: median([r[k] for r in reps]) for k in reps[0]}
    spread = {k: round(max(r[k] for r in reps) - min(r[k] for r in reps), 4) for k in reps[0]}
    res = {"scene": "c2", "spheres": scene_a.n, "spheres_moved": int(len(moved_ids)), "frame": f"{W}x{H}x{args.spp} spp", **ms,
           "spread_ms": spread,
           "unmoved_over_plain": round(ms["unmoved_table_ms"] / ms["plain_moved_ms"], 3),
           "third_over_plain": round(ms["third_moved_ms"] / ms["plain_moved_ms"], 3),
           "unmoved_equals_plain": eq(unmoved, plain), "async_equals_blocking": eq(third, blocking),
           "pixels_on_moved_spheres": int(on_moved.sum()), "history_share_on_them": {k: round(v, 4) for k, v in hist.items()},
           "frame_wall_ms": {k: median(v) for k, v in wall.items()}, "frame_wall_ms_all": wall, "repeats": reps}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
