#!/usr/bin/env python3
"""What a scene update (Context.update_scene: refit tables, candidate lists built on the
device) saves an animation frame on the host, and what the stale tree shape costs a render.

    python tools/scene_update_probe.py [--spp 4] [--frames 8] [--repeats 5]

(a) Wall time of a resident accumulator frame, the protocol of tools/temporal_motion_probe.py:
    config 2's frame (1200 x 800, the 149-sphere scene) at --spp samples, the camera swinging
    between two eyes over two scenes in turn (every third sphere moved by [0.05, 0, 0.03]),
    TemporalAccumulator(resident=True) with refit=False and with refit=True in the same run;
    the first frame of each, which allocates, left out; median of the rest.  Beside them the
    wall time of set_scene + set_camera and of update_scene alone over the same sequence, the
    split update_scene reports (refit_ms on the host, lists_ms on the device) and the setters'
    accel_build_ms + prim_list_build_ms from spt_stats.
(b) Render time after a refit against after a rebuild: the same moved scene set by
    update_scene on a context built for the unmoved scene, and by set_scene; config 2's full
    frame at 100 spp, device time of the render launches (spt_stats render_ms), median of
    --repeats; for a jitter of sigma 0.05 and 0.5 and for a permutation of the small spheres'
    centres.  The two renders are compared bit for bit.

One JSON line on stdout.  Needs a GPU; there is no fallback.
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

from temporal_probe import DEPTH, EYE_B, H, LOOK_B, SEED, W  # noqa: E402

SHIFT = (0.05, 0.0, 0.03)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("scene_update_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    scene_a = spt.generate_spheres(1)
    centers = scene_a.centers.copy()
    centers[1::3, :3] += np.asarray(SHIFT, np.float32)
    scene_b = spt.Scene(centers, scene_a.radii, scene_a.colors, scene_a.materials, scene_a.fuzz)
    scenes = (scene_a, scene_b)
    cams = [(spt.camera_basis(), np.asarray(spt.scene.DEFAULT_EYE, np.float32)),
            (spt.camera_basis(EYE_B, LOOK_B), np.asarray(EYE_B, np.float32))]

    # (a) the accumulator's frame, and the state change alone
    wall, split = {}, {}
    for refit in (False, True):
        ctx = spt.Context(0)
        acc = spt.TemporalAccumulator(ctx, W, H, args.spp, DEPTH, seed=SEED, resident=True, refit=refit)
        ts = []
        for k in range(args.frames + 1):
            t0 = time.perf_counter()
            acc.frame(*cams[k & 1], scene=scenes[k & 1])
            ts.append(time.perf_counter() - t0)
        wall["frame_refit" if refit else "frame_rebuild"] = [round(t * 1e3, 3) for t in ts[1:]]
        ctx.close()
    ctx = spt.Context(0)
    ctx.set_scene(scene_a)
    ctx.set_camera(*cams[0], spt.INIT_COLOR)
    ctx.set_params(W, H, args.spp, DEPTH, SEED)
    ts, builds = [], []
    for k in range(1, args.frames + 2):
        t0 = time.perf_counter()
        ctx.set_scene(scenes[k & 1])
        ctx.set_camera(*cams[k & 1], spt.INIT_COLOR)
        ts.append(time.perf_counter() - t0)
        st = ctx.stats()
        builds.append((st["accel_build_ms"], st["prim_list_build_ms"]))
    wall["set_scene_set_camera"] = [round(t * 1e3, 3) for t in ts[1:]]
    split["accel_build_ms"] = round(median([b[0] for b in builds[1:]]), 3)
    # the last of the two list builds of a frame (set_scene's, then set_camera's)
    split["prim_list_build_ms"] = round(median([b[1] for b in builds[1:]]), 3)
    ts, infos = [], []
    for k in range(1, args.frames + 2):
        t0 = time.perf_counter()
        infos.append(ctx.update_scene(scenes[k & 1].centers, *cams[k & 1]))
        ts.append(time.perf_counter() - t0)
    wall["update_scene"] = [round(t * 1e3, 3) for t in ts[1:]]
    split["refit_ms"] = round(median([i["refit_ms"] for i in infos[1:]]), 3)
    split["lists_ms"] = round(median([i["lists_ms"] for i in infos[1:]]), 3)
    split["lists_on_device"] = int(all(i["lists_on_device"] for i in infos))
    ctx.close()

    # (b) the cost of the stale shape
    rng = np.random.default_rng(5)
    small = np.flatnonzero(scene_a.radii <= 4 * np.median(scene_a.radii))
    moved = {}
    for sigma in (0.05, 0.5):
        c = scene_a.centers.copy()
        c[small, :3] += rng.normal(0.0, sigma, (len(small), 3)).astype(np.float32)
        moved[f"jitter_{sigma}"] = c
    c = scene_a.centers.copy()
    c[small] = scene_a.centers[rng.permutation(small)]
    moved["permutation"] = c
    stale = {}
    for name, c in moved.items():
        sc = spt.Scene(c, scene_a.radii, scene_a.colors, scene_a.materials, scene_a.fuzz)
        res, img = {}, {}
        for how in ("rebuild", "refit"):
            ctx = spt.Context(0)
            ctx.set_scene(scene_a if how == "refit" else sc)
            ctx.set_camera(*cams[0], spt.INIT_COLOR)
            ctx.set_params(W, H, 100, 50, SEED)
            if how == "refit":
                ctx.update_scene(c)
            ctx.render_segment(0, H, 0, W, rgba=False, g_data=np.zeros(W * H * 3, np.uint8))  # warm
            t = []
            for _ in range(args.repeats):
                ctx.reset_stats()
                img[how] = ctx.render_segment(0, H, 0, W)
                t.append(ctx.stats()["render_ms"])
            res[how + "_render_ms"] = round(median(t), 3)
            res[how + "_render_ms_all"] = [round(x, 3) for x in t]
            ctx.close()
        res["refit_over_rebuild"] = round(res["refit_render_ms"] / res["rebuild_render_ms"], 4)
        res["bit_identical"] = bool(np.array_equal(img["refit"].view(np.uint32), img["rebuild"].view(np.uint32)))
        stale[name] = res

    out = {"scene": "c2", "spheres": scene_a.n, "frame": f"{W}x{H}x{args.spp} spp",
           "wall_ms": {k: median(v) for k, v in wall.items()}, "wall_ms_all": wall, "split_ms": split,
           "render_after": stale}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
