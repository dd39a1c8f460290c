#!/usr/bin/env python3
"""Rate of the occlusion query (spt_occluded_rays_async) beside the closest-hit query with
hit records (spt_cast_rays_async) on the same rays, in the same process.

    python tools/occlusion_probe.py [--scene c2|stress10k|both] [--rays 4194304] [--repeats 3]

Per scene: 2^22 device-resident rays of kinds A and B (tools/cast_probe.py: mixed_rays),
shuffled.  Three limit regimes:

    unbounded   no limits: the walk ends at a lane's first blocker, nothing else bounds it
    short       L = a quarter of the batch's median ds: most hits lie beyond the limit, the
                near test culls from the first node on
    all-miss    rays from high above the scene, pointing away: nothing can end early

Per regime and repeat the two queries alternate: two warm-up launches each, then launches
timed with device events until at least 0.5 s of them have run.  The yardstick is the cast
of the same run; the spread is the repeats' own.  One JSON line per scene on stdout.  Needs a
GPU; there is no fallback.
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

from cast_probe import MIN_TIMED_S, make_scene, mixed_rays, unit  # noqa: E402

SCENES = {"c2": "random", "stress10k": "stress10k"}


def miss_rays(n, seed=2):
    """Kind G of tests/cast_rays.py: from high above the scene, pointing away."""
    rng = np.random.default_rng(seed)
    o4, d4 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    o4[:, 0], o4[:, 1], o4[:, 2] = rng.uniform(-20, 20, n), rng.uniform(40, 80, n), rng.uniform(-20, 20, n)
    dg = unit(rng, n)
    dg[:, 1] = np.abs(dg[:, 1])
    d4[:, :3] = dg
    return o4, d4


def timed(torch, launch, stream, n):
    """Mrays/s over >= MIN_TIMED_S of launch() calls (device events), after two warm-ups."""
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
    while s < MIN_TIMED_S:
        k = max(k + 1, math.ceil(1.2 * k * MIN_TIMED_S / max(s, 1e-6)))
        s = span(k)
    return n * k / s / 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="both", choices=["c2", "stress10k", "both"])
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("occlusion_probe.py needs a GPU (no fallback)")
    import simplepathtracer_amd as spt
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    eye = np.asarray(spt.scene.DEFAULT_EYE, np.float32)[:3]
    n = args.rays
    for key in (("c2", "stress10k") if args.scene == "both" else (args.scene,)):
        scene = make_scene(spt, SCENES[key])
        ctx = spt.Context(0)
        ctx.set_scene(scene)
        o, d, _ = mixed_rays(scene, eye, n)
        mo, md = miss_rays(n)
        to, td, tmo, tmd = (torch.from_numpy(x).to(dev) for x in (o, d, mo, md))
        ti = torch.zeros(n, dtype=torch.int32, device=dev)
        th = torch.zeros((n, 2, 4), dtype=torch.float32, device=dev)
        tocc = torch.zeros(n, dtype=torch.uint8, device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))

        def cast(a, b):
            return lambda: ctx.cast_rays_async(a.data_ptr(), b.data_ptr(), n, ti.data_ptr(), th.data_ptr(), stream.cuda_stream)

        def occl(a, b, lim):
            return lambda: ctx.occluded_async(a.data_ptr(), b.data_ptr(), lim.data_ptr() if lim is not None else 0, n,
                                              tocc.data_ptr(), stream=stream.cuda_stream)

        # the batch's own closest hits set the short limit; the answers' shares go on record
        cast(to, td)()
        stream.synchronize()
        hit = ti.cpu().numpy().view(np.uint32) < scene.n
        ds = th.cpu().numpy()[:, 1, 3]
        quarter = np.float32(0.25) * np.float32(np.median(ds[hit]))
        tl = torch.full((n,), float(quarter), dtype=torch.float32, device=dev)
        cast(tmo, tmd)()
        stream.synchronize()
        assert not (ti.cpu().numpy().view(np.uint32) < scene.n).any(), "the all-miss batch hits something"
        regimes = {"unbounded": (to, td, None), "short": (to, td, tl), "all_miss": (tmo, tmd, None)}
        out = {"scene": key, "spheres": scene.n, "rays": n, "hit_share": round(float(hit.mean()), 3),
               "short_limit_sq": float(quarter)}
        for name, (a, b, lim) in regimes.items():
            occ_r, cast_r = [], []
            for _ in range(args.repeats):  # alternated: occlusion, cast, occlusion, cast, ...
                occ_r.append(round(timed(torch, occl(a, b, lim), stream, n), 1))
                cast_r.append(round(timed(torch, cast(a, b), stream, n), 1))
            share = float(tocc.cpu().numpy().mean())

            def spread(v):
                return {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)}

            out[name] = {"occluded_share": round(share, 3), "occluded_mrays_s": spread(occ_r),
                         "cast_hits_mrays_s": spread(cast_r),
                         "ratio_of_medians": round(spread(occ_r)["median"] / spread(cast_r)["median"], 3)}
        ctx.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
