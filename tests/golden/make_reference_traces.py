"""Generate tests/golden/reference_traces.npz from the answers of the reference's own code.

    python tests/golden/make_reference_traces.py

Needs oracle/_ref/ref_harness (`make -C oracle ref`, run by build() where the reference's
headers are present); the oracle takes no part in the recorded colours.  The file holds data
only: the 1031 paths of tests/trace_rays.make_paths on the `random` scene of scenes.npz
through its 200 x 100 frame (o, d, seeds), a depth per path cycling through 1, 2, 10 and
50 (bounces), and for each the colour TraceAndSampleColor(d, o, bounces) returns on a
fresh reference thread seeded seeds[i] (rgba; pyoracle.ref_trace).
tests/test_gpu_trace.py traces these paths on the GPU against it, and
tests/test_reference_traces.py checks it on the CPU.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyoracle as po  # noqa: E402
from trace_rays import BOUNCES, FRAME, make_paths  # noqa: E402

EYE, SKY = [0, 1, -3, 0], [137, 207, 240, 0]


def recipe():
    """(scene, frame, o, d, seeds, bounces) of the fixture."""
    gs = np.load(os.path.join(HERE, "scenes.npz"), allow_pickle=False)
    sc = po.OracleScene(*(gs[f"random_{k}"] for k in ("centers", "radii", "colors", "materials", "fuzz")))
    fr = po.make_frame(gs["view"], EYE, SKY, FRAME[0], FRAME[1], 1, 10, 1)
    o, d, seeds = make_paths(po, sc, fr)
    bounces = np.array([BOUNCES[i % len(BOUNCES)] for i in range(len(o))], np.uint32)
    return sc, fr, o, d, seeds, bounces


def main():
    if not po.ref_available():
        sys.exit(f"{po.REF_BIN} is not built: run `make -C oracle ref` where the reference's headers are")
    sc, _, o, d, seeds, bounces = recipe()
    rgba = po.ref_trace(sc, d, o, bounces, seeds)
    path = os.path.join(HERE, "reference_traces.npz")
    np.savez_compressed(path, o=o, d=d, seeds=seeds, bounces=bounces, rgba=rgba)
    print("wrote", path, os.path.getsize(path), "bytes;", len(o), "paths")


if __name__ == "__main__":
    if sys.argv[1:]:
        sys.exit(__doc__)
    main()
