"""The path mix of the path-query tests (spt_trace_rays), shared by the GPU tests
(tests/test_gpu_trace.py), the reference fixture's recipe (tests/golden/make_reference_traces.py)
and its CPU check (tests/test_reference_traces.py).  A plain helper module: numpy only.

make_paths builds, for a scene and the frame it is looked at through, n rays and a seed each:
half are the scene's own primary rays through a grid of the frame's pixels
(pyoracle.primary_rays), half the adversarial cast mix (cast_rays.make_rays: rays from
sphere surfaces, grazing rays, directions off unit length, non-finite components, misses),
the two halves permuted together so that single waves mix them.  1031 is prime: the last
wave is partial.
"""
import ctypes

import numpy as np

from cast_rays import make_rays

N_PATHS = 1031
BOUNCES = (1, 2, 10, 50)
FIRST_SEEDS = (0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
FRAME = (200, 100)  # of the golden scenes' paths (tests/test_reference_parity.py path_case)


def make_paths(oracle, scene, frame, n=N_PATHS, ray_seed=77, rng_seed=5):
    """(o, d, seeds): float32 (n, 4) origins and directions and a uint32 seed per path.
    scene: anything with .centers and .radii; frame: the pyoracle.Frame whose eye and
    pixels the primary half uses."""
    mix = n // 2
    prim = n - mix
    pix = np.linspace(0, frame.width * frame.height - 1, prim).astype(np.int64)
    xy = np.stack([pix % frame.width, pix // frame.width], axis=1)
    d = oracle.primary_rays(frame, xy, ray_seed)
    o = np.tile(np.array(list(frame.eye), np.float32), (prim, 1))
    mo, md, _, _ = make_rays(scene.centers, scene.radii, n=mix, seed=ray_seed)
    o, d = np.concatenate([o, mo]), np.concatenate([d, md])
    rng = np.random.default_rng(rng_seed)
    order = rng.permutation(n)
    seeds = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    seeds[:len(FIRST_SEEDS)] = FIRST_SEEDS
    return np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order]), seeds


def scene_states(seeds):
    """The reference's stream start per seed, seed << 31 | seed (Random.hpp:19;
    pyoracle.scene_state), as uint64."""
    s = np.asarray(seeds, np.uint32).astype(np.uint64)
    return (s << np.uint64(31)) | s


def oracle_trace(oracle, osc, frame, o, d, bounces, states):
    """spo_trace_ray per path on the raw state states[i]: colours (n, 4), casts (n,) and the
    oracle's info rows (n, TRACE_INFO): [specular events, cut, per-event counts]."""
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    n = len(o)
    bounces = np.broadcast_to(np.asarray(bounces, np.uint32), (n,))
    out = np.zeros((n, 4), np.float32)
    info = np.zeros((n, oracle.TRACE_INFO), np.uint32)
    casts = np.zeros(n, np.uint32)
    fn, sc, fr = oracle.lib().spo_trace_ray, osc.ref, ctypes.byref(frame)
    st = ctypes.c_uint64(0)
    for i in range(n):
        st.value = int(states[i])
        casts[i] = fn(sc, fr, d.ctypes.data + 16 * i, o.ctypes.data + 16 * i, int(bounces[i]), ctypes.byref(st),
                      out.ctypes.data + 16 * i, info.ctypes.data + 4 * oracle.TRACE_INFO * i)
    return out, casts, info


def device_info(casts, info):
    """What spt_trace_rays reports for those paths: [casts, specular events | cut << 31]."""
    return np.stack([casts, info[:, 0] | (np.minimum(info[:, 1], 1) << np.uint32(31))], axis=1).astype(np.uint32)
