"""The conditions under which tests/test_gpu_degenerate.py means something, established on
the CPU from the oracle and the host table builder alone (tests/degenerate_scenes.py holds
the scenes and the plan of which variant runs on which traversal path):

  * the traversal tables the GPU test forces are valid (spt_accel_check) and the primary
    lists hold every sampled winner (check_winners of tests/test_prim_lists.py), so a GPU
    failure on these scenes is the kernels', not the builder's;
  * every scene is live: the family's odd spheres win at least 10% of the primary rays
    (sky_bytes, magnitudes: at least 10% of the pixels differ from an all-sky frame);
  * NaN cannot hide a failure: at most 25% of the oracle's sample values are NaN;
  * the 2^62 and 2^64 scenes reach the edge where a passing sphere's squared distance is
    not below FLT_MAX (Collision.hpp:87-109 starts from FLT_MAX with a strict compare);
  * the mirror room's paths end on both sides of the specular-event cap, some with
    exactly SPO_SPECULAR_CAP events and a colour, some cut at the next event with 0.
"""
import ctypes

import numpy as np
import pytest

import degenerate_scenes as D
from test_prim_lists import WALK, check_winners, prim_lists

VARIANTS = D.variants()
IDS = [v.id for v in VARIANTS]
LISTS_OFF = D.LISTS_OFF
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def spt_mod(native):
    import simplepathtracer_amd as spt
    return spt


_traced = {}


def traced(oracle, spt_mod, v):
    """The oracle's trace of every sample of the variant's frame, once per variant."""
    if v.id not in _traced:
        W, H, spp, depth, seed = v.frame
        view = spt_mod.camera_basis(v.eye, v.look, D.UP)
        sc = oracle.OracleScene(*v.arrays)
        fr = oracle.make_frame(view, v.eye, v.sky, W, H, spp, depth, seed)
        _traced[v.id] = (view, sc, fr) + oracle.trace_region(sc, fr, 0, H, 0, W)
    return _traced[v.id]


def accel_nodes(native, centers, radii, k, b):
    P = ctypes.c_void_p
    c = np.ascontiguousarray(centers, np.float32)
    r = np.ascontiguousarray(radii, np.float32)
    nodes = ctypes.c_uint32(0)
    rc = native.lib().spt_accel_check(c.ctypes.data_as(P), r.ctypes.data_as(P), len(r), k, b, ctypes.byref(nodes))
    assert rc == 0, ((k, b), native.lib().spt_last_error(None))
    return nodes.value


@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_tables_are_valid(oracle, native, spt_mod, v):
    c, r = v.arrays[0], v.arrays[1]
    shapes = D.SHAPES_ALL + (D.SHAPES_PICKED if v.id in sum(D.PICKED.values(), ()) else ())
    for k, b in shapes:
        nodes = accel_nodes(native, c, r, *D.shape_for_check(k, b, len(r)))
        assert (nodes > 0) == (k != 0), (k, b, nodes)  # more than 32 spheres: culling has a node table
    W, H, spp, _, seed = v.frame
    view = spt_mod.camera_basis(v.eye, v.look, D.UP)
    check_winners(oracle, native, spt_mod.Scene(*v.arrays), view, v.eye, W, H, spp, samples=3000, seed=seed,
                  want_on=v.id not in LISTS_OFF)
    b8 = prim_lists(native, c, r, view, v.eye, W, H)[0]
    assert ((b8[:, 1] != WALK).sum() > 0) == (v.id not in D.LISTS_OFF + D.LISTS_ALL_WALK)


@pytest.mark.parametrize("vid,walk", D.FILLER_CASES)
def test_filler_reaches_the_walk(native, spt_mod, vid, walk):
    """Behind D.FILLER[walk] stress spheres the default tree has the node count of the
    intended kernel (spt_kernels.hip launch_render), with valid tables."""
    v = D.by_id(vid)
    s = spt_mod.generate_stress(D.FILLER_SEED, D.FILLER[walk])
    a = D.with_filler(v, (s.centers, s.radii, s.colors, s.materials, s.fuzz))
    nodes = accel_nodes(native, a[0], a[1], *D.shape_for_check(D.AUTO, D.AUTO, len(a[1])))
    lo, hi = {"lds": (64, 2431), "global": (2432, 9000), "wave": (9001, 1 << 30)}[walk]
    assert lo <= nodes <= hi, nodes
    if walk != "lds":  # the smallest count within 10% of the threshold
        assert nodes <= lo * 1.1, nodes


@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_scene_is_live_and_not_all_nan(oracle, spt_mod, v):
    view, sc, fr, col, casts, spec, dropped = traced(oracle, spt_mod, v)
    W, H, spp, _, _ = v.frame
    if v.family in ("sky_bytes", "magnitudes"):
        sky_only = oracle.OracleScene(*(a[:0] for a in v.arrays))
        want, _ = oracle.render_segment(sc, fr, 0, H, 0, W)
        sky, _ = oracle.render_segment(sky_only, fr, 0, H, 0, W)
        live = float((want[:, :3].view(np.uint32) != sky[:, :3].view(np.uint32)).any(1).mean())
    else:
        xys = np.array([(x, y, s) for y in range(H) for x in range(W) for s in range(spp)], np.uint32)
        live = float(np.isin(oracle.primary_winners(sc, fr, xys), list(v.odd)).mean())
    nan = float(np.isnan(col[:, :, :3]).mean())
    print(f"{v.id}: live {live:.3f}, NaN share {nan:.3f}, rays {int(casts.sum())}")
    assert live >= 0.10
    assert nan <= 0.25


@pytest.mark.parametrize("vid", ["magnitudes/2^62", "magnitudes/2^64"])
def test_magnitudes_reach_the_edge(oracle, vid):
    """Hand-picked rays on which a sphere passes RaySphereIntersection yet find_closest
    returns none, its squared distance not below FLT_MAX.  With a unit direction a passing
    sphere has |c - o|^2 finite and a contact no farther than |c - o|, so only r * r = +inf
    gets there: the ground (r = 1000 units, r * r = inf from 2^48 on) seen from within
    sqrt(FLT_MAX) of its centre, where r*r - d2 = inf passes, the root tc - sqrt(inf) = -inf
    and the contact o + d * -inf is inf or NaN.  (No rendered ray starts there: the balls'
    own squared distances stay below |c - o|^2 - r^2 < FLT_MAX.)"""
    v = D.by_id(vid)
    sc = oracle.OracleScene(*v.arrays)
    unit = np.float32(v.arrays[1][1]) * np.float32(2.0)  # the balls' radius is half a scene unit
    g = v.arrays[0][0]
    found = 0
    for d in ([0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0.6, 0.8, 0, 0]):
        d = np.float32(d)
        o = (g - d * unit * np.float32(0.5)).astype(np.float32)
        o[3] = 0
        ok, ds, ahead = oracle.probe_sphere(sc, 0, d, o)
        win = oracle.find_closest(sc, d, o)
        print(f"{vid}: d {d[:3]} passes {ok} ds {ds} contact ahead {ahead} -> winner {win} of {sc.s.n}")
        if ok and not ds < FLT_MAX and win == sc.s.n:
            found += 1
    assert found >= 1
    # and a ball right before the camera is still found (the scene is not simply dead)
    view_d = np.float32([0, 0, 1, 0])
    assert oracle.find_closest(sc, view_d, np.float32(v.eye)) < sc.s.n


def test_spec_cap_paths_end_on_both_sides_of_the_cap(oracle, spt_mod):
    v = D.by_id("spec_cap/mirror_room")
    _, _, _, col, casts, spec, dropped = traced(oracle, spt_mod, v)
    cap = 1024  # SPO_SPECULAR_CAP
    lit = (col[:, :, :3] != 0).any(2)
    at_cap, cut = (spec == cap) & lit, (spec == cap + 1) & ~lit
    print(f"spec_cap: {int(at_cap.sum())} samples end with exactly {cap} events and a colour, {int(cut.sum())} are "
          f"cut at event {cap + 1}; {float((spec <= cap).mean()):.3f} end below or at the cap, mean {spec.mean():.0f} events")
    assert spec.max() == cap + 1
    assert at_cap.sum() >= 1
    assert cut.sum() >= 1 and (cut == (spec == cap + 1)).all()  # every cut path is black
    assert (casts[cut] == cap + 1).all()  # the primary ray and one ray per event but the last
    assert (spec <= cap).mean() >= 0.05 and (spec == cap + 1).mean() >= 0.05
    # task mode: every path still bouncing at pass 10 is dropped
    view, sc, fr = traced(oracle, spt_mod, v)[:3]
    W, H, _, _, _ = v.frame
    _, _, tspec, tdrop = oracle.trace_region(sc, fr, 0, H, 0, W, task=True)
    assert (tdrop == (spec >= 10)).all() and 0.5 < tdrop.mean() < 1.0


def test_schlick_bases_come_from_the_oracle(oracle, spt_mod):
    """The bases test_device_numerics_match_host adds to its hard list are ones the oracle's
    Schlick term takes on the nonfinite and magnitudes variants, and none of these variants
    reaches a base outside [0, 1]."""
    seen = []
    for v in D.variants("nonfinite") + D.variants("magnitudes"):
        W, H, spp, depth, seed = v.frame
        view = spt_mod.camera_basis(v.eye, v.look, D.UP)
        sc = oracle.OracleScene(*v.arrays)
        fr = oracle.make_frame(view, v.eye, v.sky, W, H, spp, depth, seed)
        seen.append(oracle.schlick_bases(lambda: oracle.render_segment(sc, fr, 0, H, 0, W)))
    seen = np.concatenate(seen)
    assert len(seen) > 1000
    for h in D.SCHLICK_BASES:
        assert (seen == np.float32(float.fromhex(h))).any(), h
    assert np.isfinite(seen).all() and seen.min() >= 0 and seen.max() <= 1
    assert seen.min() == np.float32(float.fromhex(D.SCHLICK_BASES[0]))
    assert seen.max() == np.float32(float.fromhex(D.SCHLICK_BASES[-1]))
