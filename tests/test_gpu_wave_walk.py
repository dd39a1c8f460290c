"""The wave walk of the box tree (find_closest, spt_path.h) against brute force.

The walk steps through the tree's preorder records on the scalar unit: a node's successor
is read ahead into the registers of the record just tested, a culled inner node reloads
its skip target, a leaf never does, and the walk ends where the position reaches the
table's end -- by stepping past the last record or by a skip link that points there.
Every case here compares with brute force (cluster size 0, no tree: every sphere tested
for every ray, the reference's scan) bit for bit, ray counts included.

(a) Renders of the config-2 scene, of the exact-tie scene of
    test_culling_is_exact_with_exact_distance_ties, and of a 33-sphere scene, at 64 x 40,
    4 spp, depth 50, on binary trees (the most culled inner nodes and skip reloads), 4-ary
    ones, 16-ary ones (wide and shallow: most top nodes are leaves), the largest tree the
    wave walk still takes (63 nodes: the tie scene in clusters of 7 under a 4-ary tree) and
    the smallest tree a scene of more than 32 spheres gives (33 spheres of which 16 are
    large enough for the always-tested list: 17 members in three leaves, which a binary
    tree joins with one inner node: 4 records; under a branching of 3 or more the builder
    makes no tree of three leaves but a flat list, which find_closest<false> walks).
    Every case asserts that its shape is a tree (more records than leaves: the flag the
    context passes to the kernels) and, from the launch's block size and the node count,
    which walk served it: the wave walk (256 threads, at most 63 nodes) or, for the three
    larger shapes of the issue's list, the LDS lane walk (1 024 threads).
(b) Ray queries on a scene whose layout is known without reading the tables: 48 equal
    spheres on the x axis in six clumps of eight, ten units apart.  Leaves are runs of the
    spheres' order along x, the nodes' boxes are disjoint along x, and the layout of a
    direction octant lists siblings front to back, so for rays travelling +x the last
    record is the clump at x = 50 and for rays travelling -x the clump at x = 0.  The 4 096
    rays come in waves of one kind each (the wave enters a node when any lane needs it):
      away       origins left of the scene pointing away: every record reached is culled
                 for every lane, and the last of them skips to the table's end
      first+     +x pencils from x = -3 onto the first clump: once it is hit the near test
                 culls the rest; the last record is culled
      last+      +x pencils from x = 47 onto the last clump: the clumps behind fail the front
                 test; the last record is an entered leaf
      first-     -x pencils from x = 58 onto the clump at 50 (first in that layout)
      last-      -x pencils from x = 8 onto the clump at 0 (last in that layout)
      side       from above onto one sphere each: one leaf entered
      gap        from above between two clumps: every record culled
      graze      along the axis at a height of 0.26 .. 0.34 (r = 0.3): every record entered,
                 hits and misses either side of the hh > 1e-3 threshold
      mixed      every lane a random kind of the above
      nocull     `side` waves in which one lane's direction has length 2: that lane never
                 culls (c), so the wave enters every record for it
    cast whole, and in batches of 1 and 37 rays, which leave a wave with inactive lanes.
    Every shape is asserted to be a tree of at most 63 nodes, which cast_kernel<true, 8>
    serves (a cast reports no launch shape, so the node count and the tree flag are the
    guard); (2, 16) is the wide tree whose top nodes are mostly leaves.
(c) One wave of 63 `side` lanes and a single lane that may not cull.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import assert_bitwise, bits, scene_from, setup

pytestmark = pytest.mark.gpu

FRAME = (64, 40, 4, 50)  # width, height, spp, depth
SHAPES = ((8, 2), (8, 4), (8, 16), (3, 16), (5, 4))
# spt_internal.h: kLdsMinNodes - 1 (larger trees take a lane walk), kLdsNodeRecords, kGlaneMaxNodes
WAVE_WALK_MAX_NODES, LDS_NODE_RECORDS, GLANE_MAX_NODES = 63, 2432, 9000
BLOCK_THREADS = {"wave": 256, "lds": 1024}


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ctx(spt):
    c = spt.Context(0)
    yield c
    c.close()


def members(s):
    """Spheres the builder puts into clusters (build_accel: not above four times the median
    radius, finite)."""
    c, r = np.asarray(s.centers, np.float32), np.asarray(s.radii, np.float32)
    med = np.sort(r)[s.n // 2]
    always = (r > np.float32(4.0) * med) | ~np.isfinite(r) | ~np.isfinite(c[:, :3]).all(axis=1)
    return int(s.n - always.sum())


def walk_of(spt, s, k, b):
    """(records, walk) of a shape by launch_render's rule: 'flat' when the builder made no
    inner node (as many records as leaves), else 'wave' or a lane walk."""
    nodes = tree_nodes(spt, s, k, b)
    leaves = -(-members(s) // k)
    assert nodes >= leaves
    if nodes == leaves:
        return nodes, "flat"
    if nodes <= WAVE_WALK_MAX_NODES or nodes > GLANE_MAX_NODES:
        return nodes, "wave"
    return nodes, "lds" if nodes + 1 <= LDS_NODE_RECORDS else "glane"


def tree_nodes(spt, s, k, b):
    P = ctypes.c_void_p
    nodes = ctypes.c_uint32(0)
    c, r = np.ascontiguousarray(s.centers, np.float32), np.ascontiguousarray(s.radii, np.float32)
    rc = spt._native.lib().spt_accel_check(c.ctypes.data_as(P), r.ctypes.data_as(P), s.n, k, b, ctypes.byref(nodes))
    assert rc == 0, spt._native.lib().spt_last_error(None)
    return nodes.value


# ---------------------------------------------------------------- (a) renders

def _parts(s):
    return (np.asarray(s.centers, np.float32), np.asarray(s.radii, np.float32), np.asarray(s.colors, np.float32),
            np.asarray(s.materials), np.asarray(s.fuzz, np.float32))


def tie_scene(spt, golden_scenes):
    """test_culling_is_exact_with_exact_distance_ties' scene: every small sphere twice."""
    c, r, col, m, f = _parts(scene_from(spt, golden_scenes, "random"))
    small = np.nonzero(r < 0.5)[0]
    col2 = col[small].copy()
    col2[:, :3] = 255.0 - col2[:, :3]
    m2 = np.where(m[small] == 3, 1, 3).astype(m.dtype)
    return spt.Scene(np.concatenate([c, c[small]]), np.concatenate([r, r[small]]), np.concatenate([col, col2]),
                     np.concatenate([m, m2]), np.concatenate([f, f[small]]))


def scene_of_33(spt, golden_scenes):
    """The config-2 scene's four large spheres, its first 17 small ones, and its next 12 small
    ones at ten times their radius: 16 radii above four times the median (always tested) and
    17 cluster members."""
    c, r, col, m, f = _parts(scene_from(spt, golden_scenes, "random"))
    big, small = np.nonzero(r >= 0.5)[0], np.nonzero(r < 0.5)[0]
    assert len(big) == 4
    pick = np.concatenate([big, small[:29]])
    r2 = r[pick].copy()
    r2[4 + 17:] *= np.float32(10.0)
    assert len(pick) == 33 and (r2 > 4 * np.median(r2)).sum() == 16
    return spt.Scene(c[pick], r2, col[pick], m[pick], f[pick])


RENDER_SCENES = {"config2": lambda spt, gs: scene_from(spt, gs, "random"), "ties": tie_scene, "33": scene_of_33}
RENDER_CASES = ([("config2", kb) for kb in SHAPES] + [("ties", kb) for kb in SHAPES] + [("ties", (7, 4)), ("33", (8, 2))])
# node counts that are the point of a case
RENDER_NODES = {("ties", (7, 4)): WAVE_WALK_MAX_NODES, ("33", (8, 2)): 4}
# the shapes of the issue's list that are too large for the wave walk
RENDER_LANE_WALK = (("config2", (3, 16)), ("ties", (8, 2)), ("ties", (3, 16)), ("ties", (5, 4)))
_brute = {}


def brute_render(spt, ctx, golden_scenes, name):
    """The scene, its brute-force frame and ray count: rendered once, shared, never changed."""
    if name not in _brute:
        s = RENDER_SCENES[name](spt, golden_scenes)
        W, H, spp, depth = FRAME
        setup(ctx, s, W, H, spp, depth, seed=4)
        ctx.set_cluster_size(0)
        ctx.set_cluster_tree(0)
        ctx.reset_stats()
        img = ctx.render_segment(0, H, 0, W)
        img.setflags(write=False)
        _brute[name] = (s, img, ctx.stats()["casts"])
    return _brute[name]


@pytest.mark.parametrize("case", RENDER_CASES, ids=[f"{n}-{k}-{b}" for n, (k, b) in RENDER_CASES])
def test_render_equals_brute_force(spt, ctx, golden_scenes, case):
    name, (k, b) = case
    s, want, want_casts = brute_render(spt, ctx, golden_scenes, name)
    nodes, walk = walk_of(spt, s, k, b)
    print(f"{name} ({k}, {b}): {nodes} nodes, {walk} walk")
    assert walk == ("lds" if case in RENDER_LANE_WALK else "wave")
    if case in RENDER_NODES:
        assert nodes == RENDER_NODES[case]
    W, H, spp, depth = FRAME
    try:
        setup(ctx, s, W, H, spp, depth, seed=4)
        ctx.set_cluster_size(k)
        ctx.set_cluster_tree(b)
        ctx.reset_stats()
        got = ctx.render_segment(0, H, 0, W)
        st = ctx.stats()
        casts = st["casts"]
    finally:
        ctx.set_cluster_size(spt._native.CLUSTER_AUTO)
        ctx.set_cluster_tree(spt._native.TREE_AUTO)
    assert want_casts > W * H * spp  # paths bounce: the walk serves secondary rays too
    assert_bitwise(got, want, f"{name}, tree ({k}, {b}) vs brute force")
    assert casts == want_casts
    assert st["block_threads"] == BLOCK_THREADS[walk]


# ---------------------------------------------------------------- (b), (c) ray queries

CLUMPS, PER, PITCH, GAP, R = 6, 8, 0.7, 10.0, 0.3
X_LAST = GAP * (CLUMPS - 1)
KINDS = ("away", "first+", "last+", "first-", "last-", "side", "gap", "graze")
CAST_SHAPES = ((8, 2), (8, 4), (2, 16), (3, 2), (2, 2))  # 10 / 8 / 32 / 30 / 46 nodes


def clump_scene(spt):
    n = CLUMPS * PER
    c = np.zeros((n, 4), np.float32)
    c[:, 0] = [GAP * g + PITCH * j for g in range(CLUMPS) for j in range(PER)]
    col = np.zeros((n, 4), np.float32)
    col[:, :3] = 200.0
    return spt.Scene(c, np.full(n, R, np.float32), col, np.full(n, 3, np.uint8), np.zeros(n, np.float32))


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def rays_of(kind, m, rng):
    """m rays of one kind, float64 (o, d); directions of unit length."""
    u = rng.uniform(-1.0, 1.0, (m, 3))
    o, d = np.zeros((m, 3)), np.zeros((m, 3))
    if kind == "away":
        o[:] = np.stack([-20.0 - 5.0 * np.abs(u[:, 0]), 3.0 * u[:, 1], 3.0 * u[:, 2]], axis=1)
        d[:] = np.stack([-np.ones(m), 0.3 * u[:, 1], 0.3 * u[:, 0]], axis=1)
    elif kind in ("first+", "last+", "first-", "last-"):
        sign = 1.0 if kind.endswith("+") else -1.0
        # the sphere the pencil meets first, and a start 3 units before its clump
        if kind == "first+":
            x0, target = -3.0, 0.0
        elif kind == "last+":
            x0, target = X_LAST - 3.0, X_LAST
        elif kind == "first-":
            x0, target = X_LAST + PITCH * (PER - 1) + 3.0, X_LAST + PITCH * (PER - 1)
        else:
            x0, target = PITCH * (PER - 1) + 3.0, PITCH * (PER - 1)
        o[:] = np.stack([np.full(m, x0), 0.05 * u[:, 0], 0.05 * u[:, 1]], axis=1)
        aim = np.stack([np.full(m, target), 0.2 * u[:, 1], 0.2 * u[:, 2]], axis=1)
        d[:] = aim - o
        assert (np.sign(d[:, 0]) == sign).all()
    elif kind in ("side", "gap"):
        g, j = rng.integers(0, CLUMPS, m), rng.integers(0, PER, m)
        x = GAP * g + PITCH * j if kind == "side" else GAP * rng.integers(0, CLUMPS - 1, m) + 7.5 + 0.3 * u[:, 0]
        o[:] = np.stack([x + 0.3 * u[:, 1], np.full(m, 2.0), 0.3 * u[:, 2]], axis=1)
        aim = np.stack([x, np.zeros(m), 0.25 * u[:, 0] if kind == "side" else np.zeros(m)], axis=1)
        d[:] = aim - o
    elif kind == "graze":
        y = 0.30 + 0.04 * u[:, 0]
        o[:] = np.stack([-3.0 + u[:, 1], y, np.zeros(m)], axis=1)
        d[:] = np.stack([np.ones(m), 1e-4 * u[:, 2], np.zeros(m)], axis=1)
    else:
        raise KeyError(kind)
    return o, _unit(d)


def clump_rays():
    """4 096 rays, wave by wave: 6 waves of each kind, 8 mixed, 8 `side` waves with one lane
    that may not cull.  Returns float32 o, d (n, 4) and the kind of each wave."""
    rng = np.random.default_rng(8)
    os_, ds, kinds = [], [], []
    for kind in KINDS:
        for _ in range(6):
            o, d = rays_of(kind, 64, rng)
            os_.append(o), ds.append(d), kinds.append(kind)
    for _ in range(8):
        o, d = np.zeros((64, 3)), np.zeros((64, 3))
        for lane, kind in enumerate(rng.choice(KINDS, 64)):
            o[lane], d[lane] = (a[0] for a in rays_of(kind, 1, rng))
        os_.append(o), ds.append(d), kinds.append("mixed")
    for w in range(8):
        o, d = rays_of("side", 64, rng)
        d[(17 * w + 5) % 64] *= 2.0
        os_.append(o), ds.append(d), kinds.append("nocull")
    o4, d4 = np.zeros((64 * len(kinds), 4), np.float32), np.zeros((64 * len(kinds), 4), np.float32)
    o4[:, :3], d4[:, :3] = np.concatenate(os_), np.concatenate(ds)
    assert len(o4) == 4096
    return o4, d4, kinds


_clump = {}


def clump_side(spt, ctx):
    """Scene, rays and brute force's answers, computed once."""
    if not _clump:
        s = clump_scene(spt)
        o, d, kinds = clump_rays()
        ctx.set_cluster_size(0)
        ctx.set_cluster_tree(0)
        ctx.set_scene(s)
        idx, hit = ctx.cast_rays(o, d, hits=True)
        idx.setflags(write=False), hit.setflags(write=False)
        _clump.update(scene=s, o=o, d=d, kinds=kinds, idx=idx, hit=hit)
        # the kinds do what they are for
        by = {k: np.concatenate([idx[64 * w:64 * w + 64] for w, kw in enumerate(kinds) if kw == k]) for k in set(kinds)}
        last = CLUMPS * PER - 1
        assert (by["away"] == s.n).all() and (by["gap"] == s.n).all()
        assert (by["first+"] == 0).all() and (by["last+"] == last - PER + 1).all()
        assert (by["first-"] == last).all() and (by["last-"] == PER - 1).all()
        assert (by["side"] < s.n).all()
        assert 0.2 < (by["graze"] < s.n).mean() < 0.8
    return _clump


def check_casts(got, w, sel, what):
    gi, gh = got
    bad = np.nonzero(gi != w["idx"][sel])[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(gi)} rays pick another sphere; first ray {sel[bad[0]]} "
                           f"(wave kind {w['kinds'][sel[bad[0]] // 64]}): got {gi[bad[0]]}, want {w['idx'][sel][bad[0]]}")
    assert np.array_equal(bits(gh), bits(w["hit"][sel])), f"{what}: hit records differ"


@pytest.mark.parametrize("shape", CAST_SHAPES, ids=[f"{k}-{b}" for k, b in CAST_SHAPES])
def test_casts_equal_brute_force(spt, ctx, shape):
    w = clump_side(spt, ctx)
    k, b = shape
    nodes, walk = walk_of(spt, w["scene"], k, b)
    print(f"clumps ({k}, {b}): {nodes} nodes, {walk} walk")
    assert walk == "wave" and nodes <= WAVE_WALK_MAX_NODES
    o, d = w["o"], w["d"]
    every = np.arange(len(o))
    try:
        ctx.set_cluster_size(k)
        ctx.set_cluster_tree(b)
        ctx.set_scene(w["scene"])
        check_casts(ctx.cast_rays(o, d, hits=True), w, every, "4096 rays")
        # a wave with inactive lanes: 1 and 37 rays of each kind of wave
        for kind in dict.fromkeys(w["kinds"]):
            first = 64 * w["kinds"].index(kind)
            for m in (1, 37):
                sel = every[first:first + m]
                check_casts(ctx.cast_rays(o[sel], d[sel], hits=True), w, sel, f"{m} rays of a {kind} wave")
    finally:
        ctx.set_cluster_size(spt._native.CLUSTER_AUTO)
        ctx.set_cluster_tree(spt._native.TREE_AUTO)


@pytest.mark.parametrize("shape", CAST_SHAPES, ids=[f"{k}-{b}" for k, b in CAST_SHAPES])
def test_one_lane_that_may_not_cull(spt, ctx, shape):
    """(c): a single wave of 63 ordinary lanes and one whose direction is not of unit length."""
    w = clump_side(spt, ctx)
    k, b = shape
    assert walk_of(spt, w["scene"], k, b)[1] == "wave"
    first = 64 * w["kinds"].index("nocull")
    sel = np.arange(first, first + 64)
    dlen = np.linalg.norm(w["d"][sel, :3].astype(np.float64), axis=1)
    assert (np.abs(dlen - 1.0) > 1e-3).sum() == 1 and (np.abs(dlen - 1.0) < 1e-6).sum() == 63
    try:
        ctx.set_cluster_size(k)
        ctx.set_cluster_tree(b)
        ctx.set_scene(w["scene"])
        check_casts(ctx.cast_rays(w["o"][sel], w["d"][sel], hits=True), w, sel, "one wave, one never-culling lane")
    finally:
        ctx.set_cluster_size(spt._native.CLUSTER_AUTO)
        ctx.set_cluster_tree(spt._native.TREE_AUTO)
