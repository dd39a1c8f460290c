"""Scene updates on the device (spt_update_scene, include/spt_hip.h "scene updates", DESIGN.md
§4.16): a context whose spheres and camera were moved by update_scene -- traversal tables
refit, candidate lists built by the kernel -- computes what a fresh context given set_scene
and set_camera for the moved state computes, on float bits and bytes; the device's lists are
sound (the oracle's winner of a primary ray is in its block's list) and are the host
builder's, except where a device atan2 / asin rounds a (block, slot) pair across its bound:
such a pair's margin (tests/prim_cones.py) is below 1e-9 rad, and such blocks are at most 1 in
1 000.  No comparison has another tolerance.

Frames are 75 x 37 at 4 spp and 8 bounces: two super-blocks in x, the second 11 columns wide
with a 3-pixel last block, a 5-row last 8-block and a 1-row last 4-block; 7 x 3 and 64 x 64
besides."""
import ctypes

import numpy as np
import pytest

import prim_cones
from cast_rays import make_rays
from test_gpu_parity import SKY, bits
from test_refit_abi import moves

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, DEPTH, SEED = 75, 37, 4, 8, 3
WALK = 0xFFFFFFFF
UP = [0.0, 1.0, 0.0, 0.0]
EYE0, LOOK0 = [0.0, 1.0, -3.0, 0.0], [0.0, 1.0, 0.0, 0.0]
EYE1, LOOK1 = [0.4, 1.3, -2.6, 0.0], [0.2, 0.8, 0.0, 0.0]
OTHER_CAMERAS = [([4.0, 1.0, 3.0, 0.0], [4.0, 1.0, 0.0, 0.0]),   # tests/test_prim_lists.py test_other_cameras
                 ([0.3, 0.25, 0.4, 0.0], [3.0, 0.2, 2.0, 0.0]),
                 ([0.0, 30.0, 0.1, 0.0], [0.0, 0.0, 0.0, 0.0]),
                 ([0.0, 1.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0])]


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


def cam(spt, eye, look):
    return spt.camera_basis(eye, look, UP), eye


def moved_scene(spt, scene, centers):
    return spt.Scene(np.ascontiguousarray(centers, F), scene.radii, scene.colors, scene.materials, scene.fuzz)


def make_ctx(spt, scene, camera, frame=(W, H, SPP), tree=None, devices=None):
    c = spt.Context(0) if devices is None else spt.Context(devices=devices)
    if tree is not None:
        c.set_cluster_tree(tree)
    c.set_scene(scene)
    c.set_camera(camera[0], camera[1], SKY)
    c.set_params(frame[0], frame[1], frame[2], DEPTH, SEED)
    return c


def outputs(c, rays, frame=(W, H, SPP)):
    """Everything a state computes: a render (float pixels and g_data bytes), ray queries with
    hit records, path queries, feature buffers with ids."""
    w, h, _ = frame
    g = np.zeros(w * h * 3, np.uint8)
    px = c.render_segment(0, h, 0, w, g)
    o, d = rays
    idx, hit = c.cast_rays(o, d, hits=True)
    tr = c.trace_rays(o, d, DEPTH, seed=7)
    feat, ids = c.render_features(0, h, 0, w, ids=True)
    return dict(pixels=bits(px), g_data=g, cast_idx=idx, cast_hit=bits(hit), trace=bits(tr), feat=bits(feat), ids=ids)


def assert_same(got, want, what):
    for k in want:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs in {int((got[k] != want[k]).sum())} of {got[k].size}"


def rays_for(scene, n=1031):
    o, d, _, _ = make_rays(scene.centers, scene.radii, n=n)
    return o, d


def parity(spt, scene, centers_b, cam0, cam1, what, frame=(W, H, SPP), tree=None, devices=None, lists="device",
           rays_of=None):
    """update_scene(B, cam1) on a context set up for (scene, cam0) against a fresh context for
    (B, cam1); returns the update's info."""
    b = scene if centers_b is None else moved_scene(spt, scene, centers_b)
    rays = rays_for(scene if rays_of is None else rays_of)
    upd = make_ctx(spt, scene, cam0, frame, tree, devices)
    fresh = make_ctx(spt, b, cam1 if cam1 is not None else cam0, frame, tree)
    try:
        outputs(upd, rays, frame)  # the state before the move has rendered: tables and lists are in use
        info = upd.update_scene(None if centers_b is None else b.centers, *(cam1 if cam1 is not None else (None, None)))
        assert_same(outputs(upd, rays, frame), outputs(fresh, rays, frame), what)
        assert info["refit"] == (0 if centers_b is None else 1)
        assert (info["lists_on_device"], info["lists_reason"]) == ((1, "device") if lists == "device" else (0, lists)), info
        if lists == "device":
            st = upd.stats()
            assert (info["list_blocks"], info["list_entries"]) == (st["prim_list_blocks"], st["prim_list_entries"])
            assert info["list_blocks"] > 0 or frame[0] * frame[1] < 64  # a 7 x 3 frame's one block may walk
        return info
    finally:
        upd.close()
        fresh.close()


# ---------------------------------------------------------------- parity

@pytest.mark.parametrize("move", ("jitter", "permutation", "far"))
def test_wave_walk_tree_with_lists(spt, move):
    sc = spt.generate_spheres(1)
    parity(spt, sc, moves(sc)[move], cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), move)


@pytest.mark.parametrize("frame", ((7, 3, 4), (64, 64, 4)))
def test_other_frames(spt, frame):
    sc = spt.generate_spheres(1)
    parity(spt, sc, moves(sc)["jitter"], cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), str(frame), frame=frame)


def test_brute_force_scene(spt):
    sc = spt.cornell3()
    parity(spt, sc, moves(sc)["jitter"], cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), "cornell3")


@pytest.mark.parametrize("move", ("jitter", "permutation"))
def test_flat_list(spt, move):
    sc = spt.generate_spheres(1)
    parity(spt, sc, moves(sc)[move], cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), "flat " + move, tree=0)


def test_stress_scene_wave_walk(spt):
    sc = spt.generate_stress(3, 300)
    parity(spt, sc, moves(sc)["jitter"], cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), "stress 300")


@pytest.mark.parametrize("move", ("jitter", "permutation"))
def test_lds_lane_walk_refit_only(spt, move):
    sc = spt.generate_stress(3, 600)
    info = parity(spt, sc, moves(sc)[move], cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), "stress 600 " + move, lists="off")
    assert info["list_blocks"] == 0 and info["lists_ms"] == 0


@pytest.mark.parametrize("move", ("jitter", "permutation"))
def test_global_lane_walk_refit_only(spt, move):
    sc = spt.generate_stress(2, 20000)
    parity(spt, sc, moves(sc)[move], cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), "stress 20000 " + move, frame=(24, 16, 2),
           lists="off")


def test_camera_only_and_centres_only(spt):
    sc = spt.generate_spheres(1)
    info = parity(spt, sc, None, cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), "camera only")
    assert info["refit_ms"] == 0
    parity(spt, sc, moves(sc)["jitter"], cam(spt, EYE0, LOOK0), None, "centres only")


def test_ten_updates_in_a_row(spt):
    sc = spt.generate_spheres(1)
    rng = np.random.default_rng(9)
    c = np.array(sc.centers, F, copy=True)
    upd = make_ctx(spt, sc, cam(spt, EYE0, LOOK0))
    try:
        for k in range(10):
            c[:, :3] += rng.normal(0.0, 0.05, (sc.n, 3)).astype(F)
            eye = [0.1 * k, 1.0 + 0.05 * k, -3.0 + 0.1 * k, 0.0]
            info = upd.update_scene(c, *cam(spt, eye, LOOK1))
            assert info["lists_on_device"] == 1 and info["refit"] == 1
            if k in (0, 4, 9):
                g = np.zeros(W * H * 3, np.uint8)
                upd.render_segment(0, H, 0, W, g)
        b = moved_scene(spt, sc, c)
        fresh = make_ctx(spt, b, cam(spt, eye, LOOK1))
        try:
            rays = rays_for(sc)
            assert_same(outputs(upd, rays), outputs(fresh, rays), "after ten updates")
        finally:
            fresh.close()
    finally:
        upd.close()


def test_eye_inside_a_spheres_reach_and_a_sphere_on_the_eye(spt):
    sc = spt.generate_spheres(1)
    big = int(np.argmax(np.where(sc.radii < 100, sc.radii, 0)))  # one of the r = 1 balls
    inside = (np.array(sc.centers[big], F) + F([0.0, 0.0, 0.5, 0.0])).tolist()
    parity(spt, sc, moves(sc)["jitter"], cam(spt, EYE0, LOOK0), cam(spt, inside, LOOK1), "eye inside a ball")
    c = np.array(sc.centers, F, copy=True)
    small = int(np.argmin(sc.radii))
    c[small, :3] = F(EYE1[:3])
    parity(spt, sc, c, cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), "a sphere on the eye")


def test_multi_member_context(spt):
    sc = spt.generate_spheres(1)
    b = moved_scene(spt, sc, moves(sc)["jitter"])
    cam0, cam1 = cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1)
    parity(spt, sc, b.centers, cam0, cam1, "devices [0, 0]", devices=[0, 0])
    upd, fresh = make_ctx(spt, sc, cam0, devices=[0, 0]), make_ctx(spt, b, cam1)
    try:
        upd.update_scene(b.centers, *cam1)
        got = upd.render_frame()  # strips on both members
        want = fresh.render_segment(0, H, 0, W)
        assert np.array_equal(bits(got), bits(want))
    finally:
        upd.close()
        fresh.close()


def test_a_refused_move_leaves_the_state(spt):
    sc = spt.generate_spheres(1)
    c0 = cam(spt, EYE0, LOOK0)
    upd = make_ctx(spt, sc, c0)
    try:
        rays = rays_for(sc)
        before = outputs(upd, rays)
        for bad in (np.nan, np.inf):
            c = np.array(sc.centers, F, copy=True)
            c[sc.n // 2, 2] = bad
            with pytest.raises(spt.SptError) as e:
                upd.update_scene(c, *cam(spt, EYE1, LOOK1))
            assert e.value.code == 1 and "not finite" in str(e.value)
            assert_same(outputs(upd, rays), before, "after a refused move")
        view = np.ascontiguousarray(cam(spt, EYE1, LOOK1)[0], F)
        assert spt.lib().spt_update_scene(upd.handle, None, view.ctypes.data_as(ctypes.c_void_p), None, None) == 1  # no eye
        tilted = view.copy()
        tilted[13] = 1.0
        eye = np.asarray(EYE1, F)
        assert spt.lib().spt_update_scene(upd.handle, None, tilted.ctypes.data_as(ctypes.c_void_p),
                                          eye.ctypes.data_as(ctypes.c_void_p), None) == 1  # viewMatrix row 3 not zero
        assert_same(outputs(upd, rays), before, "after a refused camera")
    finally:
        upd.close()


def test_before_a_scene_is_a_state_error(spt):
    c = spt.Context(0)
    try:
        with pytest.raises(spt.SptError) as e:
            c.update_scene(np.zeros((3, 4), F))
        assert e.value.code == 2
        with pytest.raises(spt.SptError) as e:
            c.update_scene(None, *cam(spt, EYE1, LOOK1))
        assert e.value.code == 2
    finally:
        c.close()


def test_the_folds_colour_table_survives_an_update(spt):
    import torch
    sc = spt.generate_spheres(1)
    upd = make_ctx(spt, sc, cam(spt, EYE0, LOOK0))
    d = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def launched_render():  # a launched render builds the table where it is stale (a batched host call does not)
        upd.render_rows_async(0, 0, H, 1, 1, 0, 0, W, d.data_ptr(), 0)
        upd.synchronize()
        return d.cpu().numpy()

    try:
        launched_render()
        n0 = upd.stats()["fold_table_entries"]
        assert n0 > 0
        b = moved_scene(spt, sc, moves(sc)["jitter"])
        upd.update_scene(b.centers, *cam(spt, EYE1, LOOK1))
        assert upd.stats()["fold_table_entries"] == n0  # still valid: the next render does not rebuild it
        got = launched_render()
        assert upd.stats()["fold_table_entries"] == n0
        fresh = make_ctx(spt, b, cam(spt, EYE1, LOOK1))
        try:
            assert np.array_equal(bits(got), bits(fresh.render_segment(0, H, 0, W)))  # the table fold of the moved scene
        finally:
            fresh.close()
    finally:
        upd.close()


def test_forced_fallback_to_the_host_builder(spt, monkeypatch):
    monkeypatch.setenv("SPT_PRIM_DEVICE_SLOTS", "64")  # generate_spheres(1) has 164 slots
    sc = spt.generate_spheres(1)
    info = parity(spt, sc, moves(sc)["jitter"], cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1), "host fallback", lists="slots")
    assert info["list_blocks"] > 0 and info["lists_ms"] == 0


# ---------------------------------------------------------------- the device's lists

def updated(spt, move, camera, frame=(W, H, SPP)):
    """A context moved by update_scene to (moved scene, camera), and the moved scene."""
    sc = spt.generate_spheres(1)
    b = sc if move is None else moved_scene(spt, sc, moves(sc)[move])
    c = make_ctx(spt, sc, cam(spt, EYE0, LOOK0), frame)
    info = c.update_scene(None if move is None else b.centers, *camera)
    assert info["lists_on_device"] == 1
    return c, b


def winners_in_lists(oracle, scene, camera, lists, w, h, spp, samples=3000, seed=1, focus=None):
    """check_winners' property (tests/test_prim_lists.py) on given lists: the oracle's winner of
    sampled primary rays is in its 8x8 and its 8x4 block's list wherever the block has one."""
    b8, b4, ids, orig, on = lists
    assert on
    view, eye = camera
    osc = oracle.OracleScene(scene.centers, scene.radii, scene.colors, scene.materials, scene.fuzz)
    fr = oracle.make_frame(view, eye, SKY, w, h, spp, 50, seed)
    rng = np.random.default_rng(seed)
    xs, ys = rng.integers(0, w, samples), rng.integers(0, h, samples)
    if focus is not None:
        x0, y0, x1, y1 = focus
        xs[: samples // 2] = rng.integers(x0, x1, samples // 2)
        ys[: samples // 2] = rng.integers(y0, y1, samples // 2)
    ss = rng.integers(0, spp, samples)
    win = oracle.primary_winners(osc, fr, np.stack([xs, ys, ss], 1))
    slot_of = {int(o): s for s, o in enumerate(orig) if o != WALK}
    bw = (w + 7) // 8
    hits = 0
    for x, y, wn in zip(xs, ys, win):
        for blk in (b8[(y // 8) * bw + x // 8], b4[(y // 4) * bw + x // 8]):
            first, cnt = int(blk[0]), int(blk[1])
            if cnt == WALK or wn >= scene.n:
                continue
            hits += 1
            run = ids[first:first + cnt]
            assert slot_of[int(wn)] in run, f"pixel ({x}, {y}): winner {wn} (slot {slot_of[int(wn)]}) not in {run}"
    return hits


SOUND = [(m, (EYE1, LOOK1)) for m in ("jitter", "permutation", "far")] + [(None, c) for c in OTHER_CAMERAS]


@pytest.mark.parametrize("move,camera", SOUND, ids=[f"{m}-{k}" for k, (m, _) in enumerate(SOUND)])
def test_device_lists_hold_every_winner(spt, oracle, move, camera):
    camera = cam(spt, *camera)
    c, b = updated(spt, move, camera)
    try:
        hits = winners_in_lists(oracle, b, camera, c.prim_lists(0), W, H, SPP, focus=(20, 8, 60, 30))
        print(f"device lists, {move} from {camera[1]}: {hits} winners looked up")
        assert hits > 100  # rays that hit a sphere in blocks that have a list: the property was tested
    finally:
        c.close()


def compare_lists(spt, dev, host, slots4, camera, w, h):
    """Blocks whose device and host lists differ; asserts each differs only in pairs whose
    margin is below 1e-9 rad in magnitude."""
    differing = total = 0
    for level, (d, hb) in enumerate(((dev[0], host[0]), (dev[1], host[1]))):
        total += len(d)
        for blk in range(len(d)):
            runs = []
            for tab, ids in ((d, dev[2]), (hb, host[2])):
                first, cnt = int(tab[blk][0]), int(tab[blk][1])
                if cnt == WALK:
                    runs.append(None)
                    continue
                run = ids[first:first + cnt]
                assert cnt % 4 == 0 and (np.diff(run[slots4[run, 3] != -np.inf].astype(np.int64)) > 0).all()  # ascending, padded
                runs.append(set(int(s) for s in run if slots4[s, 3] != -np.inf))
            if runs[0] == runs[1]:
                continue
            differing += 1
            rect = prim_cones.block_rects(w, h, level)[blk:blk + 1]
            m = prim_cones.margins(prim_cones.cones(camera[0], w, h, rect), slots4, camera[1])[0]
            ms = prim_cones.margins(prim_cones.cones(camera[0], w, h, prim_cones.super_rects(w, h, rect)), slots4, camera[1])[0]
            close = set(np.flatnonzero((np.abs(m) < 1e-9) | (np.abs(ms) < 1e-9)).tolist())
            if runs[0] is None or runs[1] is None:  # one side's list passed the cap: a pair at the bound decided it
                assert close, f"level {level} block {blk}: walk against a list with no pair at a bound"
            else:
                assert (runs[0] ^ runs[1]) <= close, f"level {level} block {blk}: {sorted(runs[0] ^ runs[1])} differ, margins {m[sorted(runs[0] ^ runs[1])]}"
    return differing, total


@pytest.mark.parametrize("move,camera,frame", [("jitter", (EYE1, LOOK1), (W, H, SPP)), ("permutation", (EYE1, LOOK1), (W, H, SPP)),
                                               ("far", (EYE1, LOOK1), (W, H, SPP)), ("jitter", (EYE1, LOOK1), (323, 203, 1)),
                                               (None, OTHER_CAMERAS[1], (323, 203, 1)), (None, OTHER_CAMERAS[3], (323, 203, 1))],
                         ids=["jitter", "permutation", "far", "jitter-323x203", "low-323x203", "inside-323x203"])
def test_device_lists_are_the_host_builders(spt, move, camera, frame):
    camera = cam(spt, *camera)
    c, b = updated(spt, move, camera, frame)
    try:
        dev, host = c.prim_lists(0), c.prim_lists(1)
        assert dev[4] and host[4] and np.array_equal(dev[3], host[3])
        slots4 = prim_cones.slot_table(b.centers, b.radii, dev[3])
        differing, total = compare_lists(spt, dev, host, slots4, camera, frame[0], frame[1])
        print(f"device against host lists, {move} {frame[0]}x{frame[1]}: {differing} of {total} blocks differ")
        assert differing <= total // 1000
        again = compare_lists(spt, host, c.prim_lists(1), slots4, camera, frame[0], frame[1])
        assert again[0] == 0  # the host builder against itself
    finally:
        c.close()


# ---------------------------------------------------------------- the accumulator

def test_accumulator_with_refit_returns_the_same_images(spt):
    sc = spt.generate_spheres(1)
    w, h = 72, 40
    images = {}
    for refit in (False, True):
        ctx = spt.Context(0)
        try:
            acc = spt.TemporalAccumulator(ctx, w, h, SPP, DEPTH, seed=5, sky=SKY, resident=True, refit=refit)
            r = np.random.default_rng(4)
            c = np.array(sc.centers, F, copy=True)
            out = []
            for k in range(6):
                eye = [0.05 * k, 1.0, -3.0 + 0.04 * k, 0.0]
                view = spt.camera_basis(eye, LOOK0, UP)
                if k % 2 == 0:  # the spheres move (and the camera with them); odd frames move the camera alone
                    c[:, :3] += r.normal(0.0, 0.02, (sc.n, 3)).astype(F)
                    out.append(acc.frame(view, eye, scene=moved_scene(spt, sc, c.copy())).copy())
                else:
                    out.append(acc.frame(view, eye).copy())
            images[refit] = out
        finally:
            ctx.close()
    for k, (a, b) in enumerate(zip(images[False], images[True])):
        assert np.array_equal(bits(a), bits(b)), f"frame {k}"
    assert not np.array_equal(bits(images[True][0]), bits(images[True][5]))


# ---------------------------------------------------------------- setters and updates in turn

def launched_render(c, w=W, h=H):
    """A launched render: it builds the fold's colour table where that is stale (a batched host
    call does not), so fold_table_entries shows whether a step left the table standing."""
    import torch
    d = torch.zeros((w * h, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    c.render_rows_async(0, 0, h, 1, 1, 0, 0, w, d.data_ptr(), 0)
    c.synchronize()


def visible(c):
    st = c.stats()
    return (st["prim_list_builds"], st["prim_list_blocks"], st["prim_list_entries"], st["fold_table_entries"])


# (prim_list_builds, prim_list_blocks, prim_list_entries, fold_table_entries) after each step of
# cases 1-3, as the commit before the scene state had one owner gave them for these sequences
# (this test's body run against that commit's library on an MI355X); they pin that a refit
# leaves the colour table standing, that a setter rebuilds lists only when their key changed,
# and which builder (packed host runs, fixed-stride device runs) filled the counters
STEPS = {
    "params": [(1, 41, 588, 1312), (2, 48, 728, 1312), (3, 57, 1052, 1312), (3, 57, 1052, 1312)],
    "tree": [(2, 48, 728, 1312), (3, 48, 728, 0), (3, 48, 728, 1280), (4, 48, 756, 1280)],
    "camera": [(2, 48, 728, 1312), (2, 48, 728, 1312), (3, 41, 588, 1312)],
}


def same_as_fresh(spt, upd, scene, camera, what, frame=(W, H, SPP), tree=None, rays_of=None):
    fresh = make_ctx(spt, scene, camera, frame, tree)
    try:
        rays = rays_for(scene if rays_of is None else rays_of)
        assert_same(outputs(upd, rays, frame), outputs(fresh, rays, frame), what)
    finally:
        fresh.close()


def interleave_params(spt, a, b, cam0, cam1, seen):
    upd = make_ctx(spt, a, cam0)
    try:
        launched_render(upd)
        seen.append(visible(upd))
        upd.update_scene(b.centers, *cam1)
        seen.append(visible(upd))
        upd.set_params(64, 64, SPP, DEPTH, SEED)
        seen.append(visible(upd))
        same_as_fresh(spt, upd, b, cam1, "update, then set_params", frame=(64, 64, SPP), rays_of=a)
        seen.append(visible(upd))
    finally:
        upd.close()


def interleave_tree(spt, a, b, cam0, cam1, seen):
    upd = make_ctx(spt, a, cam0)
    try:
        launched_render(upd)
        upd.update_scene(b.centers, *cam1)
        seen.append(visible(upd))
        upd.set_cluster_tree(0)  # rebuilds from the context's host copy of the centres: the moved ones
        seen.append(visible(upd))
        same_as_fresh(spt, upd, b, cam1, "update, then set_cluster_tree(0)", tree=0, rays_of=a)
        launched_render(upd)
        seen.append(visible(upd))
        info = upd.update_scene(a.centers)
        assert info["refit"] == 1
        seen.append(visible(upd))
        same_as_fresh(spt, upd, a, cam1, "then update on the flat list", tree=0, rays_of=a)
    finally:
        upd.close()


def interleave_camera(spt, a, b, cam0, cam1, seen):
    upd = make_ctx(spt, a, cam0)
    try:
        launched_render(upd)
        info = upd.update_scene(b.centers, *cam1)
        assert info["lists_on_device"] == 1
        seen.append(visible(upd))
        before = upd.prim_lists(0)
        upd.set_camera(cam1[0], cam1[1], SKY)  # the values the update gave: the key stands
        seen.append(visible(upd))
        assert seen[-1][0] == seen[-2][0], "set_camera with the update's own camera built lists"
        for x, y in zip(upd.prim_lists(0), before):
            assert np.array_equal(x, y)
        upd.set_camera(cam0[0], cam0[1], SKY)
        seen.append(visible(upd))
        assert seen[-1][0] == seen[-2][0] + 1
        dev, host = upd.prim_lists(0), upd.prim_lists(1)
        assert dev[4] and host[4]
        for x, y in zip(dev, host):  # a setter's lists are the host builder's packed runs
            assert np.array_equal(x, y)
        same_as_fresh(spt, upd, b, cam0, "update, then set_camera", rays_of=a)
    finally:
        upd.close()


def interleave_sphere_count(spt, a, b, cam0, cam1, seen):
    upd = make_ctx(spt, a, cam0)
    try:
        upd.update_scene(b.centers)
        small = spt.cornell3()
        upd.set_scene(small)
        moved = moved_scene(spt, small, moves(small)["jitter"])
        info = upd.update_scene(moved.centers)
        assert info["refit"] == 1
        same_as_fresh(spt, upd, moved, cam0, "update, set_scene of 4 spheres, update")
    finally:
        upd.close()


def interleave_fallback(spt, a, b, cam0, cam1, seen, monkeypatch):
    monkeypatch.setenv("SPT_PRIM_DEVICE_SLOTS", "64")  # generate_spheres(1) has 164 slots
    host = make_ctx(spt, a, cam0)
    monkeypatch.delenv("SPT_PRIM_DEVICE_SLOTS")
    dev = make_ctx(spt, a, cam0)
    try:
        ih, idv = host.update_scene(b.centers, *cam1), dev.update_scene(b.centers, *cam1)
        assert (ih["lists_on_device"], ih["lists_reason"]) == (0, "slots")
        assert (idv["lists_on_device"], idv["lists_reason"]) == (1, "device")
        rays = rays_for(a)
        assert_same(outputs(host, rays), outputs(dev, rays), "host fallback against the device builder")
    finally:
        host.close()
        dev.close()


@pytest.mark.parametrize("case", ("params", "tree", "camera", "sphere_count", "fallback"))
def test_setters_and_updates_interleave(spt, monkeypatch, case):
    """Setters and spt_update_scene in turn on one context leave the state a fresh context
    given the same final state has; the counters spt_stats shows after every step of the
    first three sequences are the ones recorded in STEPS."""
    a = spt.generate_spheres(1)
    b = moved_scene(spt, a, moves(a)["jitter"])
    cam0, cam1 = cam(spt, EYE0, LOOK0), cam(spt, EYE1, LOOK1)
    seen = []
    body = {"params": interleave_params, "tree": interleave_tree, "camera": interleave_camera,
            "sphere_count": interleave_sphere_count}.get(case)
    if body is None:
        interleave_fallback(spt, a, b, cam0, cam1, seen, monkeypatch)
    else:
        body(spt, a, b, cam0, cam1, seen)
    print(f"interleave {case}: {seen}")
    if case in STEPS:
        assert seen == STEPS[case]
