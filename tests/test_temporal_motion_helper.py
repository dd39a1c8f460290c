"""The motion rule's definition itself (tests/temporal_motion.py, the numpy restatement the GPU
tests compare against), checked on the CPU against the oracle alone: where a sphere moved it
has to find more history than the plain definition, find it on the same point of the sphere,
and bring the frame closer to the converged image; everywhere else it has to be the plain
definition, bit for bit.

Scene A is the golden `random` scene.  Scene B is scene A with its three spheres of radius 3
moved -- sphere 2 at (5, 3, 5) by (1.5, 0, 0.9), sphere 1 at (0, 3, 10) by (-1.2, 0.6, 0),
sphere 3 at (-7, 3, 14) by (0, 0.6, 0) with its radius times 1.25 -- and every other sphere
with index % 3 == 0 and a radius below 1 moved by (0.6, 0, 0.3).  The history frame is scene A
with seed 3, the current frame scene B with seed 4, 45 x 37 x 7, depth 8, the cameras those of
tests/test_temporal_helper.py: camera 0 -> camera 1 ("moving"), and camera 0 twice ("static").

Measured with this helper, moving / static camera: 419 / 402 of the 1 665 pixels lie on a moved
sphere (mv), 998 / 1 020 on one that stood still, 248 / 243 are sky and 70 / 66 have cov > 0
with id == n.  Of the mv pixels 349 / 334 find history under the motion rule, 108 / 55 under
the plain definition.  RMSE over the mv pixels against the oracle's 300-spp image of scene B
(seed 103): raw 10.23 / 10.56, plain 10.53 / 10.62, motion rule 9.75 / 9.35; over the whole
frame raw 7.48 / 7.56, plain 7.58 / 7.50, motion rule 7.32 / 7.08.  The sphere-local geometry
check: the history found lies 0.14 / 0.12 of a pixel footprint (2 z / height) from the pixel's
own point of the sphere in the median under the motion rule (314 / 291 pixels), 1.79 / 1.57
under the plain definition (99 / 52).
"""
import numpy as np

from denoise import rmse
from features import expected_features
from moments import expected_moments
from temporal import DEFAULTS, expected_temporal, inverse3, reproject
from temporal_motion import expected_temporal_motion, motion_table
from test_gpu_features import DEPTH, SEED
from test_gpu_parity import SKY, bits
from test_temporal_helper import REF_SEED, REF_SPP, camera, scene_arrays

F = np.float32
W1, H1, S1 = 45, 37, 7
BIG = {2: ((5, 3, 5), (1.5, 0, 0.9), 1.0), 1: ((0, 3, 10), (-1.2, 0.6, 0), 1.0), 3: ((-7, 3, 14), (0, 0.6, 0), 1.25)}
SMALL_SHIFT = (0.6, 0, 0.3)
PAIRS = {"moving": (0, 1), "static": (0, 0)}

_frames = {}


def scene_b(golden_scenes):
    """Scene B's five arrays (the docstring's), scene A's but for centers and radii."""
    centers, radii, colors, materials, fuzz = (np.array(a) for a in scene_arrays(golden_scenes))
    centers, radii = centers.astype(F).reshape(len(radii), 4), radii.astype(F)
    for k, (at, by, scale) in BIG.items():
        assert radii[k] == 3 and tuple(centers[k, :3]) == at, (k, centers[k], radii[k])
        centers[k, :3] += np.asarray(by, F)
        radii[k] *= F(scale)
    small = [k for k in range(len(radii)) if k % 3 == 0 and k not in BIG and radii[k] < 1]
    assert len(small) >= 10
    centers[small, :3] += np.asarray(SMALL_SHIFT, F)
    return centers, radii, colors, materials, fuzz


def scene_of(golden_scenes, which):
    return scene_arrays(golden_scenes) if which == "A" else scene_b(golden_scenes)


def table(golden_scenes, now="B", prev="A"):
    a, b = scene_of(golden_scenes, now), scene_of(golden_scenes, prev)
    return motion_table(a[0], a[1], b[0], b[1])


def oracle_frame(oracle, golden_scenes, which, cam, W, H, spp, seed, moments=True):
    """The oracle's frame of scene `which` ("A" / "B") seen by camera `cam` (0, 1, 2, or a
    (view, eye) pair), as test_temporal_helper.oracle_frame's dict; computed once."""
    view, eye = camera(golden_scenes, cam) if isinstance(cam, int) else cam
    key = (which, bits(view).tobytes(), bits(eye).tobytes(), W, H, spp, seed, moments)
    if key not in _frames:
        arrays = scene_of(golden_scenes, which)
        osc = oracle.OracleScene(*arrays)
        fr = oracle.make_frame(view, eye, SKY, W, H, spp, DEPTH, seed)
        rgba, _ = oracle.render_segment(osc, fr, 0, H, 0, W)
        f = dict(rgba=rgba.reshape(H, W, 4), view=view, eye=eye)
        if moments:
            col = oracle.trace_region(osc, fr, 0, H, 0, W)[0]
            w = expected_features(oracle, osc, fr, arrays, (0, H, 0, W))
            f.update(mom=expected_moments(col).reshape(H, W, 4), feat=w["feat"].reshape(H, W, 2, 4), ids=w["ids"].reshape(H, W))
        _frames[key] = f
    return _frames[key]


def pair(oracle, golden_scenes, W, H, spp, cams=(0, 1)):
    """(history frame: scene A, cams[0], seed 3; current frame: scene B, cams[1], seed 4)."""
    return (oracle_frame(oracle, golden_scenes, "A", cams[0], W, H, spp, SEED),
            oracle_frame(oracle, golden_scenes, "B", cams[1], W, H, spp, SEED + 1))


def accumulate(cur, prev, motion, minv=None, **kw):
    """expected_temporal_motion of `cur` against the history frame `prev`; motion None: the
    plain definition (expected_temporal)."""
    history = kw.pop("history", (prev["rgba"], prev["mom"], prev["feat"], prev["ids"]))
    H, W = cur["ids"].shape
    minv = inverse3(prev["view"]) if minv is None else minv
    args = (cur["rgba"], cur["mom"], cur["feat"], cur["ids"], cur["view"], cur["eye"], W, H)
    if motion is None:
        return expected_temporal(*args, history, prev["view"], prev["eye"], minv, **kw)
    return expected_temporal_motion(*args, motion, history, prev["view"], prev["eye"], minv, **kw)


def same_bits(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def local_distance(cur, prev, motion, use_motion):
    """The sphere-local geometry check: the history's colour is the previous frame's hit point
    in its sphere's own frame, (P_prev - Cp_id) / rp_id, with count 1e6, so the output colour
    is where on the sphere the history came from; returns its distance from the pixel's own
    (P - C_id) / r_id in pixel footprints (2 z / height), over the fully covered mv pixels
    that found history."""
    H, W = cur["ids"].shape
    n = len(motion)
    P_prev = reproject(prev["feat"], prev["view"], prev["eye"], W, H, inverse3(prev["view"]), prev["eye"])[4]
    P_cur = reproject(cur["feat"], cur["view"], cur["eye"], W, H, inverse3(prev["view"]), prev["eye"])[4]
    pid, cid = np.minimum(prev["ids"], n - 1), np.minimum(cur["ids"], n - 1)
    loc_prev = (P_prev.astype(np.float64) - motion[pid][..., 4:7]) / motion[pid][..., 7:8]
    loc_cur = (P_cur.astype(np.float64) - motion[cid][..., 0:3]) / motion[cid][..., 3:4]
    h_rgba = np.concatenate([loc_prev, np.zeros((H, W, 1))], axis=2).astype(F)
    h_mom = prev["mom"].copy()
    h_mom[..., 3] = F(1e6)
    out, _, info = accumulate(cur, prev, motion if use_motion else None, history=(h_rgba, h_mom, prev["feat"], prev["ids"]),
                              tol_normal=0.25, tol_depth=0.1, max_history=1e6)
    mv = accumulate(cur, prev, motion, **DEFAULTS)[2]["mv"]
    sel = mv & info["has"] & (cur["feat"][:, :, 0, 3] == 1)
    r = motion[cid][..., 3][sel].astype(np.float64)
    z = cur["feat"][:, :, 1, 3][sel].astype(np.float64)
    dist = np.linalg.norm(out[sel][:, :3].astype(np.float64) - loc_cur[sel], axis=1) * np.abs(r)
    return dist / (2.0 * z / H), int(sel.sum())


def test_the_motion_rule_on_the_two_pairs(oracle, golden_scenes):
    motion = table(golden_scenes)
    n = len(motion)
    for name, cams in PAIRS.items():
        prev, cur = pair(oracle, golden_scenes, W1, H1, S1, cams)
        plain = accumulate(cur, prev, None, **DEFAULTS)
        moved = accumulate(cur, prev, motion, **DEFAULTS)
        mv, hit = moved[2]["mv"], cur["feat"][:, :, 0, 3] > 0
        pops = [int(mv.sum()), int((hit & ~mv).sum()), int((~hit).sum()), int((hit & (cur["ids"] == n)).sum())]
        found = int((moved[2]["has"] & mv).sum()), int((plain[2]["has"] & mv).sum())
        ref = oracle_frame(oracle, golden_scenes, "B", cams[1], W1, H1, REF_SPP, REF_SEED, moments=False)["rgba"]
        err = {k: rmse(img[mv], ref[mv]) for k, img in (("raw", cur["rgba"]), ("plain", plain[0]), ("motion", moved[0]))}
        whole = {k: rmse(img, ref) for k, img in (("raw", cur["rgba"]), ("plain", plain[0]), ("motion", moved[0]))}
        rel_m, n_m = local_distance(cur, prev, motion, True)
        rel_p, n_p = local_distance(cur, prev, motion, False)
        print(f"motion {name} camera 45x37x7: mv / !mv hit / sky / cov > 0 with id == n = {pops}; history on mv pixels "
              f"{found[0]} (plain {found[1]}); RMSE over mv pixels raw {err['raw']:.2f} plain {err['plain']:.2f} motion "
              f"{err['motion']:.2f}; whole frame raw {whole['raw']:.2f} plain {whole['plain']:.2f} motion {whole['motion']:.2f}; "
              f"median distance in footprints motion {np.median(rel_m):.2f} ({n_m} pixels) plain {np.median(rel_p):.2f} ({n_p})")
        assert all(p >= 1 for p in pops), pops
        assert found[0] >= 2 * found[1] and found[1] >= 1, found
        assert n_m >= 50 and n_p >= 10
        assert np.median(rel_m) < 0.5 and np.median(rel_p) > 1.0, (np.median(rel_m), np.median(rel_p))
        assert err["motion"] < err["raw"] and err["motion"] < err["plain"], err
        # every pixel whose sphere did not move keeps the plain definition's bits
        assert np.array_equal(bits(moved[0][~mv]), bits(plain[0][~mv])) and np.array_equal(bits(moved[1][~mv]), bits(plain[1][~mv]))
        assert (bits(moved[0][mv]) != bits(plain[0][mv])).any()


def test_a_table_in_which_nothing_moved_is_the_plain_definition(oracle, golden_scenes):
    still = table(golden_scenes, "B", "B")
    for cams in PAIRS.values():
        prev, cur = pair(oracle, golden_scenes, W1, H1, S1, cams)
        plain = accumulate(cur, prev, None, **DEFAULTS)
        for motion in (still, np.zeros((0, 8), F)):
            got = accumulate(cur, prev, motion, **DEFAULTS)
            assert not got[2]["mv"].any() and same_bits(got, plain)
            assert np.array_equal(got[2]["has"], plain[2]["has"])
