"""tests/prim_cones.py (the cone test of the primary-ray candidate lists in float64 numpy, with
each pair's margin) against the library's host builder through spt_prim_lists_check, on the
scenes, cameras and frames of tests/test_prim_lists.py: the host's lists are exactly the pairs
with margin >= 0, ascending, padded to groups of 4 with a dummy slot; blocks whose cone is
unusable or whose list is longer than 24 walk.  No GPU.

The two sides compute the same fp64 expressions in the same order; they can part only where
numpy's atan2 / asin and the C library's round a pair across its bound, which the margins
themselves would show (a pair at |margin| < 1e-12): none of these scenes has one."""
import numpy as np
import pytest

import prim_cones
from test_prim_lists import EYE, WALK, prim_lists


@pytest.fixture(scope="module")
def spt_mod():
    import simplepathtracer_amd as spt
    return spt


def check_lists(native, scene, view, eye, W, H, sample=None, seed=1):
    """Every block's list (or `sample` random blocks per level) against the restatement."""
    b8, b4, ids, orig, on = prim_lists(native, scene.centers, scene.radii, view, eye, W, H)
    assert on
    slots4 = prim_cones.slot_table(scene.centers, scene.radii, orig)
    rng = np.random.default_rng(seed)
    lists = walks = 0
    for level, tab in ((0, b8), (1, b4)):
        assert len(tab) == len(prim_cones.block_rects(W, H, level))
        blocks = None if sample is None or sample >= len(tab) else np.sort(rng.choice(len(tab), sample, replace=False))
        want = prim_cones.expected_lists(slots4, view, eye, W, H, level, blocks)
        for blk, exp in want.items():
            first, cnt = int(tab[blk][0]), int(tab[blk][1])
            if exp is None:
                assert cnt == WALK, (level, blk)
                walks += 1
                continue
            assert cnt != WALK and cnt % 4 == 0 and cnt - len(exp) in (0, 1, 2, 3), (level, blk, cnt, len(exp))
            run = ids[first:first + cnt]
            assert np.array_equal(run[:len(exp)], exp), (level, blk, run, exp)
            assert (slots4[run[len(exp):], 3] == -np.inf).all(), (level, blk)  # padded with a dummy slot
            lists += 1
    return lists, walks


def test_config2_scene_default_camera(native, spt_mod):
    lists, walks = check_lists(native, spt_mod.generate_spheres(1), spt_mod.camera_basis(), spt_mod.scene.DEFAULT_EYE,
                               1200, 800)
    assert lists + walks == 45000 and lists > 40000


@pytest.mark.parametrize("eye,look", [([4.0, 1.0, 3.0, 0.0], [4.0, 1.0, 0.0, 0.0]),
                                      ([0.3, 0.25, 0.4, 0.0], [3.0, 0.2, 2.0, 0.0]),
                                      ([0.0, 30.0, 0.1, 0.0], [0.0, 0.0, 0.0, 0.0]),
                                      ([0.0, 1.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0])])
def test_other_cameras(native, spt_mod, eye, look):
    view = spt_mod.camera_basis(eye, look, [0.0, 1.0, 0.0, 0.0])
    check_lists(native, spt_mod.generate_spheres(1), view, eye, 320, 200)


def test_ragged_frame(native, spt_mod):
    check_lists(native, spt_mod.generate_spheres(2), spt_mod.camera_basis(), spt_mod.scene.DEFAULT_EYE, 203, 117)


def test_stress_and_small_scenes(native, spt_mod):
    check_lists(native, spt_mod.generate_stress(3, 300), spt_mod.camera_basis(), spt_mod.scene.DEFAULT_EYE, 256, 160)
    v3 = spt_mod.camera_basis([0.0, 1.0, -3.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0])
    check_lists(native, spt_mod.cornell3(), v3, [0.0, 1.0, -3.0, 0.0], 200, 100)


def test_config5_stress_scene_sampled_blocks(native, spt_mod):
    """Config 5 at full size holds 10^9 (block, slot) pairs: 400 random blocks of each level."""
    lists, walks = check_lists(native, spt_mod.generate_stress(1, 10000), spt_mod.camera_basis(),
                               spt_mod.scene.DEFAULT_EYE, 1920, 1080, sample=400, seed=11)
    assert lists > 600


def test_margins_mark_dummies_and_untested_slots(spt_mod):
    """-inf for a dummy slot, +inf where the eye is inside a sphere's reach, finite otherwise."""
    slots4 = np.array([[0, 0, -5, 1], [0, 0, 0, -np.inf], [13, 2, 3, 4], [np.inf, 0, 0, 1]], np.float32)
    cn = prim_cones.cones(spt_mod.camera_basis(), 64, 64, prim_cones.block_rects(64, 64, 0)[:3])
    assert cn["ok"].all()
    m = prim_cones.margins(cn, slots4, EYE)
    assert np.isfinite(m[:, 0]).all() and (m[:, 1] == -np.inf).all() and (m[:, 2] == np.inf).all() and (m[:, 3] == np.inf).all()
