"""The frames of the render kernels' regime sweep (tests/render_regimes.py) are worth rendering -- shown on the CPU oracle alone, scene
seed 0, 20 x 34 x 6 spp at depth 12, both stream modes.  tests/test_gpu_render_regimes.py holds the kernels to the oracle on
exactly these frames.
  1. every (regime, camera) frame is a real frame: the oracle scatters on all three materials, the canvas is no flat colour, and no
     frame but `tele` and `behind` at 1e9 holds a NaN;
  2. the frames from 1e9 units away do hold NaNs (measured: 1257 .. 1905 of 2040 values) beside at least 100 finite values; on the
     `behind` cameras the padding sphere of the layouts (centre 0, r^2 = -1) has a discriminant > 0 in plain float64 on 64 .. 505 of
     the 680 pixel-centre rays, and it lies in front of the scene;
  3. on every `closeup` camera at least a quarter of the pixel-centre rays at time 0 cross 64 or more spheres (measured: 638 of 680 on
     dense and dense_ties, 595 on dense2; up to 397 spheres on one ray): more than a candidate queue or a pooled list (576) holds;
  4. on dense_ties/closeup, exchanging every duplicate with its original in the list changes the oracle's canvas in at least 16
     pixels, in both stream modes (measured: 158 and 139 of 680; the whole-scene camera shows 2): the canvas says which of two
     coincident spheres won.
And the layouts are what the sweep's family count relies on: which regimes are two-level, and which carry several time groups."""
import numpy as np
import pytest

import render_regimes as R

SEED = 0
_frames = {}


def _frame(oracle, name, cam, seeding, recs=None):
    key = (name, cam, seeding)
    if recs is not None or key not in _frames:
        scene = R.scene(name, SEED) if recs is None else recs
        ocam = R.oracle_camera(oracle, R.camera(name, cam, R.scene(name, SEED)))
        res = oracle.render(R.H, R.W, R.SPP, ocam, scene, max_depth=R.DEPTH, seeding=seeding, math=oracle.MATH_PORTABLE, accum=seeding,
                            collect_stats=True)
        if recs is not None:
            return res
        res.pixels.setflags(write=False)
        _frames[key] = res
    return _frames[key]


def test_the_issues_regimes_and_cameras_are_all_there():
    assert set(R.ISSUE_REGIMES) <= set(R.REGIMES) and "needle" not in R.REGIMES and "reach_split" not in R.REGIMES
    for name in R.REGIMES:
        names = R.camera_names(name)
        assert names[:2] == ["outside", "inside"]
        assert ("closeup" in names) == (name in ("dense", "dense_ties", "dense2"))
        assert [n for n in names if n.startswith("tele")] == (["tele_1e+06", "tele_1.1e+06", "tele_1e+09"] if name in ("dense", "groups") else [])
        assert (R.BEHIND in names) == (name in ("far", "dense2", "far_x5"))
    assert R.H * R.W * R.SPP == 64 * 64 - 16               # 64 waves of samples, the last one short
    dense, ties = R.scene("dense", SEED), R.scene("dense_ties", SEED)
    assert np.array_equal(dense[:, :10], ties[:, :10]) and np.array_equal(dense[:-24], ties[:-24])
    assert (dense[-24:, 10] != ties[-24:, 10]).all() and (dense[-24:, 11:14] != ties[-24:, 11:14]).all()
    assert len(R.duplicate_pairs(ties)) == 24


@pytest.mark.parametrize("name,cam", R.CASES)
def test_every_frame_is_a_real_frame(oracle, name, cam):
    for seeding in (0, 1):
        res = _frame(oracle, name, cam, seeding)
        st, px = res.stats, res.pixels
        nans = int(np.isnan(px).sum())
        print(f"{name}/{cam} seeding {seeding}: scatters {st.scatter_lambertian} / {st.scatter_metal} / {st.scatter_dielectric}, "
              f"{nans} NaN, std {np.nanstd(px):.3f}")
        assert min(st.scatter_lambertian, st.scatter_metal, st.scatter_dielectric) > 0
        assert np.nanstd(px) > 0.05
        if cam.endswith("1e+09"):
            assert nans >= 1 and int(np.isfinite(px).sum()) >= 100
        else:
            assert nans == 0


@pytest.mark.parametrize("name", R.CLOSEUP_REGIMES)
def test_closeup_rays_cross_more_spheres_than_a_list_holds(name):
    recs = R.scene(name, SEED)
    o, d = R.pixel_centre_rays(R.camera(name, "closeup", recs))
    n = R.spheres_crossed(recs, o, d, time=0.0)
    print(f"{name}/closeup: {int((n >= 64).sum())} of {n.size} pixel-centre rays cross 64 or more spheres, the most {int(n.max())}")
    assert n.size == R.H * R.W and (n >= 64).mean() >= 0.25


@pytest.mark.parametrize("name", R.BEHIND_REGIMES)
def test_behind_cameras_see_the_padding_sphere_in_front_of_the_scene(name):
    """A record of centre 0 and r^2 = -1 is "never hit" only while |o|^2 + 1 != |o|^2."""
    kw = R.camera(name, R.BEHIND, R.scene(name, SEED))
    o, d = R.pixel_centre_rays(kw)
    hb, a, cc = (o * d).sum(axis=1), (d * d).sum(axis=1), (o * o).sum() + 1.0
    hits = int((hb * hb - a * cc > 0).sum())
    print(f"{name}/{R.BEHIND}: the padding sphere has a discriminant > 0 on {hits} of {len(d)} pixel-centre rays")
    assert cc == (o * o).sum() and hits >= 32              # measured: 505 (far), 400 (dense2), 64 (far_x5)
    assert np.linalg.norm(o) < np.linalg.norm(o - np.array(kw["look_at"]))   # the world origin is nearer than the scene


def test_the_canvas_tells_which_duplicate_won(oracle):
    ties = R.scene("dense_ties", SEED)
    other = R.swapped(ties)
    assert sorted(map(tuple, other)) == sorted(map(tuple, ties)) and not np.array_equal(other, ties)
    for seeding in (0, 1):
        a = _frame(oracle, "dense_ties", "closeup", seeding).pixels
        b = _frame(oracle, "dense_ties", "closeup", seeding, recs=other).pixels
        changed = int((a != b).any(axis=2).sum())
        print(f"dense_ties/closeup seeding {seeding}: {changed} of {R.H * R.W} pixels change when the duplicates come first")
        assert changed >= 16


def test_layout_facts_the_family_count_relies_on(tor):
    """Two-level layouts, time groups among the blocks' movers and the build both accelerations call for, per regime."""
    two_level, several, both = set(), set(), {}
    for name in R.REGIMES:
        recs = R.scene(name, SEED)
        lay = tor.debug_accel_layout(tor.Scene.from_records(recs).list(), min(0.0, R.SHUTTER[0]), max(0.0, R.SHUTTER[1]))
        assert lay is not None, name
        if lay[3]:
            two_level.add(name)
        if len(R.time_groups_in_blocks(recs, lay)) > 1:
            several.add(name)
        both[name] = R.expected_variant(recs, lay, 3, 0)[1:]
        assert R.expected_variant(recs, lay, 0, 1) == (1, 2, 0, 0) and R.expected_variant(recs, lay, 0, 1, screen=False) == (1, 0, 0, 0)
        assert R.expected_variant(recs, lay, 1, 0) == (0, 0, 0, 1) and R.expected_variant(recs, lay, 2, 0) == (0, 0, 1, 0)
    assert two_level == {"dense2"} | set(R.TILED)
    assert several == {"huge_far", "groups", "noground", "huge_far_x3", "groups_x2", "noground_x12"}
    assert {n for n, v in both.items() if v == (0, 1, 1)} == {"tiny", "far", "dense", "dense_ties"}
    assert {n for n, v in both.items() if v == (0, 1, 2)} == {"tiny_x5", "far_x5", "dense_x2"}
    # the rest runs the float64 block expansion: several time groups, or (dense2: one sphere beyond 8 x the median distance from the
    # filter's origin; odd_objects: the mover displaced by 1e200) an object in the blocks that the float32 filter may not take
    assert {n for n, v in both.items() if v == (0, 0, 1)} == several | {"dense2", "odd_objects"}
