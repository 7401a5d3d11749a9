"""The inputs of the query kernels' regime sweep (tests/query_regimes.py) are worth running -- shown on the CPU, with the numpy
restatements and the host's culling layout alone: per regime enough rays hit something other than the ground, cross many surfaces
and (dense) tie; every regime has a culling layout and only dense2 a two-level one; the restated reach is none for needle and
odd_objects, cuts through the ray origins for reach_split and is far larger than the scene elsewhere; the grazing rays do land on
the band in which the reference's rounding accepts a ray that passes outside the sphere; and the restatements agree with each other
on every regime.  tests/test_gpu_query_regimes.py compares the kernels with these restatements on these inputs.

Every floor below is half of what the restatements gave with the committed generator (scene seed 0, rays seed 7, reach rays seed 3);
the measured value stands beside it."""
import numpy as np
import pytest

import crossings_restatement as X
import hit_restatement as H
import masked_restatement as M
import query_regimes as Q

N_RAYS, SCENE_SEED, RAY_SEED, REACH_SEED = 2048, 0, 7, 3

# regime: (share of rays that hit something other than the ground, share with more than 4 crossings, with more than 16) -- measured
MEASURED = {
    "tiny":        (0.597, 0.264, 0.000),
    "far":         (0.570, 0.236, 0.000),
    "huge_far":    (0.727, 0.554, 0.020),
    "dense":       (0.589, 0.512, 0.494),
    "dense2":      (0.725, 0.558, 0.520),
    "groups":      (0.768, 0.610, 0.071),
    "noground":    (0.516, 0.042, 0.000),
    "needle":      (0.589, 0.512, 0.494),
    "reach_split": (0.589, 0.512, 0.494),
    "odd_objects": (0.584, 0.506, 0.486),
}
# regime: grazing rays of reach_rays that pass ABOVE the top of their sphere and still cross it in the restatement -- measured
MEASURED_GRAZING = {"tiny": 197, "far": 286, "huge_far": 303, "dense": 243, "dense2": 299, "groups": 259, "noground": 130,
                    "reach_split": 231}

_cache = {}


def _regime(tor, name):
    """Scene, layout for the time range (0, 1), rays and the restatements' answers: computed once per regime, never changed."""
    if name not in _cache:
        recs = Q.scene(name, SCENE_SEED)
        layout = tor.debug_accel_layout(tor.Scene.from_records(recs).list(), 0.0, 1.0)
        rays, tr = Q.rays(recs, N_RAYS, RAY_SEED)
        hit = H.world_hit(recs, rays, tr)
        cross = X.crossings(recs, rays, 17, tr)
        for a in (recs, rays, tr, hit):
            a.setflags(write=False)
        _cache[name] = dict(recs=recs, layout=layout, rays=rays, tr=tr, hit=hit, cross=cross)
    return _cache[name]


@pytest.mark.parametrize("name", Q.REGIMES)
def test_enough_rays_hit_cross_and_mix(tor, name):
    g = _regime(tor, name)
    rays, tr = g["rays"], g["tr"]
    obj = H.fields(g["hit"])["object"]
    ground = 0 if Q.has_ground(name) else -1
    nonground = float(((obj >= 0) & (obj != ground)).mean())
    total = g["cross"]["total"]
    over4, over16 = float((total > 4).mean()), float((total > 16).mean())
    want = MEASURED[name]
    print(f"{name}: non-ground hits {nonground:.3f}, more than 4 crossings {over4:.3f}, more than 16 {over16:.3f}")
    assert 0.2 <= nonground <= 0.9, nonground                                # neither all-miss nor all-hit
    assert nonground >= 0.5 * want[0] and over4 >= 0.5 * want[1] and over16 >= 0.5 * want[2], (nonground, over4, over16)
    # every 64 consecutive rays hold every kind, a finite and an infinite range end, and times inside and outside [0, 1]
    for w0 in range(0, N_RAYS, 64):
        w = slice(w0, w0 + 64)
        assert np.isinf(tr[w, 1]).any() and (tr[w, 1] == 1.0).any()
        assert ((rays[w, 6] < 0) | (rays[w, 6] > 1)).sum() == 8 and ((rays[w, 6] >= 0) & (rays[w, 6] <= 1)).sum() == 56
        norm = np.linalg.norm(rays[w, 3:6], axis=1)
        assert (np.abs(norm - 1) < 1e-12).sum() >= 16 and (np.abs(norm - 1) > 1e-3).sum() >= 32    # unit and unnormalised directions


def test_dense_duplicates_tie_among_the_first_17_crossings(tor):
    g = _regime(tor, "dense")
    recs = g["recs"]
    assert len(recs) == 724 and all((recs[700 + k] == recs[:700]).all(axis=1).any() for k in range(24))
    aimed = np.arange(N_RAYS) % 2 == 1
    t, count = g["cross"]["t"][aimed], g["cross"]["count"][aimed]
    tie = ((t[:, 1:] == t[:, :-1]) & (np.arange(1, 17)[None, :] < count[:, None])).any(axis=1)
    print(f"dense: {tie.mean():.3f} of the aimed rays have two equal t among their first 17 crossings")    # measured: 0.252
    assert tie.mean() >= 0.2


@pytest.mark.parametrize("name", Q.REGIMES)
def test_layout_facts(tor, name):
    g = _regime(tor, name)
    lay = g["layout"]
    assert lay is not None, "every regime has a culling layout"
    assert lay[3] == (name == "dense2"), "dense2 and only dense2 is two-level"
    in_slots = lay[0][lay[0] >= 0]
    assert in_slots.size >= 32 and np.unique(in_slots).size == in_slots.size
    if Q.has_ground(name):
        assert 0 not in in_slots                                              # the ground sphere is no block's object


def test_reach_is_none_for_needle_and_for_odd_objects(tor):
    for name in ("needle", "odd_objects"):
        g = _regime(tor, name)
        _, reach, _ = Q.reach_of(g["recs"], g["layout"])
        assert not (reach > 0) or not np.isfinite(reach), (name, reach)
    g = _regime(tor, "odd_objects")
    in_slots = g["layout"][0][g["layout"][0] >= 0]
    odd = {nm: 724 + k for k, nm in enumerate(Q.ODD_NAMES)}
    # which of the odd objects the layout sorts into blocks: the radius-0 sphere (no reach whatever else the scene holds) and the
    # finite but overflowing ones; the non-finite ones and the time0 == time1 mover are tested for every ray
    assert {nm for nm, j in odd.items() if j in in_slots} == {"radius 0", "centre 1e300", "mover displaced by 1e200"}


def test_reach_cuts_through_the_ray_origins_of_reach_split(tor):
    g = _regime(tor, "reach_split")
    org, reach, half_diag = Q.reach_of(g["recs"], g["layout"])
    assert 0 < reach < 2 * half_diag, (reach, half_diag)                      # measured: 20.05 against a half diagonal of 17.46
    rr, _, info = Q.reach_rays(g["recs"], g["layout"], REACH_SEED)
    inside = (((rr[:, 0:3] - org) ** 2).sum(axis=1) <= reach * reach).mean()
    print(f"reach_split: reach {reach:.4g}, half diagonal {half_diag:.4g}, {inside:.3f} of reach_rays' origins inside")   # 0.356
    assert 0.25 <= inside <= 0.75
    # both kinds of lane in every wave of them, and origins within 2e-9 of the reach on either side
    d2 = ((rr[:, 0:3] - org) ** 2).sum(axis=1)
    for w0 in range(0, len(rr), 64):
        assert (d2[w0:w0 + 64] <= reach * reach).any() and (d2[w0:w0 + 64] > reach * reach).any()
    near = np.abs(np.sqrt(d2) / reach - 1) < 2e-9
    assert (near & (d2 <= reach * reach)).sum() >= 64 and (near & (d2 > reach * reach)).sum() >= 64


@pytest.mark.parametrize("name", Q.BASE)
def test_reach_is_far_larger_than_the_scene(tor, name):
    g = _regime(tor, name)
    _, reach, half_diag = Q.reach_of(g["recs"], g["layout"])
    assert reach >= 10 * half_diag, (reach, half_diag)                        # measured: 15.4 x (huge_far) to 6500 x (tiny)


@pytest.mark.parametrize("name", sorted(MEASURED_GRAZING))
def test_grazing_rays_land_on_the_band_the_reference_rounds_in(tor, name):
    """Of the rays that pass strictly above a sphere's top, the restatement accepts some and rejects some: they sit on the rounding
    band, which is what a box without its margin, or a reach that is too large, gets wrong."""
    g = _regime(tor, name)
    rr, rtr, info = Q.reach_rays(g["recs"], g["layout"], REACH_SEED)
    above = (info["sphere"] >= 0) & (info["offset"] > 0)
    crosses = np.zeros(len(rr), dtype=bool)                                   # ... its own sphere, whatever else lies in front
    for j in np.unique(info["sphere"][above]):
        sel = np.flatnonzero(above & (info["sphere"] == j))
        crosses[sel] = np.isfinite(X.all_roots(g["recs"][j:j + 1], rr[sel], rtr[sel])).any(axis=1)
    print(f"{name}: {int(crosses.sum())} of {int(above.sum())} rays above a sphere's top cross it")
    assert crosses.sum() >= 0.5 * MEASURED_GRAZING[name] and (above & ~crosses).sum() >= 100
    factors = info["factor"][info["sphere"] < 0]
    assert set(np.unique(factors)) == set(Q.REACH_FACTORS)


def test_no_finite_block_bounds_over_an_overflowing_time_range(tor):
    """The second reason the block path falls back for: over the time range (0, 1e200) the centre of the mover displaced by 1e200
    overflows, and the host has no finite bounds -- for the same list that has a layout over (0, 1)."""
    g = _regime(tor, "odd_objects")
    world = tor.Scene.from_records(g["recs"]).list()
    assert g["layout"] is not None and tor.debug_accel_layout(world, 0.0, 1e200) is None
    assert tor.debug_accel_layout(tor.Scene.from_records(_regime(tor, "dense")["recs"]).list(), 0.0, 1e200) is not None


@pytest.mark.parametrize("name", Q.REGIMES)
def test_restatements_agree_with_each_other(tor, name):
    g = _regime(tor, name)
    recs, rays, tr, cross = g["recs"], g["rays"], g["tr"], g["cross"]
    f = H.fields(g["hit"])
    assert np.array_equal(cross["object"][:, 0], f["object"])                 # crossing 0 is world.hit's record
    assert np.array_equal(cross["t"][:, 0].view(np.uint64), f["t"].view(np.uint64))
    assert np.array_equal(cross["total"] > 0, f["object"] >= 0)               # ... and the any-hit bit
    first = {k: (v[:, :1] if v.ndim == 2 else np.minimum(v, 1)) for k, v in cross.items() if k in ("t", "object", "which", "count")}
    assert not H.mismatches(X.records(recs, rays, first)[:, 0], g["hit"])
    assert not H.mismatches(M.world_hit(recs, None, rays, Q.ALL, tr), g["hit"])
    assert np.array_equal(M.occluded(recs, None, rays, Q.ALL, tr), f["object"] >= 0)
    masked = X.masked_crossings(recs, None, rays, Q.ALL, 17, tr)
    assert not X.mismatches(masked, cross) and np.array_equal(masked["total"], cross["total"])
    # the sweep's group words and masks change enough answers to mean something, and differ inside every wave
    groups, masks = Q.group_words(len(recs)), Q.ray_masks(N_RAYS, RAY_SEED)
    changed, keeps, mixed = M.meaningful(recs, groups, rays, masks, tr)
    print(f"{name}: the masks change {changed:.3f} of the answers, {keeps:.3f} keep a hit")
    assert changed >= 0.2 and keeps >= 0.2 and mixed
    assert all(np.unique(masks[w0:w0 + 64]).size > 1 for w0 in range(0, N_RAYS, 64))
