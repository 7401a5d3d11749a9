"""Nearest-surface point queries without a GPU: tor_nearest_device / tor_nearest_host are declared, exported and bound with matching
signatures, every argument check that needs no device answers TOR_ERR_INVALID_ARGUMENT with its reason, and the numpy restatement
the GPU tests compare against (tests/nearest_restatement.py) is itself held to hand-worked cases, to the order independence the
kernel's pruning rests on and to the sub-list reading of the masks.  Last, the inputs of tests/test_gpu_nearest_query.py
(tests/nearest_inputs.py) are shown to mean something, from the restatement alone.

Every floor of MEASURED is half of what the restatement gave here with the committed generator (point seed 11); the measured value
stands in the table."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import nearest_inputs as I
import nearest_restatement as N
import query_regimes as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tor_nearest_device", "tor_nearest_host")


def _err(tor):
    return tor.lib().tor_last_error().decode()


def _sphere(c, r):
    return [0, *c, *c, 0, 1, r, 0, .5, .5, .5, 0, 1.5]


def _mover(c0, c1, t0, t1, r):
    return [1, *c0, *c1, t0, t1, r, 0, .5, .5, .5, 0, 1.5]


def _pt(*rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 4)


def test_new_symbols_are_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in NEW:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
        assert name in tor.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
        decl = re.search(r"TOR_API\s+int\s+" + name + r"\s*\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(getattr(L, name).argtypes), name
    assert len(L.tor_nearest_device.argtypes) == 15 and len(L.tor_nearest_host.argtypes) == 14
    assert re.search(r"TOR_NEAREST_MAX\s*=\s*(\d+)", src).group(1) == str(tor.NEAREST_MAX)
    assert re.search(r"typedef struct TorPoint \{ TorVec3 p; double time; \} TorPoint;", src)
    assert re.search(r"typedef struct TorNear \{ double distance; int32_t object; int32_t inside; \} TorNear;", src)
    kw = list(inspect.signature(tor.Context.nearest).parameters)
    assert kw == ["self", "points", "k", "max_distance", "index", "time_range", "mode", "mask", "out"]
    assert inspect.signature(tor.Context.nearest).parameters["k"].default == 1
    assert hasattr(tor, "NearestResult")
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*tor_nearest\.hip", mk, re.M) and re.search(r"^ASM_SRCS = .*tor_nearest\.hip", mk, re.M)


def test_argument_checks_need_no_device(tor):
    L = tor.lib()
    b = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    big = (0x7fffffff * 256) + 1
    for name, extra in (("tor_nearest_device", (None,)), ("tor_nearest_host", ())):
        fn = getattr(L, name)

        def refused(word, ctx=b, n=4, points=b, lst=None, n_list=4, k=4, lo=0.0, hi=1.0, mode=0, near=b, count=b):
            rc = fn(ctx, n, points, None, lst, n_list, k, None, 0xFFFFFFFF, lo, hi, mode, near, count, *extra)
            msg = _err(tor)
            assert rc == tor.ERR_INVALID_ARGUMENT, (name, word, rc)
            assert msg.startswith(name + ":") and word in msg, (name, word, msg)

        refused("ctx is NULL", ctx=None)
        refused("< 0", n=-1, n_list=-1)
        refused("above 2^31 - 1 workgroups", n=big, n_list=big)
        for k in (0, -1, tor.NEAREST_MAX + 1, 1 << 20):
            refused("k must be in 1 .. TOR_NEAREST_MAX", k=k)
        for lo, hi in ((math.nan, 1.0), (0.0, math.nan), (-math.inf, 1.0), (0.0, math.inf), (1.0, 0.5)):
            refused("time range", lo=lo, hi=hi)
        for mode in (-1, 3, 7):
            refused("mode", mode=mode)
        refused("NULL points, near or count", points=None)
        refused("NULL points, near or count", near=None)
        refused("NULL points, near or count", count=None)
        # the list rules of tor_crossings_device
        refused("n_list < 0", lst=b, n_list=-1)
        refused("without a list n_list must be", lst=None, n_list=3)
        refused("n_list above", lst=b, n_list=big)
        refused("NULL points, near or count", lst=b, n_list=2, near=None)
        # the documented order: the count before k, k before the time range, the time range before the arrays
        refused("< 0", n=-1, n_list=-1, k=0, lo=math.nan, points=None)
        refused("k must be", k=0, lo=math.nan, points=None)
        refused("time range", lo=math.nan, mode=9, points=None)
        refused("mode", mode=9, points=None)


def test_context_nearest_rejects_bad_arguments_before_the_library(tor):
    ctx = object.__new__(tor.Context)  # a context whose creation never happened (no device here)
    ctx._h = C.c_void_p()
    for pts, k, dm in ((np.zeros((4, 3)), 2, None), (np.zeros((4, 7)), 2, None), (np.zeros(4), 2, None),
                       (np.zeros((4, 4)), 0, None), (np.zeros((4, 4)), tor.NEAREST_MAX + 1, None),
                       (np.zeros((4, 4)), 2, np.zeros(3)), (np.zeros((4, 4)), 2, np.zeros((4, 2)))):
        with pytest.raises(ValueError):
            ctx.nearest(pts, k, max_distance=dm)
    with pytest.raises(ValueError):
        ctx.nearest(np.zeros((4, 4)), 2, out=np.zeros((4, 2, 2)))
    with pytest.raises(KeyError):
        ctx.nearest(np.zeros((4, 4)), 2, mode="fastest")
    with pytest.raises(tor.TorError) as e:
        ctx.nearest(np.zeros((4, 4)))
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "tor_nearest_host" in str(e.value)  # the NULL context, refused by the library


def test_unit_sphere_and_negative_radius_by_hand():
    one = np.array([_sphere((0, 0, 0), 1.0)])
    pts = _pt([3, 0, 0, 0], [0, 4, 3, 0], [0, 0, 0, 0], [0.5, 0, 0, 0], [0, 0, -0.25, 0.7])
    got = N.nearest(one, pts, 2)
    assert got["distance"][:, 0].tolist() == [2.0, 4.0, -1.0, -0.5, -0.75]          # on the centre d = -r
    assert got["inside"][:, 0].tolist() == [0, 0, 1, 1, 1] and (got["object"][:, 0] == 0).all() and (got["count"] == 1).all()
    assert (got["object"][:, 1] == -1).all() and (got["distance"][:, 1] == 0).all() and (got["inside"][:, 1] == 0).all()
    # a negative radius is a surface at abs(radius): the hollow-glass idiom, inner shell -0.9 r inside the outer one
    ball = np.array([_sphere((0, 0, 0), 2.0), _sphere((0, 0, 0), -1.8)])
    got = N.nearest(ball, _pt([5, 0, 0, 0], [1.9, 0, 0, 0], [1, 0, 0, 0]), 2)
    assert got["object"].tolist() == [[0, 1], [0, 1], [0, 1]]
    assert got["distance"].tolist() == [[3.0, 5.0 - 1.8], [1.9 - 2.0, 1.9 - 1.8], [-1.0, 1.0 - 1.8]]
    assert got["inside"].tolist() == [[0, 0], [1, 0], [1, 1]]
    # radii whose square overflows or underflows: the distance uses abs(radius), never sqrt(radius * radius)
    odd = np.array([_sphere((0, 0, 0), 1e200), _sphere((0, 0, 0), -1e-200)])
    got = N.nearest(odd, _pt([3, 0, 0, 0]), 2)
    assert got["object"][0].tolist() == [0, 1] and got["distance"][0].tolist() == [3.0 - 1e200, 3.0 - 1e-200]


def test_ties_go_to_the_lower_index_at_entries_k_and_k_plus_1():
    two = np.array([_sphere((-2, 0, 0), 1.0), _sphere((2, 0, 0), 1.0)])
    p = _pt([0, 0, 0, 0])
    got = N.nearest(two, p, 2)
    assert got["distance"][0].tolist() == [1.0, 1.0] and got["object"][0].tolist() == [0, 1] and got["tied"][0]
    got = N.nearest(two, p, 1)
    assert got["object"][0].tolist() == [0] and got["count"][0] == 1 and got["total"][0] == 2 and got["tied"][0]
    assert N.nearest(two[::-1], p, 1)["object"][0].tolist() == [0]                  # ... whichever sphere stands first in the list
    # exact duplicates behind a nearer sphere: entries K and K + 1 share one distance at K = 2
    recs = np.array([_sphere((0, 3, 0), 1.0), _sphere((0, 0, 1), 0.5), _sphere((0, 3, 0), 1.0), _sphere((0, 3, 0), 1.0)])
    got = N.nearest(recs, p, 2)
    assert got["object"][0].tolist() == [1, 0] and got["distance"][0].tolist() == [0.5, 2.0] and got["tied"][0]
    got = N.nearest(recs, p, 4)
    assert got["object"][0].tolist() == [1, 0, 2, 3] and not N.nearest(recs, p, 1)["tied"][0]


def test_a_mover_at_three_times_and_objects_without_a_distance():
    mover = np.array([_mover((0, 0, 0), (0, 2, 0), 0.0, 1.0, 0.5)])
    got = N.nearest(mover, _pt([0, 0, 0, 0.0], [0, 0, 0, 0.5], [0, 0, 0, 1.0], [0, 0, 0, 2.0], [0, 0, 0, math.nan]), 1)
    assert got["distance"][:, 0].tolist() == [-0.5, 0.5, 1.5, 3.5, 0.0] and got["inside"][:, 0].tolist() == [1, 0, 0, 0, 0]
    assert got["count"].tolist() == [1, 1, 1, 1, 0]                                  # a NaN time gives a mover no distance
    # a time0 == time1 mover (the fraction is never finite), radius NaN, a centre at +inf: no neighbours, never an entry
    odd = np.array([_mover((0, 0, 0), (0, 1, 0), 0.25, 0.25, 0.5), _sphere((0, 0, 0), math.nan), _sphere((math.inf, 0, 0), 1.0)])
    pts = _pt([0, 0, 0, 0.25], [1, 2, 3, 0.0], [math.inf, 0, 0, 0.5])
    got = N.nearest(odd, pts, 3)
    assert (got["count"] == 0).all() and (got["object"] == -1).all() and (got["distance"] == 0).all() and (got["inside"] == 0).all()
    both = np.concatenate([odd, [_sphere((0, 0, 0), 1.0)]])
    got = N.nearest(both, pts[:2], 3)
    assert got["object"].tolist() == [[3, -1, -1], [3, -1, -1]] and got["count"].tolist() == [1, 1]


def test_d_max_is_strict_and_nan_accepts_nothing():
    recs = np.array([_sphere((0, 0, 0), 1.0), _sphere((4, 0, 0), 1.0), _sphere((0, 9, 0), 1.0)])
    p = _pt([0.5, 0, 0, 0])                                                          # distances -0.5, 2.5, about 8.01
    for d_max, want in ((0.0, [0]), (-0.25, [0]), (-0.5, []), (-1.0, []), (2.5, [0]), (np.nextafter(2.5, 3), [0, 1]),
                        (math.inf, [0, 1, 2]), (math.nan, []), (-math.inf, [])):
        got = N.nearest(recs, p, 3, d_max)
        assert got["object"][0][:got["count"][0]].tolist() == want and got["count"][0] == len(want), (d_max, got["object"])
    # one limit per point
    got = N.nearest(recs, np.repeat(p, 3, axis=0), 3, np.array([math.nan, 0.0, math.inf]))
    assert got["count"].tolist() == [0, 1, 3]


@pytest.fixture(scope="module")
def scene_points():
    recs = Q.scene("groups", 0)
    rng = np.random.default_rng(51)
    lo, hi = Q._box(recs)
    pts = np.concatenate([rng.uniform(lo, hi, (1024, 3)), rng.uniform(-0.5, 1.5, (1024, 1))], axis=1)
    d_max = rng.choice([np.inf, 0.5, 2.0], 1024)
    return recs, pts, d_max


def test_the_answer_does_not_depend_on_the_list_order(scene_points):
    """The neighbours are a set of keys, one per object; a permutation of the list renames the objects and nothing else.  Mapped
    back, every distance, object and inside flag is the same wherever no two of the first K + 1 share a distance."""
    recs, pts, d_max = scene_points
    rng = np.random.default_rng(52)
    want = N.nearest(recs, pts, 4, d_max)
    clear = ~want["tied"]
    assert clear.mean() > 0.99 and (want["total"] > 4).sum() > 40 and (want["total"] < 4).sum() > 40
    for _ in range(3):
        perm = rng.permutation(len(recs))
        got = N.nearest(recs[perm], pts, 4, d_max)
        back = np.where(got["object"] >= 0, perm[np.maximum(got["object"], 0)], -1)
        assert np.array_equal(got["count"], want["count"])
        assert np.array_equal(got["distance"][clear].view(np.uint64), want["distance"][clear].view(np.uint64))
        assert np.array_equal(back[clear], want["object"][clear]) and np.array_equal(got["inside"][clear], want["inside"][clear])


def test_masked_restatement_is_the_sub_list(scene_points):
    recs, pts, d_max = scene_points
    groups = Q.group_words(len(recs))
    masks = Q.ray_masks(len(pts), 53)
    got = N.masked_nearest(recs, groups, pts, masks, 4, d_max)
    assert (got["count"][masks == 0] == 0).all()
    full = N.nearest(recs, pts, 4, d_max)
    assert not N.mismatches(N.masked_nearest(recs, None, pts, N.ALL, 4, d_max), full)
    assert (got["total"] != full["total"]).mean() > 0.2
    sel = masks == 6
    seen = np.nonzero((groups & 6) != 0)[0]
    sub = N.nearest(recs[seen], pts[sel], 4, d_max[sel])
    assert sel.sum() > 100 and (sub["count"] > 0).sum() > 50
    assert np.array_equal(np.where(sub["object"] >= 0, seen[np.maximum(sub["object"], 0)], -1), got["object"][sel])
    assert np.array_equal(sub["distance"].view(np.uint64), got["distance"][sel].view(np.uint64))
    assert N.mismatches(got, full)                                                   # (and mismatches() does see a difference)


# scene: share of the points with a neighbour under the scene's d_max (K = 1 is full), with 4 neighbours under the per-point limits,
# inside at least one sphere, with an exact tie among the first 5 and among the first 17 without a limit, beyond the point reach
MEASURED = {
    "random":      (0.500, 0.217, 0.318, 0.000, 0.000, 0.062),
    "anim":        (0.499, 0.186, 0.313, 0.000, 0.000, 0.062),
    "dense":       (0.500, 0.438, 0.528, 0.042, 0.235, 0.062),
    "dense2":      (0.500, 0.470, 0.532, 0.000, 0.000, 0.062),
    "groups":      (0.497, 0.203, 0.386, 0.000, 0.000, 0.062),
    "far":         (0.500, 0.132, 0.412, 0.000, 0.000, 0.062),
    "reach_split": (0.500, 0.438, 0.528, 0.042, 0.235, 0.062),
    "odd_objects": (0.500, 0.441, 0.530, 0.043, 0.226, 1.000),
}


@pytest.mark.parametrize("name", I.SCENES)
def test_the_gpu_files_inputs_mean_something(tor, name):
    recs = I.scene(tor, name)
    lay = I.layout(tor, recs)
    assert len(recs) == {"random": 485, "anim": 1601, "dense": 724, "dense2": 1300, "groups": 700, "far": 200, "reach_split": 724,
                         "odd_objects": 730}[name]
    assert lay is not None and bool(lay[3]) == (name in ("anim", "dense2"))          # the two-level scenes
    pts = I.points(recs, lay)
    n = len(pts)
    assert n == I.N_POINTS and n % 64 != 0
    org, reach = I.point_reach_of(recs, lay)
    far = ((pts[:, 0:3] - org) ** 2).sum(axis=1) > reach * reach if reach > 0 else np.ones(n, dtype=bool)
    open16 = N.nearest(recs, pts, 16)
    d_scene = I.scene_d_max(open16)
    under = N.nearest(recs, pts, 1, d_scene)
    per_point = N.nearest(recs, pts, 4, I.point_d_max(n, d_scene))
    with np.errstate(invalid="ignore"):
        inside = (N.distances(recs, pts) < 0).any(axis=1)
    got = (float((under["total"] >= 1).mean()), float((per_point["total"] >= 4).mean()), float(inside.mean()),
           float(N.nearest(recs, pts, 4)["tied"].mean()), float(open16["tied"].mean()), float(far.mean()))
    print(f"{name}: neighbour under d_max = {d_scene:.4g}: {got[0]:.3f}, 4 under the per-point limits {got[1]:.3f}, inside a sphere "
          f"{got[2]:.3f}, tie among 5 {got[3]:.3f}, among 17 {got[4]:.3f}, beyond the reach {got[5]:.3f} (reach {reach:.4g})")
    assert all(g >= 0.5 * w for g, w in zip(got, MEASURED[name])), (got, MEASURED[name])
    assert 0.3 <= got[0] <= 0.7, "the scene's d_max leaves about half of the points without a neighbour"
    assert (name == "odd_objects") == (not reach > 0)                                # only odd_objects has no point reach
    if reach > 0:                                                                    # points on either side of the reach, 2e-9 from it
        r = np.sqrt(((pts[:, 0:3] - org) ** 2).sum(axis=1)) / reach
        assert ((np.abs(r - 1) < 2e-9) & ~far).sum() >= 32 and ((np.abs(r - 1) < 2e-9) & far).sum() >= 32
        assert (np.abs(r - 3) < 1e-6).sum() >= 32 and (np.abs(r - 0.5) < 1e-6).sum() >= 32
    # every wave holds times inside and outside the range and NaN, points inside a sphere and points with short lists
    t = pts[:, 3]
    for w0 in range(0, n - 63, 64):
        w = slice(w0, w0 + 64)
        assert np.isnan(t[w]).sum() == 4 and ((t[w] < 0) | (t[w] > 1)).sum() == 4 and ((t[w] >= 0) & (t[w] <= 1)).sum() == 56
        assert inside[w].any() and (~inside[w]).any() and far[w].any()
        assert (under["total"][w] == 0).any() and (under["total"][w] > 0).any()
    # the shells: points 2^-52 |r| inside and outside a surface do land on either side of it
    d0 = open16["distance"]
    assert ((d0 < 0) & (d0 > -1e-12)).any() and ((d0 > 0) & (d0 < 1e-12)).any() or name == "far"
