"""Scenes and points for the nearest-surface query's tests (tests/test_nearest_query.py shows on the CPU that they mean something,
tests/test_gpu_nearest_query.py compares the kernels with the restatement on them).

points() mixes the point kinds inside every wave of 64: uniform points in and around the scene's box, object centres exactly, points
a hair inside and outside a surface, points on either side of the point reach and far beyond it; times inside and outside (0, 1) and
NaN.  point_reach_of() restates the library's point reach on tor.debug_accel_layout's boxes to PLACE points on it -- it
never judges an answer.  numpy only."""
import numpy as np

import nearest_restatement as N
import query_regimes as Q

SCENES = ("random", "anim", "dense", "dense2", "groups", "far", "reach_split", "odd_objects")
N_POINTS = 2048 + 37                                   # a ragged tail: the last wave is partly empty
POINT_SEED = 11
TIME_RANGE = (0.0, 1.0)
EPS = 2.0 ** -53
REACH_FACTORS = (0.5, 1.0 - 1e-9, 1.0 + 1e-9, 3.0)
SHELLS = tuple(s * 2.0 ** -k for k in (52, 40, 20, 3) for s in (-1.0, 1.0))   # centre + u |r| (1 + shell)

_scenes = {}


def scene(tor, name):
    """(n, 16) float64 records: random_scene(0xFACADE) (485 objects, one level), animation frame 6 at 108 x 192 (1601 objects, two
    levels), or a regime of tests/query_regimes.py."""
    if name not in _scenes:
        if name == "random":
            recs = tor.random_scene(0xFACADE).to_records()
        elif name == "anim":
            recs = next(iter(tor.Animation(108, 192).scenes(skip=6)))[1].to_records()
        else:
            recs = Q.scene(name, 0)
        recs = np.array(recs, dtype=np.float64).reshape(-1, 16)
        recs.setflags(write=False)
        _scenes[name] = recs
    return _scenes[name]


def layout(tor, recs):
    return tor.debug_accel_layout(tor.Scene.from_records(np.asarray(recs)).list(), *TIME_RANGE)


def point_reach_of(recs, lay, time_range=TIME_RANGE):
    """(org (3,), reach) of DESIGN 4.16 restated: org is the centre of the boxes' union (as for the rays), and within `reach` of it
    32 eps (M + reach) <= 1e-6 / 4 with M the largest |c0| + |f| |c1 - c0| + |r| over the objects in the layout's slots, f the
    centre's fraction at either end of the time range.  reach is -inf without a layout."""
    if lay is None:
        return np.zeros(3), -np.inf
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    slots = np.asarray(lay[0]).reshape(-1)
    sp = recs[slots[slots >= 0]]
    boxes = np.asarray(lay[1], dtype=np.float64).reshape(-1, 6)
    boxes = boxes[~np.isnan(boxes[:, 0])]
    org = 0.5 * boxes[:, 0:3].min(axis=0) + 0.5 * boxes[:, 3:6].max(axis=0)
    with np.errstate(all="ignore"):
        moving = sp[:, 0] != 0
        dt = sp[:, 8] - sp[:, 7]
        f = np.where(moving, np.maximum(np.abs((time_range[0] - sp[:, 7]) / dt), np.abs((time_range[1] - sp[:, 7]) / dt)), 0.0)
        m = np.linalg.norm(sp[:, 1:4], axis=1) + np.where(moving, f * np.linalg.norm(sp[:, 4:7] - sp[:, 1:4], axis=1), 0.0) + np.abs(sp[:, 9])
    if not np.isfinite(m).all():
        return org, -np.inf
    big = m.max() * (1.0 + 1e-5) + 1e-5
    reach = 0.25e-6 / (32.0 * EPS) * (1.0 - 1e-9) - big
    return org, (float(reach) if reach > 0 else -np.inf)


def points(recs, lay, seed=POINT_SEED, n=N_POINTS):
    """(n, 4) float64 {x, y, z, time}.  Point i is of kind i % 8: 0, 1 uniform in 1.5 x the scene's box; 2 an object's centre at the
    point's time, exactly; 3, 4, 5 that centre + a unit direction x |r| (1 + SHELLS[..]): a hair, and an eighth of the radius, inside
    and outside the surface; 6 at REACH_FACTORS x the point reach from the boxes' centre (without a reach: 1e6 .. 1e8 scene sizes
    away, and high above the scene); 7 uniform in the scene's box.  Point i with i % 16 == 5 has a time outside [0, 1], with
    i % 16 == 11 a NaN time; the others one inside."""
    rng = np.random.default_rng([seed, 5])
    full = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    place = Q._placeable(full)
    lo, hi = Q._box(place)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    i = np.arange(n)
    kind = i % 8
    time = rng.uniform(0.0, 1.0, n)
    time[i % 16 == 5] = rng.choice([-3.0, -0.7, 1.6, 2.5], int((i % 16 == 5).sum()))
    time[i % 16 == 11] = np.nan
    p = mid + rng.uniform(-1.5, 1.5, (n, 3)) * half
    inner = kind == 7
    p[inner] = mid + rng.uniform(-1.0, 1.0, (int(inner.sum()), 3)) * half
    # by an object: its centre at the point's time (time NaN: at time 0.5), the restatement's own expression
    r = np.abs(place[:, 9])
    pool = np.flatnonzero(r <= 10.0 * np.median(r))
    by = np.flatnonzero((kind >= 2) & (kind <= 5))
    j = rng.choice(pool, by.size)
    t_at = np.where(np.isnan(time[by]), 0.5, time[by])
    with np.errstate(all="ignore"):
        c = np.stack([np.array([N._centre(place[jj], tt)[a] for jj, tt in zip(j, t_at)]) for a in range(3)], axis=1)
    u = rng.normal(size=(by.size, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    shell = np.asarray(SHELLS)[(np.arange(by.size) // 3) % len(SHELLS)]
    off = np.where((kind[by] == 2)[:, None], 0.0, u * (r[j] * (1.0 + shell))[:, None])
    ok = np.isfinite(c).all(axis=1)
    p[by[ok]] = (c + off)[ok]
    # on and beyond the reach
    org, reach = point_reach_of(full, lay)
    out = np.flatnonzero(kind == 6)
    u = rng.normal(size=(out.size, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    if reach > 0:
        fs = np.asarray(REACH_FACTORS)[np.arange(out.size) % len(REACH_FACTORS)]
        p[out] = org + (fs * reach)[:, None] * u
    else:
        p[out] = mid + (10.0 ** rng.uniform(6, 8, out.size) * np.linalg.norm(half))[:, None] * u
    high = out[1::8]
    p[high] = mid + np.array([0.0, 1.0, 0.0]) * (np.linalg.norm(half) * 10.0 ** rng.uniform(1, 3, (high.size, 1)))
    pts = np.concatenate([p, time[:, None]], axis=1)
    pts.setflags(write=False)
    return pts


def scene_d_max(want_open):
    """One d_max for a scene, near the median nearest distance: the median of neighbour 0's distance in the restatement's answer
    without a limit, over the points that have a neighbour."""
    d = want_open["distance"][:, 0][want_open["count"] > 0]
    return float(np.median(d))


def point_d_max(n, d_scene, seed=POINT_SEED):
    """One d_max per point: 0, negative, +inf, NaN and multiples of the scene's value, drawn."""
    rng = np.random.default_rng([seed, 6])
    return rng.choice(np.array([0.0, -0.05 * abs(d_scene), -abs(d_scene), np.inf, np.nan, d_scene, 3.0 * abs(d_scene), 30.0 * abs(d_scene)]), n)
