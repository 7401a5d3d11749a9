"""Scene regimes and ray families for the query kernels' sweep (tests/test_query_regimes.py, tests/test_gpu_query_regimes.py).

The query tests before these ran on three scenes of one size at the world origin; the block path's exactness rests on quantities
that are derived from the SCENE (hit_reach's org / reach2 / a_min, the boxes' inflation, the layout's levels).  scene(name, seed)
builds one named regime -- tiny, far from the origin, huge, dense clusters with duplicates, two-level, every time group, no ground,
radii that leave no reach or one that cuts through the scene, non-finite and overflowing objects -- after the ideas of
tools/fuzz_accel.py's generator, with the regime fixed by name instead of drawn.  rays() mixes the ray kinds inside every wave;
reach_of() restates hit_reach's formula to PLACE rays on the reach and on the boxes' margin -- it never judges an answer.
numpy only."""
import numpy as np

import hit_restatement as H

TIME_GROUPS = [(0.0, 1.0), (-0.5, 0.5), (0.25, 2.0), (1.0, 0.0), (0.5, 0.5)]   # (the last: time0 == time1, never a finite fraction)
RADII = (0.15, 0.2, 0.3, 0.45, 1.0)
EPS = 2.0 ** -53

# name: objects, spread, distance of the scene from the world origin, and what else the regime fixes
_SPECS = {
    "tiny":     dict(n=200, spread=0.02, shift=0.0, movers=0.3),
    "far":      dict(n=200, spread=1.0, shift=1e5, movers=0.3),
    "huge_far": dict(n=485, spread=3000.0, shift=1e5, groups=2, movers=0.5, general="both"),
    "dense":    dict(n=700, spread=12.0, shift=10.0, clusters=2, tight=0.002, movers=0.3, duplicates=24),
    "dense2":   dict(n=1300, spread=4.0, shift=1e3, clusters=3, tight=0.1, movers=0.5),
    "groups":   dict(n=700, spread=12.0, shift=0.0, groups=5, movers=0.9, general="both", levels=3),
    "noground": dict(n=90, spread=60.0, shift=1e3, groups=3, movers=0.5, general="all", ground=False),
}
BASE = tuple(_SPECS)                                   # the seven regimes whose reach is far larger than the scene
DERIVED = ("needle", "reach_split", "odd_objects")     # `dense` with one object changed / a few appended
REGIMES = BASE + DERIVED
NEEDLE_RADIUS, SPLIT_RADIUS = 1e-9, 1e-5
ODD_NAMES = ("radius 0", "radius NaN", "centre +inf", "centre 1e300", "time0 == time1 mover", "mover displaced by 1e200")


def has_ground(name):
    """Record 0 is the ground sphere (radius 1000 rscale)."""
    return _SPECS.get(name, _SPECS["dense"]).get("ground", True)


def _generate(rng, n, spread, shift, groups=1, movers=0.0, general="none", ground=True, clusters=0, tight=0.0, levels=0, duplicates=0):
    rscale = spread / 12.0
    u = rng.normal(size=3)
    shift = shift * u / np.linalg.norm(u)
    tg = TIME_GROUPS[:groups]
    recs = []
    if ground:
        R = 1000.0 * rscale
        recs.append([0, shift[0], shift[1] - R, shift[2], shift[0], shift[1] - R, shift[2], 0, 1, R, 0, .5, .5, .5, 0, 0])
    heights = shift[1] + rng.uniform(0, 0.3 * spread, levels) if levels else None
    centres = shift + rng.uniform(-0.3, 0.3, (max(clusters, 1), 3)) * spread * (1, 0.3, 1) + (0, 0.1 * spread, 0)
    clustered = []
    while len(recs) < n:
        c = shift + np.array([rng.uniform(-spread, spread), rng.uniform(0, 0.3 * spread), rng.uniform(-spread, spread)])
        in_cluster = clusters > 0 and rng.random() < 0.9
        if in_cluster:
            c = centres[int(rng.integers(0, clusters))] + rng.uniform(-tight, tight, 3) * rscale
        if heights is not None and rng.random() < 0.9:
            c[1] = heights[int(rng.integers(0, levels))]
        r = float(rng.choice(RADII)) * rscale * (1 if rng.random() > 0.03 else -1)
        mat, alb = int(rng.integers(0, 3)), rng.uniform(0.1, 0.95, 3)
        fuzz, ri = rng.uniform(0, 0.6), rng.uniform(1.2, 1.8)
        if in_cluster:
            clustered.append(len(recs))
        if rng.random() >= movers:
            recs.append([0, *c, *c, 0, 1, r, mat, *alb, fuzz, ri])
            continue
        t0, t1 = tg[int(rng.integers(0, len(tg)))]
        g = general == "all" or (general == "both" and rng.random() < 0.5)
        d = rng.uniform(-0.6, 0.6, 3) * rscale if g else np.array([0.0, rng.uniform(0, 0.6) * rscale, 0.0])
        recs.append([1, *c, *(c + d), t0, t1, r, mat, *alb, fuzz, ri])
    recs = np.asarray(recs, dtype=np.float64)
    if duplicates:                                     # exact duplicates of cluster objects, behind the list: ties to the lower index
        recs = np.concatenate([recs, recs[rng.choice(clustered, duplicates, replace=False)]])
    return recs


def _small_static(recs):
    """The static spheres of ordinary size: what the culling layout sorts into blocks (|r| <= 2.5 median)."""
    r = np.abs(recs[:, 9])
    return np.flatnonzero((recs[:, 0] == 0) & (r > 0) & (r <= 2.5 * np.median(r)))


def odd_objects(recs):
    """One record per ODD_NAMES entry, modelled on a small static sphere of `recs`."""
    base = recs[_small_static(recs)[7]].copy()
    out = np.tile(base, (len(ODD_NAMES), 1))
    out[0, 9] = 0.0
    out[1, 9] = np.nan
    out[2, [1, 4]] = np.inf
    out[3, [1, 4]] = 1e300
    out[4, 0], out[4, 5], out[4, 7:9] = 1, base[2] + 0.1, (0.25, 0.25)
    out[5, 0], out[5, 4:7], out[5, 7:9] = 1, base[1:4] + (1e200, 0.0, -1e200), (0.0, 1.0)
    return out


def scene(name, seed=0):
    """(n, 16) float64 records of the named regime."""
    if name in _SPECS:
        spec = dict(_SPECS[name])
        return _generate(np.random.default_rng([seed, BASE.index(name)]), spec.pop("n"), spec.pop("spread"), spec.pop("shift"), **spec)
    recs = scene("dense", seed)
    if name in ("needle", "reach_split"):
        recs[_small_static(recs)[3], 9] = NEEDLE_RADIUS if name == "needle" else SPLIT_RADIUS
        return recs
    if name == "odd_objects":
        return np.concatenate([recs, odd_objects(recs)])
    raise KeyError(name)


def _placeable(recs):
    """The records a ray can be placed by: finite, and not astronomically far out."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(recs[:, 1:10]).all(axis=1) & (np.abs(recs[:, 1:7]) < 1e100).all(axis=1)
    return recs[ok]


def _box(recs):
    r = np.abs(recs[:, 9:10])
    lo = np.minimum(recs[:, 1:4], recs[:, 4:7]) - r
    hi = np.maximum(recs[:, 1:4], recs[:, 4:7]) + r
    return np.percentile(lo, 2, axis=0), np.percentile(hi, 98, axis=0)     # (the ground sphere's top is what matters)


def _aim(rng, recs, origins):
    """Unnormalised directions from `origins` to jittered centres of ordinary objects."""
    r = np.abs(recs[:, 9])
    pool = np.flatnonzero(r <= 10.0 * np.median(r))
    j = rng.choice(pool, len(origins))
    target = recs[j, 1:4] + rng.uniform(-0.8, 0.8, (len(origins), 3)) * r[j, None]
    return (target - origins) * rng.choice([0.01, 1.0, 37.5], (len(origins), 1))


def rays(recs, n, seed):
    """(rays (n, 7), t_range (n, 2)): ray i is of kind i % 4 -- 0 incoherent (hit_restatement.incoherent_rays), 1 and 3 aimed at a
    jittered object centre with an unnormalised direction (they cross a cluster many times), 2 a segment between two points of the
    scene's box with the range (0.001, 1) -- so every 64 consecutive rays hold every kind; ray i with i % 8 == 5 has a time outside
    [0, 1], the others one inside."""
    rng = np.random.default_rng([seed, 1])
    recs = _placeable(recs)
    lo, hi = _box(recs)
    out = H.incoherent_rays(recs, n, seed)
    tr = np.tile([0.001, np.inf], (n, 1))
    i = np.arange(n)
    aimed = np.flatnonzero(i % 2 == 1)
    out[aimed, 3:6] = _aim(rng, recs, out[aimed, 0:3])
    seg = np.flatnonzero(i % 4 == 2)
    out[seg, 3:6] = rng.uniform(lo, hi, (len(seg), 3)) - out[seg, 0:3]
    tr[seg, 1] = 1.0
    outside = np.flatnonzero(i % 8 == 5)
    out[outside, 6] = rng.choice([-3.0, -0.7, 1.6, 2.5], len(outside))
    return out, tr


ALL = 0xFFFFFFFF
MASK_VALUES = np.array([0, 1, 6, 0x15, ALL], dtype=np.uint32)


def group_words(n):
    """One visibility word per object: 1 << (j % 5), every 11th 0 (seen by no ray), every 13th 0xFFFFFFFF (seen by every mask but 0)."""
    j = np.arange(n)
    w = (np.uint32(1) << (j % 5).astype(np.uint32)).astype(np.uint32)
    w[::11] = 0
    w[::13] = ALL
    return w


def ray_masks(n, seed):
    """One of MASK_VALUES per ray, drawn; the tests assert that the values differ inside every 64 consecutive rays."""
    return np.random.default_rng([seed, 3]).choice(MASK_VALUES, n)


def _spatial(recs, layout):
    slots = np.asarray(layout[0]).reshape(-1)
    return slots[slots >= 0]


def _union(layout):
    boxes = np.asarray(layout[1], dtype=np.float64).reshape(-1, 6)
    boxes = boxes[~np.isnan(boxes[:, 0])]
    return boxes[:, 0:3].min(axis=0), boxes[:, 3:6].max(axis=0)


def reach_of(recs, layout):
    """(org (3,), reach, half diagonal) of DESIGN 4.8 restated on tor.debug_accel_layout's boxes and the radii of the objects in its
    slots: within `reach` of org, 16 eps (|oc|^2 + r_max^2) / r_min <= 1e-6 / 4.  reach is -inf where the margin covers no origin."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    lo, hi = _union(layout)
    r = np.abs(recs[_spatial(recs, layout), 9])
    org = 0.5 * lo + 0.5 * hi
    with np.errstate(all="ignore"):
        half_diag = 0.5 * np.sqrt(((hi - lo) ** 2).sum()) * (1.0 + 1e-9)
        oc2 = 0.25e-6 * r.min() / (16.0 * EPS) - r.max() ** 2
        reach = np.sqrt(oc2) * (1.0 - 1e-9) - half_diag if oc2 > 0 and np.isfinite(oc2) and r.min() > 0 else -np.inf
    return org, (float(reach) if np.isfinite(reach) else -np.inf), float(half_diag)


REACH_FACTORS = (0.5, 0.9, 1.0 - 1e-9, 1.0 + 1e-9, 1.1, 3.0)
SLACK_OFFSETS = (0.0, 0.05, 0.2, 0.5, 1.0, 2.0)        # times 6 eps (D^2 + r^2) / r: how far outside a sphere the reference accepts
MARGIN_OFFSETS = (0.5, 1.0, 2.0)                       # times 1e-6: the least a box is inflated by
PAD_MULTIPLES = (4.0, 64.0, 1024.0)                    # distances at which the slack is this many times the boxes' own inflation


def _pad(layout):
    """The largest inflation of a box of the layout (compute_block_bounds: 1e-6 (1 + |lo| + |hi| + (hi - lo)) per axis)."""
    lo, hi = _union(layout)
    return float(1e-6 * (1.0 + np.abs(lo) + np.abs(hi) + (hi - lo)).max())


def reach_rays(recs, layout, seed, per_factor=64, n_spheres=48):
    """Rays placed on the reach: (rays (n, 7), t_range (n, 2), info) with info = dict of per-ray arrays `factor` (the origin's
    distance from org in units of the reach; NaN for the grazing rays placed by the boxes' inflation), `sphere` (the object a grazing
    ray passes over, -1 for the first family) and `offset` (its height above that sphere's top).

    Family one: origins at REACH_FACTORS times the reach from org in random directions, aimed back at the scene's objects.
    Family two, in the style of hit_restatement.far_grazing_rays: horizontal rays over the top of small static spheres, from origins
    at those same distances from org and from the distances at which the reference's rounding slack 6 eps (D^2 + r^2) / r is
    PAD_MULTIPLES times the boxes' inflation (at most half the radius); the ray passes SLACK_OFFSETS times that slack, or MARGIN_OFFSETS times 1e-6, above the
    top.  Needs reach_of(recs, layout)[1] > 0."""
    rng = np.random.default_rng([seed, 2])
    full = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    org, reach, _ = reach_of(full, layout)
    assert reach > 0
    place = _placeable(full)
    out, factor, sphere, offset = [], [], [], []
    n_one = per_factor * len(REACH_FACTORS)            # ray i at REACH_FACTORS[i % 6]: every wave holds origins on both sides
    fs = np.tile(REACH_FACTORS, per_factor)
    u = rng.normal(size=(n_one, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = org + (fs * reach)[:, None] * u
    out.append(np.concatenate([o, _aim(rng, place, o), rng.uniform(0, 1, (n_one, 1))], axis=1))
    factor += list(fs)
    sphere += [-1] * n_one
    offset += [0.0] * n_one
    spatial = set(int(j) for j in _spatial(full, layout))
    small = [int(j) for j in _small_static(full) if int(j) in spatial and np.isfinite(full[j, 1:4]).all() and np.abs(full[j, 1:4]).max() < 1e100]
    # the spheres that carry the top face of their block's box come first: a hit beyond the box shows on them; then the smallest
    # radii (the largest slack), then any
    slots, boxes = np.asarray(layout[0]), np.asarray(layout[1], dtype=np.float64).reshape(-1, 6)
    top_of = {int(j): boxes[b, 4] for b in range(slots.shape[0]) for j in slots[b] if j >= 0}
    carries = [j for j in small if top_of[j] - (full[j, 2] + abs(full[j, 9])) <= 2e-6 * (1.0 + 4.0 * abs(top_of[j]))]
    rest = [j for j in sorted(small, key=lambda j: abs(full[j, 9])) if j not in carries]
    rng.shuffle(carries)
    small = (carries[:n_spheres - 4] + rest[:4] + list(rng.permutation(rest[4:])))[:n_spheres]
    pad = _pad(layout)
    graze = []
    for j in small:
        c, r = full[j, 1:4], abs(full[j, 9])
        top = c + np.array([0.0, r, 0.0])
        by_reach = [(f, None) for f in REACH_FACTORS]
        by_pad = [(np.nan, np.sqrt(min(k * pad, 0.5 * r) * r / (6.0 * EPS))) for k in PAD_MULTIPLES]
        dists = [by_reach[0], by_pad[0], by_reach[1], by_reach[3], by_reach[2], by_pad[1], by_reach[4], by_reach[5], by_pad[2]]   # (inside and outside the reach alternate)
        for f, dist in dists:
            a = rng.uniform(0, 2 * np.pi)
            u = np.array([np.cos(a), 0.0, np.sin(a)])
            if dist is None:                           # s > 0 with |top - s u - org| = f reach
                w = top - org
                b, cc = -(w @ u), w @ w - (f * reach) ** 2
                if b * b - cc < 0 or -b + np.sqrt(b * b - cc) <= 0:
                    continue
                dist = -b + np.sqrt(b * b - cc)
            slack = 6.0 * EPS * (dist * dist + r * r) / r
            for off in [k * slack for k in SLACK_OFFSETS] + [k * 1e-6 for k in MARGIN_OFFSETS]:
                p = top + np.array([0.0, off, 0.0])
                graze.append([*(p - dist * u), *u, 0.0])
                factor.append(f)
                sphere.append(j)
                offset.append(p[1] - top[1])
    out = np.concatenate(out + [np.asarray(graze, dtype=np.float64).reshape(-1, 7)])
    info = {"factor": np.asarray(factor), "sphere": np.asarray(sphere), "offset": np.asarray(offset)}
    return out, np.tile([0.001, np.inf], (len(out), 1)), info
