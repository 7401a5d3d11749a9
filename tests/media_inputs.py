"""Named inputs of the participating-media queries (include/tor_media.h), the smallest at which a kernel can go wrong: tables of 1,
2 overlapping, 3 nested (sigma 0.1 / 0.2 / 0.3: (0.1 + 0.2) + 0.3 != (0.3 + 0.2) + 0.1, a reversed sum shows), 64 media (bit 63,
several active at once, lanes of one wave with very different step counts), coincident boundaries, a medium of sigma 0, a moving boundary with per-ray times, a negative
radius; origins inside, on (s0 == t_min to the bit) and tangent to a boundary; t_max inside a medium and equal to a root; tau of
0, +inf, NaN, negative and equal to a step exactly; a zero direction, non-finite rays, t_min >= t_max; one ray, found by search,
whose collision parameter rounds above t_next (the clamp); lists of 1, 63, 64, 65 and 257 entries.  Every case is a dict of recs
(n_objects, 16), objects, sigma, albedo (or None), rays (n, 7), tau (n,), t_range ((n, 2) or None).  assert_coverage() shows on
the restatement alone that each case does what its name says."""
import numpy as np

import media_restatement as R

INF, NAN = np.inf, np.nan


def _sphere(c, r, mat=0):
    return [0, c[0], c[1], c[2], c[0], c[1], c[2], 0.0, 1.0, r, mat, 0.5, 0.5, 0.5, 0.0, 1.5]


def _mover(c0, c1, t0, t1, r):
    return [1, c0[0], c0[1], c0[2], c1[0], c1[1], c1[2], t0, t1, r, 0, 0.5, 0.5, 0.5, 0.0, 1.5]


def _rays(seed, n, centre=(0.0, 0.0, 0.0), reach=5.0, spread=1.5, inside=0.25):
    """n seeded rays: origins within `reach` of centre (a share `inside` of them within `spread`), aimed at points within `spread`
    of it, direction lengths in [0.3, 3], times in [0, 1]."""
    g = np.random.default_rng(seed)
    c = np.asarray(centre, dtype=np.float64)
    o = c + g.normal(size=(n, 3)) * np.where(g.random(n) < inside, spread * 0.4, reach * 0.6)[:, None]
    aim = c + g.normal(size=(n, 3)) * spread * 0.5
    d = aim - o
    d = d / np.sqrt((d * d).sum(axis=1))[:, None] * g.uniform(0.3, 3.0, n)[:, None]
    return np.concatenate([o, d, g.random((n, 1))], axis=1)


def _taus(seed, n):
    g = np.random.default_rng(seed)
    tau = -np.log1p(-g.random(n)) * g.choice([0.3, 1.0, 3.0], size=n)
    tau[g.random(n) < 0.2] = INF
    return tau


def _case(name, recs, objects, sigma, albedo, rays, tau=None, t_range=None, seed=1):
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = len(rays)
    return dict(name=name, recs=np.asarray(recs, dtype=np.float64), objects=np.asarray(objects, dtype=np.int32),
                sigma=np.asarray(sigma, dtype=np.float64), albedo=None if albedo is None else np.asarray(albedo, dtype=np.float64),
                rays=rays, tau=_taus(seed, n) if tau is None else np.asarray(tau, dtype=np.float64),
                t_range=None if t_range is None else np.ascontiguousarray(t_range, dtype=np.float64))


def _row_of_64():
    """Three surface spheres, then 64 boundary spheres along x, each overlapping its neighbours; the table lists them in reverse
    object order, so medium m is object 66 - m and bit 63 is the sphere at x = 0."""
    recs = [_sphere((0, -1000, 0), 1000), _sphere((0, 3, 0), 0.5, 1), _sphere((5, 3, 0), 0.5, 2)]
    recs += [_sphere((0.5 * k, 0, 0), 0.6) for k in range(64)]
    objects = [66 - m for m in range(64)]
    sigma = [0.05 + 0.01 * (m % 7) for m in range(64)]
    albedo = [[0.1 + 0.01 * m, 0.9 - 0.01 * m, 0.5] for m in range(64)]
    g = np.random.default_rng(64)
    n = 257
    rays = _rays(64, n, centre=(15.75, 0, 0), reach=30.0, spread=8.0)
    along = np.arange(0, n, 3)                                  # every third ray runs along the row: up to 129 steps
    rays[along, 0:3] = np.stack([g.uniform(-3, 34, along.size), g.normal(size=along.size) * 0.1, g.normal(size=along.size) * 0.1], axis=1)
    rays[along, 3:6] = np.stack([g.choice([-1.0, 1.0], along.size) * g.uniform(0.5, 2, along.size),
                                 g.normal(size=along.size) * 0.01, g.normal(size=along.size) * 0.01], axis=1)
    rays[1:40:4, 0:3] = g.normal(size=(10, 3)) * 0.1            # origins inside the sphere at x = 0: bit 63 active at t_min
    tau = _taus(65, n)
    tau[along[::2]] = INF
    return _case("row64", recs, objects, sigma, albedo, rays, tau)


def _edges():
    """One unit ball of sigma 0.5 at the origin, hand-built rays; the named rows are in EDGE_ROWS."""
    recs = [_sphere((0, 0, 0), 1.0)]
    base = np.array([-6.0, 0, 0, 3.0, 0, 0, 0.25])
    has, s0, s1 = R.roots(recs, [0], [base])
    a0, a1 = s0[0, 0], s1[0, 0]
    full = R.march(recs, [0], [0.5], [base], INF)["depth"][0]   # the one step's sigma * length
    rows, tau, tr = [], [], []

    def add(name, ray, t, rng=(0.0, INF)):
        EDGE_ROWS[name] = len(rows)
        rows.append(ray)
        tau.append(t)
        tr.append(rng)
    EDGE_ROWS.clear()
    add("central", base, INF)
    add("tau_zero_outside", base, 0.0)                          # rho = 0 until s0: collides AT s0 (rem = 0 < step)
    add("tau_inf", base, INF)
    add("tau_nan", base, NAN)
    add("tau_negative", base, -1.0)
    add("tau_negative_zero", base, -0.0)
    add("tau_equals_step", base, full)                          # rem == step: strict <, no collision
    add("tau_just_below_step", base, np.nextafter(full, 0.0))
    add("origin_inside", [0.2, 0.1, -0.3, 1.0, 2.0, 0.5, 0.0], 0.4)
    add("tau_zero_inside", [0.2, 0.1, -0.3, 1.0, 2.0, 0.5, 0.0], 0.0)
    add("on_boundary", base, INF, (a0, INF))                    # s0 == t_min to the bit: active from the first step
    add("on_far_boundary", base, INF, (a1, INF))                # t == s1: not active (t < s1 strict)
    add("tangent", [-6.0, 1.0, 0, 3.0, 0, 0, 0.0], INF)         # disc == 0: no medium
    add("miss", [-6.0, 1.5, 0, 3.0, 0, 0, 0.0], 1.0)
    add("t_max_inside", base, INF, (0.0, 2.0))
    add("t_max_at_s0", base, 0.0, (0.0, a0))
    add("t_max_at_s1", base, INF, (0.0, a1))
    add("t_max_inf_inside", [0.0, 0, 0, 1.0, 0, 0, 0.0], INF, (0.0, INF))   # the far root ends it, not t_max
    add("behind", [6.0, 0, 0, 3.0, 0, 0, 0.0], 1.0)             # both roots negative
    add("zero_direction", [0.2, 0, 0, 0.0, 0, 0, 0.0], 1.0)
    add("zero_direction_outside", [3.0, 0, 0, 0.0, 0, 0, 0.0], INF)
    add("nan_origin", [NAN, 0, 0, 3.0, 0, 0, 0.0], 1.0)
    add("nan_direction", [-6.0, 0, 0, 3.0, NAN, 0, 0.0], 1.0)
    add("inf_direction", [-6.0, 0, 0, INF, 0, 0, 0.0], 1.0)
    add("inf_origin", [-INF, 0, 0, 3.0, 0, 0, 0.0], INF)
    add("huge_direction", [-6.0, 0, 0, 1e200, 0, 0, 0.0], 1.0)
    add("tiny_direction", [-6.0, 0, 0, 1e-170, 0, 0, 0.0], 1.0)
    add("nan_time", [-6.0, 0, 0, 3.0, 0, 0, NAN], 1.0)
    add("range_empty", base, 1.0, (2.0, 2.0))
    add("range_reversed", base, 1.0, (3.0, 1.0))
    add("range_nan", base, 1.0, (NAN, 3.0))
    add("range_negative", base, INF, (-INF, INF))
    add("t_min_inf", base, 1.0, (INF, INF))
    return _case("edges", recs, [0], [0.5], [[0.25, 0.5, 1.0]], rows, tau, tr)


EDGE_ROWS = {}

# t + (rem / rho) / len rounds above t_next: the first of the 12049 rows search_clamp(2 * 10 ** 6, 5) reports (about 0.6 % of its
# candidates, so the clamp is no corner: it decides one collision in 170 that falls within an ulp of a boundary); the unit ball at
# the origin with this sigma, the origin inside it, t_min = 0, tau the largest float64 below the step.  Set below, after the search.
CLAMP = None


def search_clamp(n, seed):
    """Rays from inside the unit ball (one medium, t_min = 0, so t = 0 and t_next = s1 at the only step) with tau the largest
    float64 below the step: the rows (ray, sigma, tau) whose unclamped collision parameter lies above t_next."""
    g = np.random.default_rng(seed)
    found = []
    for lo in range(0, n, 1 << 18):
        k = min(1 << 18, n - lo)
        o = g.normal(size=(k, 3)) * 0.3
        d = g.normal(size=(k, 3)) * g.uniform(0.1, 4.0, k)[:, None]
        sg = g.uniform(0.05, 5.0, k)
        rays = np.concatenate([o, d, np.zeros((k, 1))], axis=1)
        has, s0, s1 = R.roots([_sphere((0, 0, 0), 1.0)], [0], rays)
        with np.errstate(all="ignore"):
            ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
            step = sg * ((s1[:, 0] - 0.0) * ln)
            tau = np.nextafter(step, 0.0)
            t_c = 0.0 + (tau / sg) / ln
            hit = has[:, 0] & (s0[:, 0] <= 0.0) & (0.0 < s1[:, 0]) & (t_c > s1[:, 0])
        for i in np.nonzero(hit)[0]:
            found.append((rays[i].copy(), float(sg[i]), float(tau[i])))
    return found


def _clamp():
    ray, sg, tau = CLAMP
    return _case("clamp", [_sphere((0, 0, 0), 1.0)], [0], [sg], None, [ray], [tau])


def _build():
    cases = []
    cases.append(_case("one", [_sphere((0, 0, 0), 1.0)], [0], [0.5], None, _rays(1, 65), seed=2))
    cases.append(_case("two_overlap", [_sphere((0, 0, 0), 1.0), _sphere((0, 9, 9), 0.5, 1), _sphere((0.8, 0, 0), 1.0)], [2, 0],
                       [0.7, 1.3], [[0.9, 0.1, 0.5], [0.2, 0.8, 1.0]], _rays(3, 63, centre=(0.4, 0, 0)), seed=4))
    cases.append(_case("nested3", [_sphere((0, 0, 0), 3.0), _sphere((0, 0, 0), 2.0), _sphere((0, 0, 0), 1.0)], [0, 1, 2],
                       [0.1, 0.2, 0.3], [[1.0, 0.5, 0.25], [0.3, 0.6, 0.9], [0.7, 0.7, 0.1]], _rays(5, 64, reach=7.0, spread=1.0), seed=6))
    cases.append(_row_of_64())
    cases.append(_case("coincident", [_sphere((0, 0, 0), 1.0), _sphere((0, 0, 0), 1.0), _sphere((0.5, 0.5, 0), 1.0)], [0, 1, 2],
                       [0.4, 0.6, 0.2], None, _rays(7, 64), seed=8))
    cases.append(_case("sigma0", [_sphere((0, 0, 0), 1.5), _sphere((0.5, 0, 0), 1.0)], [0, 1], [0.0, 1.0], [[0.5, 0.5, 0.5], [0.0, 1.0, 0.0]],
                       _rays(9, 64), seed=10))
    cases.append(_case("moving", [_mover((-1, 0, 0), (1, 0.5, 0), 0.0, 1.0, 1.0), _sphere((0, 0, 0), 0.7)], [0, 1], [0.8, 0.3], None,
                       _rays(11, 65, spread=2.0), seed=12))
    cases.append(_case("negative_radius", [_sphere((0, 0, 0), -1.5), _sphere((1, 0, 0), 1.0)], [0, 1], [0.5, 0.25], None,
                       _rays(13, 63), seed=14))
    cases.append(_edges())
    if CLAMP is not None:
        cases.append(_clamp())
    return cases


CLAMP = (np.array([float.fromhex(h) for h in ("-0x1.a137385803e60p-4", "-0x1.aebb45b8f778bp-4", "-0x1.94d3fede3a144p-4",
                                               "-0x1.1446eddd1ae03p+1", "0x1.165db15ad69c0p+2", "0x1.5c25b88fc867cp+0", "0x0.0p+0")]),
         float.fromhex("0x1.9d02806fa9281p+1"), float.fromhex("0x1.b61eb04794078p+1"))
CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]

# lists over row64's 257 rays: lengths 1, 63, 64, 65 and 257 (the last with two entries outside [0, n), which are skipped)
def lists():
    g = np.random.default_rng(99)
    perm = g.permutation(257)
    out = {k: perm[:k].astype(np.int32) for k in (1, 63, 64, 65)}
    out[257] = np.concatenate([perm[:100], [-1], perm[100:255], [260]]).astype(np.int32)
    return out


def answer(c, index=None, into=None, steps=None, variant=None):
    return R.march(c["recs"], c["objects"], c["sigma"], c["rays"], c["tau"], c["t_range"], index, into, steps, variant)


def physics_rays(n=4096, seed=31, b_max=0.0):
    """The physics checks' rays against the unit ball at the origin: n rays with impact parameter b <= b_max (0: central rays),
    origins 5 .. 8 from the centre, direction lengths in [0.5, 3].  Returns (rays (n, 7), b (n,))."""
    g = np.random.default_rng(seed)
    u = g.normal(size=(n, 3))
    u = u / np.sqrt((u * u).sum(axis=1))[:, None]
    w = np.cross(u, g.normal(size=(n, 3)))
    w = w / np.sqrt((w * w).sum(axis=1))[:, None]
    b = g.random(n) * b_max
    o = w * b[:, None] - u * g.uniform(5.0, 8.0, n)[:, None]
    return np.concatenate([o, u * g.uniform(0.5, 3.0, n)[:, None], np.zeros((n, 1))], axis=1), b


PHYSICS_RECS = np.asarray([_sphere((0, 0, 0), 1.0)], dtype=np.float64)
PHYSICS_P = 1.0 - np.exp(-1.0)                                   # a central chord of 2 at sigma 0.5: depth 1
PHYSICS_TOL = 5.0 * np.sqrt(PHYSICS_P * (1.0 - PHYSICS_P) / 4096)  # 5 binomial standard errors at 4096 rays: 0.0377


def states(n, seed=2024):
    """n seeded xoshiro256+ states (any nonzero words are a state)."""
    return np.random.default_rng(seed).integers(1, 2 ** 64, size=(n, 4), dtype=np.uint64)   # all 64 bits: s0 + s3 must be uniform


def assert_coverage():
    """Each case does what its name says, on the restatement alone; returns the measured counts (the floors below are half of
    what was measured when the cases were made)."""
    got = {}
    for c in CASES:
        n = len(c["rays"])
        steps = np.zeros(n, dtype=np.int64)
        a = answer(c, steps=steps)
        act = a["active"]
        pop = np.array([bin(int(v)).count("1") for v in act])
        got[c["name"]] = dict(n=n, collided=int((a["status"] == 1).sum()), escaped=int((a["status"] == 0).sum()),
                              refused=int((a["status"] == -1).sum()), multi=int((pop > 1).sum()), max_steps=int(steps.max()),
                              depth_pos=int(((a["status"] == 0) & (a["depth"] > 0)).sum()))
    assert sorted(got[k]["n"] for k in ("one", "two_overlap", "nested3", "row64")) == [63, 64, 65, 257]
    for name, (col, esc) in FLOORS.items():
        assert got[name]["collided"] >= col and got[name]["depth_pos"] >= esc, (name, got[name])
    assert got["two_overlap"]["multi"] >= 5 and got["nested3"]["multi"] >= 10 and got["coincident"]["multi"] >= 10
    # 64 media: bit 63, several at once, and lanes of one wave with very different step counts
    c = BY_NAME["row64"]
    steps = np.zeros(257, dtype=np.int64)
    a = answer(c, steps=steps)
    assert int(((a["active"] >> np.uint64(63)) & np.uint64(1)).sum()) >= 3 and got["row64"]["multi"] >= 17
    first_wave = steps[:64]
    assert first_wave.max() >= 40 and first_wave.min() <= 2 and steps.max() >= 100, (first_wave.max(), first_wave.min(), steps.max())
    # coincident boundaries: equal s0 for two media on every ray that meets them
    has, s0, s1 = R.roots(BY_NAME["coincident"]["recs"], [0, 1, 2], BY_NAME["coincident"]["rays"])
    assert (has[:, 0] == has[:, 1]).all() and (s0[has[:, 0], 0] == s0[has[:, 0], 1]).all() and has[:, 0].sum() >= 20
    # per-ray times move the boundary: the same ray at another time has other roots
    m = BY_NAME["moving"]
    other = m["rays"].copy()
    other[:, 6] = 1.0 - other[:, 6]
    assert (R.roots(m["recs"], [0], other)[1] != R.roots(m["recs"], [0], m["rays"])[1]).sum() >= 20
    assert BY_NAME["negative_radius"]["recs"][0, 9] < 0 and got["negative_radius"]["collided"] >= 5
    # the edges, by name
    e = BY_NAME["edges"]
    a = answer(e)
    row = EDGE_ROWS
    st, t, dep, ac, rho = a["status"], a["t"], a["depth"], a["active"], a["rho"]
    has, s0, s1 = R.roots(e["recs"], [0], e["rays"])
    r0, r1 = s0[row["central"], 0], s1[row["central"], 0]
    assert st[row["central"]] == 0 and dep[row["central"]] == 1.0 and t[row["central"]] == INF
    assert st[row["tau_zero_outside"]] == 1 and t[row["tau_zero_outside"]] == r0 and ac[row["tau_zero_outside"]] == 1
    for name in ("tau_nan", "tau_negative", "range_empty", "range_reversed", "range_nan", "t_min_inf"):
        assert st[row[name]] == -1 and dep[row[name]] == 0 and ac[row[name]] == 0, name
    assert st[row["tau_negative_zero"]] == 1                                               # -0.0 >= 0
    assert st[row["tau_equals_step"]] == 0 and dep[row["tau_equals_step"]] == e["tau"][row["tau_equals_step"]]
    assert st[row["tau_just_below_step"]] == 1 and t[row["tau_just_below_step"]] <= r1
    assert st[row["origin_inside"]] == 1 and rho[row["origin_inside"]] == 0.5 and 0 < t[row["origin_inside"]]
    assert st[row["tau_zero_inside"]] == 1 and t[row["tau_zero_inside"]] == 0.0
    assert e["t_range"][row["on_boundary"], 0] == r0 and dep[row["on_boundary"]] == 1.0    # active at t == s0
    assert e["t_range"][row["on_far_boundary"], 0] == r1 and dep[row["on_far_boundary"]] == 0.0
    assert not has[row["tangent"], 0] and dep[row["tangent"]] == 0 and not has[row["miss"], 0]
    assert st[row["t_max_inside"]] == 0 and 0 < dep[row["t_max_inside"]] < 1.0 and t[row["t_max_inside"]] == 2.0
    assert st[row["t_max_at_s0"]] == 0 and dep[row["t_max_at_s0"]] == 0.0                  # tau = 0 never collides outside
    assert st[row["t_max_at_s1"]] == 0 and dep[row["t_max_at_s1"]] == 1.0
    assert st[row["t_max_inf_inside"]] == 0 and dep[row["t_max_inf_inside"]] == 0.5
    assert dep[row["behind"]] == 0 and st[row["zero_direction"]] == 0 and dep[row["zero_direction"]] == 0
    assert st[row["range_negative"]] == 0 and dep[row["range_negative"]] == 1.0
    for name in ("nan_origin", "nan_direction", "inf_direction", "inf_origin", "nan_time"):
        assert st[row[name]] in (0, 1), name
    if CLAMP is not None:
        c = BY_NAME["clamp"]
        clamped, loose = answer(c), answer(c, variant="no_clamp")
        has, s0, s1 = R.roots(c["recs"], [0], c["rays"])
        assert clamped["status"][0] == 1 and clamped["t"][0] == s1[0, 0] and loose["t"][0] > s1[0, 0]
    return got


# name: (collided at least, escaped with depth > 0 at least): half of what was measured (one 19 / 32, two_overlap 33 / 14, nested3
# 39 / 25, row64 36 / 70, coincident 24 / 22, sigma0 19 / 13, moving 15 / 18, negative_radius 27 / 32, edges 5 / 9)
FLOORS = {"one": (9, 16), "two_overlap": (16, 7), "nested3": (19, 12), "row64": (18, 35), "coincident": (12, 11), "sigma0": (9, 6),
          "moving": (7, 9), "negative_radius": (13, 16), "edges": (2, 4)}
