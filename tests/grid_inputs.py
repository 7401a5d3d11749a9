"""Named inputs of the heterogeneous-media queries (include/tor_grid.h), the smallest at which the kernel can go wrong: grids of
1 x 1 x 1, 2 x 2 x 2, 3 x 5 x 7 (a distinct density per cell: a wrong axis order shows), 64 x 3 x 2 and 16 x 16 x 16 cells; a dyadic
4 x 4 x 4 grid on [-1, 1]^3 with exact corner and edge ties; axis-parallel rays inside and outside the slab; a box smaller than the
sphere, larger than it, and offset from the centre; zero-density cells and an all-zero grid; a moving boundary; a negative radius;
a row, found by search, on which the guard (tn < t) decides the depth; a row whose collision parameter rounds above the step's
end (the clamp); named edge rows; one wave whose lanes take between 1 and 40 and more steps; lists of 1, 63, 64, 65 and 257.
Every case is a dict of recs (n_objects, 16), objects, sigma, albedo (or None), grid (grid_restatement.make_grid's), rays (n, 7),
tau (n,), t_range ((n, 2) or None).  assert_coverage() shows on the restatement alone that each case does what its name says."""
import numpy as np

import grid_restatement as R
import media_inputs as MI

INF, NAN = np.inf, np.nan
_sphere, _mover = MI._sphere, MI._mover


def _distinct(shape, seed):
    """A distinct density per cell, in (0.25, 2.25)."""
    n = int(np.prod(shape))
    return (0.25 + 2.0 * np.random.default_rng(seed).permutation(n) / n).reshape(shape)


def _case(name, recs, objects, sigma, medium, density, rays, box=None, tau=None, t_range=None, seed=1, albedo=None):
    recs = np.asarray(recs, dtype=np.float64)
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = len(rays)
    return dict(name=name, recs=recs, objects=np.asarray(objects, dtype=np.int32), sigma=np.asarray(sigma, dtype=np.float64),
                albedo=albedo, grid=R.make_grid(recs, objects, medium, density, box), density=np.asarray(density, dtype=np.float64),
                box=None if box is None else np.asarray(box, dtype=np.float64),
                rays=rays, tau=MI._taus(seed, n) * 2.0 if tau is None else np.asarray(tau, dtype=np.float64),
                t_range=None if t_range is None else np.ascontiguousarray(t_range, dtype=np.float64))


def _dyadic():
    """A ball of radius 2 with a 4 x 4 x 4 grid on [-1, 1]^3 (h = 0.5: every plane, and every crossing of the rays below, is exact).
    Rows 0 .. 7: the diagonals from the eight corners (+-2, +-2, +-2) towards the centre: every crossing is a three-way tie; 10
    steps, depth 2 sqrt(3) at sigma 1, density 1.  Rows 8 .. 19: face diagonals in the planes z = +-0.25 ..: two-way ties.  The rest seeded."""
    rows = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                rows.append([2.0 * sx, 2.0 * sy, 2.0 * sz, -1.0 * sx, -1.0 * sy, -1.0 * sz, 0.0])
    for z in (-0.75, -0.25, 0.25, 0.75):
        rows.append([-2.0, -2.0, z, 1.0, 1.0, 0.0, 0.0])
        rows.append([2.0, -2.0, z, -1.0, 1.0, 0.0, 0.0])
        rows.append([z, -2.0, 2.0, 0.0, 1.0, -1.0, 0.0])
    rays = np.concatenate([np.asarray(rows), MI._rays(41, 200, reach=4.0, spread=1.2)])
    tau = np.concatenate([np.full(len(rows), INF), MI._taus(42, 200) * 2.0])
    return _case("dyadic4", [_sphere((0, 0, 0), 2.0)], [0], [1.0], 0, np.ones((4, 4, 4)), rays, box=[-1, -1, -1, 1, 1, 1], tau=tau)


DIAGONAL_ROWS = range(8)


def _axis():
    """Axis-parallel rays (one or two of d_k == 0) through a 3 x 5 x 7 grid on the unit cube's half, inside and outside the slab."""
    g = np.random.default_rng(43)
    n = 216
    rays = np.zeros((n, 7))
    rays[:, 0:3] = g.uniform(-1.6, 1.6, (n, 3))
    axis = g.integers(0, 3, n)
    two = g.random(n) < 0.5
    d = g.uniform(0.3, 2.0, (n, 3)) * g.choice([-1.0, 1.0], (n, 3))
    for i in range(n):
        keep = [axis[i]] if two[i] else [axis[i], (axis[i] + 1) % 3]
        for k in range(3):
            if k not in keep:
                d[i, k] = 0.0
        rays[i, axis[i]] = -3.0 * np.sign(d[i, axis[i]])         # start outside along the moving axis
    rays[:, 3:6] = d
    rays[::9, 3:6] = np.where(rays[::9, 3:6] == 0.0, -0.0, rays[::9, 3:6])   # a negative zero is a zero
    return _case("axis", [_sphere((0, 0, 0), 2.0)], [0], [0.8], 0, _distinct((3, 5, 7), 7), rays, box=[-1, -1.2, -0.9, 1, 1.2, 0.9], seed=44)


def _wave():
    """A 16 x 16 x 16 grid, 257 rays: in every wave lanes that stop after one step (a short range, a corner clipped) next to
    diagonal lanes of 40 and more steps."""
    g = np.random.default_rng(45)
    n = 257
    rays = MI._rays(45, n, reach=4.0, spread=1.0)
    tau = MI._taus(46, n) * 4.0
    tr = np.zeros((n, 2))
    tr[:, 1] = INF
    diag = np.arange(0, n, 3)
    s = g.choice([-1.0, 1.0], (diag.size, 3))
    rays[diag, 0:3] = -2.0 * s + g.normal(size=(diag.size, 3)) * 0.01
    rays[diag, 3:6] = s * g.uniform(0.9, 1.1, (diag.size, 3))
    tau[diag] = INF
    short = np.arange(1, n, 3)
    rays[short, 0:3] = g.uniform(-0.5, 0.5, (short.size, 3))
    tr[short, 1] = g.uniform(0.001, 0.02, short.size)
    return _case("wave16", [_sphere((0, 0, 0), 2.0)], [0], [0.6], 0, _distinct((16, 16, 16), 16), rays, box=[-1, -1, -1, 1, 1, 1],
                 tau=tau, t_range=tr)


EDGE_ROWS = {}


def _edges():
    """The dyadic grid (ball of radius 2, 4 x 4 x 4 on [-1, 1]^3, sigma 1, density 1), hand-built rays; the named rows are in
    EDGE_ROWS.  base runs along +x at y = z = 0.25 with |d| = 3: in the box from t = 5/3 to 7/3, planes at 11/6, 2, 13/6."""
    recs = [_sphere((0, 0, 0), 2.0)]
    dens = np.ones((4, 4, 4))
    grid = R.make_grid(recs, [0], 0, dens, [-1, -1, -1, 1, 1, 1])
    base = np.array([-6.0, 0.25, 0.25, 3.0, 0, 0, 0.25])
    t_plane = (np.float64(-0.5) - np.float64(-6.0)) / np.float64(3.0)
    with np.errstate(all="ignore"):
        first = R.march_one(recs[0], 1.0, grid, base, INF, 0.0, t_plane)[2]       # the first cell's step
    rows, tau, tr = [], [], []

    def add(name, ray, t, rng=(0.0, INF)):
        EDGE_ROWS[name] = len(rows)
        rows.append(ray)
        tau.append(t)
        tr.append(rng)
    EDGE_ROWS.clear()
    add("central", base, INF)
    add("tau_zero_outside", base, 0.0)                          # collides AT the entry: rem = 0 < step
    add("tau_inf", base, INF)
    add("tau_nan", base, NAN)
    add("tau_negative", base, -1.0)
    add("tau_negative_zero", base, -0.0)
    add("tau_equals_step", base, first)                         # rem == step in the first cell: strict <, collides AT the plane in the next
    add("tau_just_below_step", base, np.nextafter(first, 0.0))
    add("tau_second_cell", base, 0.75)
    add("range_empty", base, 1.0, (2.0, 2.0))
    add("range_reversed", base, 1.0, (3.0, 1.0))
    add("range_nan", base, 1.0, (NAN, 3.0))
    add("range_negative", base, INF, (-INF, INF))
    add("t_min_inf", base, 1.0, (INF, INF))
    add("t_max_inside_cell", base, INF, (0.0, 2.1))
    add("t_max_on_plane", base, INF, (0.0, 2.0))                # x = 0 exactly
    add("t_max_at_entry", base, 0.0, (0.0, 5.0 / 3.0))
    add("t_min_on_plane", base, INF, (2.0, INF))
    add("origin_on_plane", [-0.5, 0.25, 0.25, 1.0, 0, 0, 0.0], INF)
    add("origin_on_plane_backwards", [-0.5, 0.25, 0.25, -1.0, 0, 0, 0.0], INF)
    add("origin_on_corner", [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0], INF)
    add("inside_backwards", [0.3, 0.25, 0.25, -1.0, 0, 0, 0.0], INF)
    add("origin_on_hi_face", [1.0, 0.25, 0.25, 1.0, 0, 0, 0.0], INF)     # q == hi: outside (half-open box)
    add("origin_on_lo_face", [-1.0, 0.25, 0.25, 1.0, 0, 0, 0.0], INF)
    add("in_sphere_outside_box", [0.0, 1.5, 0.0, 1.0, 0, 0, 0.0], INF)
    add("parallel_on_hi_face", [-3.0, 1.0, 0.25, 1.0, 0, 0, 0.0], INF)   # d_y == 0 and oc_y == hi_y: empty
    add("parallel_on_lo_face", [-3.0, -1.0, 0.25, 1.0, 0, 0, 0.0], INF)  # oc_y == lo_y: inside
    add("miss", [-6.0, 2.5, 0, 3.0, 0, 0, 0.0], 1.0)
    add("behind", [6.0, 0.25, 0.25, 3.0, 0, 0, 0.0], 1.0)
    add("zero_direction", [0.2, 0, 0, 0.0, 0, 0, 0.0], 1.0)
    add("zero_direction_outside", [3.0, 0, 0, 0.0, 0, 0, 0.0], INF)
    add("nan_origin", [NAN, 0, 0, 3.0, 0, 0, 0.0], 1.0)
    add("nan_direction", [-6.0, 0, 0, 3.0, NAN, 0, 0.0], 1.0)
    add("inf_direction", [-6.0, 0, 0, INF, 0, 0, 0.0], 1.0)
    add("inf_origin", [-INF, 0, 0, 3.0, 0, 0, 0.0], INF)
    add("huge_direction", [-6.0, 0.25, 0.25, 1e200, 0, 0, 0.0], 1.0)
    add("tiny_direction", [-6.0, 0.25, 0.25, 1e-170, 0, 0, 0.0], 1.0)
    add("nan_time", [-6.0, 0, 0, 3.0, 0, 0, NAN], 1.0)
    return _case("edges", recs, [0], [1.0], 0, dens, rows, box=[-1, -1, -1, 1, 1, 1], tau=tau, t_range=tr)


def near_plane_rays(n, seed):
    """Rays against the dyadic grid whose t_min lies within two ulps of a grid plane: (rays (n, 7), t_range (n, 2))."""
    g = np.random.default_rng(seed)
    o = g.uniform(-0.95, 0.95, (n, 3))
    d = g.normal(size=(n, 3)) * g.uniform(0.3, 3.0, n)[:, None]
    axis = g.integers(0, 3, n)
    plane = g.choice([-0.5, 0.0, 0.5], n)
    rows = np.arange(n)
    t = (plane - o[rows, axis]) / d[rows, axis]
    flip = t < 0
    d[flip] = -d[flip]
    t = np.abs(t)
    for _ in range(2):
        step = g.integers(-1, 2, n)
        t = np.where(step > 0, np.nextafter(t, INF), np.where(step < 0, np.nextafter(t, 0.0), t))
    tr = np.stack([t, np.full(n, INF)], axis=1)
    return np.concatenate([o, d, np.zeros((n, 1))], axis=1), tr


def _dyadic_parts():
    recs = [_sphere((0, 0, 0), 2.0)]
    dens = _distinct((4, 4, 4), 4)
    return recs, dens, R.make_grid(recs, [0], 0, dens, [-1, -1, -1, 1, 1, 1])


def search_guard(n, seed):
    """(rows where tn < t held at least once, those of them whose depth changes without the guard, rays, t_range)."""
    recs, dens, grid = _dyadic_parts()
    rays, tr = near_plane_rays(n, seed)
    trails = {}
    a = R.march(recs, [0], [1.0], grid, rays, INF, tr, trails=trails)
    b = R.march(recs, [0], [1.0], grid, rays, INF, tr, variant="no_guard")
    hit = [i for i in range(n) if trails[i].get("guard", 0) > 0]
    changed = [i for i in hit if a["depth"][i] != b["depth"][i]]
    return hit, changed, rays, tr


def search_clamp(n, seed):
    """media_inputs.search_clamp's rows (the unit ball, the origin inside, tau the largest float64 below the one step) that decide
    the 1 x 1 x 1 grid of density 1 as well: the arithmetic of the only step is the same."""
    found = []
    for ray, sg, tau in MI.search_clamp(n, seed):
        recs = [_sphere((0, 0, 0), 1.0)]
        grid = R.make_grid(recs, [0], 0, np.ones((1, 1, 1)))
        with np.errstate(all="ignore"):
            a = R.march_one(recs[0], sg, grid, ray, tau, 0.0, INF)
            b = R.march_one(recs[0], sg, grid, ray, tau, 0.0, INF, "no_collision_clamp")
        if a[0] == 1 and b[1] > a[1]:
            found.append((ray, sg, tau))
    return found


# the first row search_guard(4000, 7) reports as changed: t_min within two ulps of a plane of the dyadic grid, tn < t at the first step
GUARD = None


def _guard():
    recs, dens, grid = _dyadic_parts()
    ray, t_min = GUARD
    return _case("guard", recs, [0], [1.0], 0, dens, [ray], box=[-1, -1, -1, 1, 1, 1], tau=[INF], t_range=[[t_min, INF]])


def _clamp():
    ray, sg, tau = MI.CLAMP
    return _case("clamp", [_sphere((0, 0, 0), 1.0)], [0], [sg], 0, np.ones((1, 1, 1)), [ray], tau=[tau])


def _build():
    ball2 = [_sphere((0, 0, 0), 2.0)]
    zeros = _distinct((4, 4, 4), 8)
    zeros[np.random.default_rng(9).random((4, 4, 4)) < 0.4] = 0.0
    cases = [
        _case("g1", [_sphere((0, 0, 0), 1.0)], [0], [0.5], 0, np.full((1, 1, 1), 1.5), MI._rays(1, 200), seed=2),
        _case("g2", [_sphere((0, 0, 0), 1.0), _sphere((0, 9, 9), 0.5, 1), _sphere((0.8, 0, 0), 1.0)], [2, 0], [0.7, 1.3], 1,
              _distinct((2, 2, 2), 2), MI._rays(3, 208), seed=4, albedo=[[0.9, 0.1, 0.5], [0.2, 0.8, 1.0]]),
        _case("g357", ball2, [0], [0.9], 0, _distinct((3, 5, 7), 3), MI._rays(5, 240, reach=5.0, spread=2.0), seed=6),
        _case("g64x3x2", ball2, [0], [3.0], 0, _distinct((64, 3, 2), 64), MI._rays(7, 256, reach=5.0, spread=2.0), box=[-1.9, -0.3, -0.2, 1.9, 0.3, 0.2], seed=8),
        _dyadic(),
        _axis(),
        _case("box_small", ball2, [0], [1.1], 0, _distinct((3, 4, 5), 10), MI._rays(11, 200, reach=5.0, spread=1.5), box=[-0.5, -0.6, -0.4, 0.5, 0.7, 0.3], seed=12),
        _case("box_large", [_sphere((0, 0, 0), 1.0)], [0], [1.1], 0, _distinct((5, 4, 3), 13), MI._rays(13, 200), box=[-3, -2.5, -2, 3, 2.5, 2], seed=14),
        _case("box_offset", [_sphere((1, -1, 0.5), 1.5)], [0], [0.9], 0, _distinct((4, 3, 5), 15),
              MI._rays(15, 200, centre=(1, -1, 0.5), reach=5.0, spread=1.8), box=[0.1, -0.4, -1.2, 1.6, 0.9, 0.2], seed=16),
        _case("zeros", ball2, [0], [1.0], 0, zeros, MI._rays(17, 200, reach=4.0, spread=1.2), box=[-1, -1, -1, 1, 1, 1], seed=18),
        _case("all_zero", ball2, [0], [1.0], 0, np.zeros((3, 3, 3)), MI._rays(19, 200, reach=4.0, spread=1.2), seed=20),
        _case("moving", [_mover((-1, 0, 0), (1, 0.5, 0), 0.0, 1.0, 1.2), _sphere((0, 0, 0), 0.7)], [0, 1], [0.8, 0.3], 0,
              _distinct((4, 4, 4), 21), MI._rays(21, 200, spread=2.0), seed=22),
        _case("negative_radius", [_sphere((0, 0, 0), -1.5)], [0], [0.5], 0, _distinct((3, 3, 3), 23), MI._rays(23, 200), seed=24),
        _wave(),
        _edges(),
        _clamp(),
    ]
    if GUARD is not None:
        cases.append(_guard())
    return cases


GUARD = None
CASES = []
BY_NAME = {}
NAMES = []


def _finish():
    global CASES, BY_NAME, NAMES
    CASES = _build()
    BY_NAME = {c["name"]: c for c in CASES}
    NAMES = [c["name"] for c in CASES]


def answer(c, index=None, into=None, steps=None, variant=None, trails=None):
    return R.march(c["recs"], c["objects"], c["sigma"], c["grid"], c["rays"], c["tau"], c["t_range"], index, into, steps, variant, trails)


def lookup_points(c, n=200, seed=5):
    """Points around the case's medium, with the rays' times: inside the box, inside the sphere only, outside both; the first rows on
    the box's faces (lo: inside; hi: outside)."""
    g = np.random.default_rng(seed)
    rec = c["recs"][int(c["objects"][c["grid"]["medium"]])]
    lo, hi = np.asarray(c["grid"]["lo"]), np.asarray(c["grid"]["hi"])
    pts = np.zeros((n, 4))
    pts[:, 3] = g.random(n)
    centre = np.asarray([R._centre(rec, t) for t in pts[:, 3]], dtype=np.float64)
    span = np.maximum(np.abs(lo), np.abs(hi)).max() * 1.3
    pts[:, 0:3] = centre + g.uniform(-span, span, (n, 3))
    mid = (lo + hi) / 2
    if int(rec[0]) == 0:                                       # exact faces need an exact centre
        for k in range(3):
            for j, face in enumerate((lo, hi)):
                q = mid.copy()
                q[k] = face[k]
                pts[2 * k + j, 0:3] = centre[2 * k + j] + q
    return pts


def lists():
    """Lists over wave16's 257 rays: lengths 1, 63, 64, 65 and 257 (the last with two entries outside [0, n), which are skipped)."""
    return MI.lists()


def physics_case(n=4096, seed=31):
    """The statistics check's two-slab grid: the unit ball, sigma 1, a 2 x 1 x 1 grid on its bounding cube with density 0 for x < 0
    and 2 for x >= 0, and n central rays: each crosses a radius of density 0 and a radius of density 2 -- depth 2 -- except
    where it runs in the plane x = 0.  The expected collision fraction is 1 - exp(-2)."""
    rays, _ = MI.physics_rays(n, seed)
    dens = np.asarray([0.0, 2.0]).reshape(2, 1, 1)
    recs = np.asarray([_sphere((0, 0, 0), 1.0)], dtype=np.float64)
    return dict(recs=recs, objects=np.asarray([0], dtype=np.int32), sigma=np.asarray([1.0]), density=dens, box=None,
                grid=R.make_grid(recs, [0], 0, dens), rays=rays)


PHYSICS_P = 1.0 - np.exp(-2.0)
PHYSICS_TOL = 5.0 * np.sqrt(PHYSICS_P * (1.0 - PHYSICS_P) / 4096)    # 5 binomial standard errors at 4096 rays: 0.0267


class _Close(float):
    """A depth of the hand-built rows compared with the value worked by hand: a sum of at most 4 steps, each a few roundings of
    thirds and sixths at magnitude <= 2: equal within 16 ulps of 2."""

    def __eq__(self, other):
        return abs(float(self) - float(other)) <= 16 * 2.0 ** -52 * 2.0

    def __ne__(self, other):
        return not self == other

    __hash__ = float.__hash__


class _Near:
    def __init__(self, values):
        self.values = values

    def __getitem__(self, i):
        return _Close(self.values[i])


def assert_coverage():
    """Each case does what its name says, on the restatement alone; returns the measured counts (the floors below are half of what
    was measured when the cases were made)."""
    got = {}
    all_steps = {}
    for c in CASES:
        n = len(c["rays"])
        steps = np.zeros(n, dtype=np.int64)
        trails = {}
        a = answer(c, steps=steps, trails=trails)
        all_steps[c["name"]] = steps
        got[c["name"]] = dict(n=n, collided=int((a["status"] == 1).sum()), refused=int((a["status"] == -1).sum()),
                              depth_pos=int(((a["status"] == 0) & (a["depth"] > 0)).sum()), max_steps=int(steps.max()),
                              multi_step=int((steps >= 3).sum()), cells=len(set(a["cell"][a["cell"] >= 0].tolist())),
                              zero_depth_walks=int(((a["status"] == 0) & (a["depth"] == 0) & (steps > 0)).sum()),
                              guard=sum(1 for t in trails.values() if t.get("guard", 0)),
                              clamped=sum(1 for t in trails.values() if t.get("clamped", 0)))
    for name, (col, esc) in FLOORS.items():
        assert got[name]["collided"] >= col and got[name]["depth_pos"] >= esc, (name, got[name])
    for c in CASES:
        if c["name"] not in ("edges", "clamp", "guard"):
            assert 200 <= len(c["rays"]) <= 260, c["name"]
    assert BY_NAME["g1"]["grid"]["n"] == (1, 1, 1) and BY_NAME["g2"]["grid"]["n"] == (2, 2, 2) and BY_NAME["g357"]["grid"]["n"] == (3, 5, 7)
    assert BY_NAME["g64x3x2"]["grid"]["n"] == (64, 3, 2) and got["g64x3x2"]["max_steps"] >= 30
    assert got["g357"]["cells"] >= 30 and len(set(BY_NAME["g357"]["density"].reshape(-1).tolist())) == 105
    # the dyadic grid: the diagonals take 10 steps through exact three-way ties to depth 2 sqrt(3) (|d| = sqrt(3), 2 units of t)
    c = BY_NAME["dyadic4"]
    a = answer(c)
    for i in DIAGONAL_ROWS:
        assert all_steps["dyadic4"][i] == 10 and a["status"][i] == 0, (i, all_steps["dyadic4"][i])
        assert abs(a["depth"][i] - 2.0 * np.sqrt(3.0)) <= 4e-15
    assert (all_steps["dyadic4"][8:20] == 7).all() and np.abs(a["depth"][8:20] - 2.0 * np.sqrt(2.0)).max() <= 4e-15
    # axis-parallel rays: every ray has a zero component; some are inside the slab and gather depth, some outside and are empty
    c = BY_NAME["axis"]
    assert ((c["rays"][:, 3:6] == 0).sum(axis=1) >= 1).all() and got["axis"]["depth_pos"] + got["axis"]["collided"] >= 40
    assert int((all_steps["axis"] == 0).sum()) >= 40 and np.signbit(c["rays"][:, 3:6][c["rays"][:, 3:6] == 0]).any()
    # the boxes: smaller (clipped by the box: depth only inside it), larger (clipped by the sphere), offset
    for name in ("box_small", "box_large", "box_offset"):
        c = BY_NAME[name]
        R2 = c["recs"][int(c["objects"][0]), 9] ** 2
        lo, hi = np.asarray(c["grid"]["lo"]), np.asarray(c["grid"]["hi"])
        corner2 = (np.maximum(np.abs(lo), np.abs(hi)) ** 2).sum()
        assert (corner2 < R2) == (name == "box_small") and ((np.minimum(np.abs(lo), np.abs(hi)) ** 2).min() > R2) == (name == "box_large")
    assert not np.allclose(np.asarray(BY_NAME["box_offset"]["grid"]["lo"]), -np.asarray(BY_NAME["box_offset"]["grid"]["hi"]))
    assert got["zeros"]["collided"] >= 20 and (BY_NAME["zeros"]["density"] == 0).sum() >= 15
    assert got["all_zero"]["collided"] == 0 and got["all_zero"]["depth_pos"] == 0 and got["all_zero"]["zero_depth_walks"] >= 50
    # per-ray times move the boundary and the grid with it
    m = BY_NAME["moving"]
    other = dict(m, rays=m["rays"].copy())
    other["rays"][:, 6] = 1.0 - other["rays"][:, 6]
    assert (answer(other)["depth"] != answer(m)["depth"]).sum() >= 50
    assert BY_NAME["negative_radius"]["recs"][0, 9] < 0 and got["negative_radius"]["collided"] >= 10
    assert np.array_equal(np.asarray(BY_NAME["negative_radius"]["grid"]["hi"]), [1.5, 1.5, 1.5])
    # one wave: lanes of 1 step next to lanes of 40 and more
    first_wave = all_steps["wave16"][:64]
    assert first_wave.max() >= 40 and (first_wave == 1).sum() >= 10 and first_wave.min() <= 1, (first_wave.max(), first_wave.min())
    # the guard and the clamp
    if GUARD is not None:
        c = BY_NAME["guard"]
        assert got["guard"]["guard"] == 1 and answer(c)["depth"][0] != answer(c, variant="no_guard")["depth"][0]
    c = BY_NAME["clamp"]
    clamped, loose = answer(c), answer(c, variant="no_collision_clamp")
    assert clamped["status"][0] == 1 and loose["t"][0] > clamped["t"][0]
    # the edges, by name
    e = BY_NAME["edges"]
    a = answer(e)
    row = EDGE_ROWS
    st, t, dep, ac, rho, cell = a["status"], a["t"], _Near(a["depth"]), a["active"], a["rho"], a["cell"]
    assert st[row["central"]] == 0 and dep[row["central"]] == 2.0 and t[row["central"]] == INF and cell[row["central"]] == -1
    assert st[row["tau_zero_outside"]] == 1 and t[row["tau_zero_outside"]] == 5.0 / 3.0 and ac[row["tau_zero_outside"]] == 1
    assert cell[row["tau_zero_outside"]] == (0 * 4 + 2) * 4 + 2
    for name in ("tau_nan", "tau_negative", "range_empty", "range_reversed", "range_nan", "t_min_inf"):
        assert st[row[name]] == -1 and dep[row[name]] == 0 and ac[row[name]] == 0 and cell[row[name]] == -1, name
    assert st[row["tau_negative_zero"]] == 1
    assert st[row["tau_equals_step"]] == 1 and cell[row["tau_equals_step"]] == (1 * 4 + 2) * 4 + 2     # not in the first cell: in the second
    assert t[row["tau_equals_step"]] == (np.float64(-0.5) + 6.0) / 3.0
    assert st[row["tau_just_below_step"]] == 1 and cell[row["tau_just_below_step"]] == (0 * 4 + 2) * 4 + 2
    assert st[row["tau_second_cell"]] == 1 and cell[row["tau_second_cell"]] == (1 * 4 + 2) * 4 + 2 and rho[row["tau_second_cell"]] == 1.0
    assert st[row["range_negative"]] == 0 and dep[row["range_negative"]] == 2.0
    assert 0.9 < float(dep[row["t_max_inside_cell"]]) < 1.9 and t[row["t_max_inside_cell"]] == 2.1
    assert dep[row["t_max_on_plane"]] == 1.0 and dep[row["t_min_on_plane"]] == 1.0
    assert st[row["t_max_at_entry"]] == 0 and dep[row["t_max_at_entry"]] == 0.0
    assert dep[row["origin_on_plane"]] == 1.5 and dep[row["origin_on_plane_backwards"]] == 0.5
    assert abs(dep[row["origin_on_corner"]] - np.sqrt(3.0)) <= 4e-15 and dep[row["inside_backwards"]] == 1.3
    assert dep[row["origin_on_hi_face"]] == 0.0 and dep[row["origin_on_lo_face"]] == 2.0
    assert dep[row["in_sphere_outside_box"]] == 0.0 and dep[row["parallel_on_hi_face"]] == 0.0 and dep[row["parallel_on_lo_face"]] == 2.0
    assert dep[row["miss"]] == 0 and dep[row["behind"]] == 0 and dep[row["zero_direction"]] == 0 and st[row["zero_direction"]] == 0
    for name in ("nan_origin", "nan_direction", "inf_direction", "inf_origin", "nan_time", "huge_direction", "tiny_direction"):
        assert st[row[name]] in (0, 1), name
    return got


# set here, after the searches above exist: the first changed row of search_guard(4000, 7) as (ray, t_min)
GUARD = (np.array([float.fromhex(h) for h in ("-0x1.0b5185a63b6ccp-1", "-0x1.84cbe5db2d8ecp-2", "0x1.6b648dfee21cep-1", "0x1.0708ed3df1e4cp+0",
                                               "-0x1.39102bae4706fp+0", "-0x1.165498d564d70p+0", "0x0.0p+0")]), float.fromhex("0x1.92fcb0ae962edp-4"))
# name: (collided at least, escaped with depth > 0 at least): half of what was measured (g1 62 / 70, g2 58 / 87, g357 123 / 99, g64x3x2
# 26 / 30, dyadic4 81 / 123, axis 23 / 36, box_small 19 / 57, box_large 56 / 89, box_offset 32 / 50, zeros 73 / 105, moving 48 / 77,
# negative_radius 86 / 98, wave16 30 / 227, edges 6 / 12)
FLOORS = {"g1": (31, 35), "g2": (29, 43), "g357": (61, 49), "g64x3x2": (13, 15), "dyadic4": (40, 61), "axis": (11, 18),
          "box_small": (9, 28), "box_large": (28, 44), "box_offset": (16, 25), "zeros": (36, 52), "moving": (24, 38),
          "negative_radius": (43, 49), "wave16": (15, 113), "edges": (3, 6)}
_finish()
