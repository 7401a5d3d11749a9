"""Named inputs of the planar patch queries (include/tor_patches.h), at the smallest sizes at which they can go wrong: tables of 1, 2,
4, 9, 63, 64, 65 and 130 patches, about 250 rays or fewer each.  A case is a dict: table (patch_restatement's patches), rays (n, 7),
t_range ((n, 2) or None), mask (per-ray words, an int or None), recs (the (m, 16) spheres of the scene) and sphere (None, or the
(n, 8) sphere records a merge starts from; "world": hit_restatement.world_hit's).  assert_coverage() proves on the CPU, with the
restatement alone, that every case does what its name says."""
import numpy as np

import hit_restatement as H
import patch_restatement as R

INF, NAN = np.inf, np.nan

# three spheres that carry the materials the patches wear: Lambertian, Metal, Dielectric (records as Scene.to_records gives them)
SPHERES = np.array([[0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0, 1, 1.0, 0, 0.7, 0.6, 0.5, 0.0, 0.0],
                    [0, -2.5, 1.0, 0.5, -2.5, 1.0, 0.5, 0, 1, 1.0, 1, 0.8, 0.8, 0.9, 0.1, 0.0],
                    [0, 2.5, 1.0, -0.5, 2.5, 1.0, -0.5, 0, 1, 1.0, 2, 1.0, 1.0, 1.0, 0.0, 1.5]], dtype=np.float64)
FAR = SPHERES + np.array([0, 0, 500.0, 0, 0, 500.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])      # the same, out of every test ray's way


def up(x, k=1):
    for _ in range(k):
        x = np.nextafter(x, INF)
    return float(x)


def down(x, k=1):
    for _ in range(k):
        x = np.nextafter(x, -INF)
    return float(x)


def rays_of(origins, directions, time=0.0):
    o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    d = np.broadcast_to(d, o.shape)
    return np.ascontiguousarray(np.concatenate([o, d, np.full((o.shape[0], 1), time)], axis=1))


def _both_sides(points):
    """Rays straight down from y = 1 and straight up from y = -1 through the points (x, z) of the plane y = 0: t = 1 exactly."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    above = rays_of([(x, 1.0, z) for x, z in pts], (0.0, -1.0, 0.0))
    below = rays_of([(x, -1.0, z) for x, z in pts], (0.0, 1.0, 0.0))
    return np.concatenate([above, below])


# the unit patches of the hand-worked rows, scaled by exactly representable edges: x = 2a, z = 4b
UNIT_QUAD = R.quad((0, 0, 0), (2, 0, 0), (0, 0, 4), material=0)
UNIT_TRIANGLE = R.triangle((0, 0, 0), (2, 0, 0), (0, 0, 4), material=1)
_XS, _ZS = [down(0.0), 0.0, 1.0, 2.0, up(2.0)], [down(0.0), 0.0, 2.0, 4.0, up(4.0)]
_GRID = [(x, z) for x in _XS for z in _ZS]
_HYPOTENUSE = [(1.0, 2.0), (0.5, 3.0), (1.5, 1.0), (up(1.0), 2.0), (1.0, up(2.0)), (up(1.0, 2), 2.0), (1.0, up(2.0, 2)), (up(1.0), up(2.0))]
_FAR_OFF = [(-3.0, 1.0), (5.0, 1.0), (1.0, -2.0), (1.0, 9.0), (1.75, 3.5)]


def _case(table, rays, t_range=None, mask=None, recs=FAR, sphere=None):
    return {"table": list(table), "rays": np.ascontiguousarray(rays, dtype=np.float64),
            "t_range": None if t_range is None else np.ascontiguousarray(t_range, dtype=np.float64),
            "mask": mask, "recs": recs, "sphere": sphere}


def _fabricated(n, ts, objects):
    raw = np.zeros((n, 8))
    w = raw.view(np.int32)
    w[:, 14] = -1
    for i, (t, obj) in enumerate(zip(ts, objects)):
        raw[i, 0:3], raw[i, 3:6], raw[i, 6] = (9.0, 9.0, 9.0), (0.0, 1.0, 0.0), t
        w[i, 14], w[i, 15] = obj, 1
    return raw


def _soup(n_patches, seed, n_rays=250):
    rng = np.random.default_rng(seed)
    table = []
    for j in range(n_patches):
        q, u, v = rng.uniform(-3, 3, 3), rng.normal(0, 2.0, 3), rng.normal(0, 2.0, 3)
        make = R.quad if rng.random() < 0.5 else (lambda q, u, v, m: R.triangle(q, q + u, q + v, m))
        table.append(make(q, u, v, int(rng.integers(-1, 3))))
    o = rng.uniform(-3, 3, (n_rays, 3))
    d = rng.normal(size=(n_rays, 3))
    return _case(table, rays_of(o, d), recs=FAR)


def box(lo, hi, material=-1, groups=0xFFFFFFFF):
    """tor.box_patches restated: -x, +x, -y, +y, -z, +z, cross(u, v) outwards."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    e = np.diag(hi - lo)
    out = []
    for k in range(3):
        a, b = e[(k + 1) % 3], e[(k + 2) % 3]
        out += [R.quad(lo, b, a, material, groups), R.quad(lo + e[k], a, b, material, groups)]
    return out


ROOM_SPHERES = np.array([[0, -1.5, 0.8, -1.0, -1.5, 0.8, -1.0, 0, 1, 0.8, 0, 0.73, 0.73, 0.73, 0.0, 0.0],
                         [0, 1.6, 0.6, 1.2, 1.6, 0.6, 1.2, 0, 1, 0.6, 1, 0.9, 0.8, 0.6, 0.05, 0.0],
                         [0, 0.2, 2.6, 0.3, 0.2, 2.6, 0.3, 0, 1, 0.5, 2, 1.0, 1.0, 1.0, 0.0, 1.5]], dtype=np.float64)
ROOM_LAMP = 5          # the lamp panel's index in the room's table


def room_table():
    """A room of 6 x 5 x 6 open towards the camera (+z): floor, ceiling, back, left and right wall, a lamp panel just under the
    ceiling (no material), a Lambertian box and a glass box."""
    walls = [R.quad((-3, 0, -3), (6, 0, 0), (0, 0, 6), 0), R.quad((-3, 5, -3), (0, 0, 6), (6, 0, 0), 0),
             R.quad((-3, 0, -3), (0, 5, 0), (6, 0, 0), 0), R.quad((-3, 0, -3), (0, 0, 6), (0, 5, 0), 0),
             R.quad((3, 0, -3), (0, 5, 0), (0, 0, 6), 1)]
    lamp = [R.quad((-1, 4.96875, -1), (2, 0, 0), (0, 0, 2), -1)]
    return walls + lamp + box((0.5, 0, -2.25), (2.0, 2.5, -0.75), 0) + box((-2.5, 0, 0.5), (-1.75, 1.0, 1.5), 2)


def pinhole_rays(nrows, ncols, origin=(0.0, 2.5, 9.0), look=(0.0, 2.25, 0.0), half_width=0.42):
    """One ray per pixel of a plain pinhole camera (no lens, time 0), row-major."""
    o, w = np.asarray(origin), np.asarray(look) - np.asarray(origin)
    w = w / np.linalg.norm(w)
    a = np.cross(w, (0.0, 1.0, 0.0))
    a /= np.linalg.norm(a)
    b = np.cross(a, w)
    s, t = np.meshgrid((np.arange(ncols) + 0.5) / ncols * 2 - 1, (np.arange(nrows) + 0.5) / nrows * 2 - 1)
    d = w[None, :] + half_width * (s.reshape(-1, 1) * a[None, :] + t.reshape(-1, 1) * nrows / ncols * b[None, :])
    return rays_of(np.broadcast_to(o, d.shape), d)


def _build():
    c = {}
    c["one_quad"] = _case([UNIT_QUAD], _both_sides(_GRID + _FAR_OFF))
    c["one_triangle"] = _case([UNIT_TRIANGLE], _both_sides(_GRID + _HYPOTENUSE + _FAR_OFF))
    # det == 0 exactly, rays in the plane, a zero and a NaN direction, infinite origins; two honest hits for contrast
    c["parallel"] = _case([UNIT_QUAD, R.triangle((0, -1, 0), (2, -1, 0), (0, -1, 4), 1)], rays_of(
        [(-1, 0, 1), (1, 0, -1), (0, 1, 0), (0.5, 1, 0.5), (1, 1, 1), (1, 1, 1), (1, 1, 1), (INF, 1, 1), (1, INF, 1), (1, -INF, 1), (1, 1, 1),
         (0.25, 1, 0.25)],
        [(1, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0), (0, 0, 0), (NAN, -1, 0), (0, NAN, 0), (0, -1, 0), (0, -1, 0), (0, 1, 0), (0, -1, 0),
         (0.125, -1, 0.25)]))
    # t == 1 for the rays from above, t == -1 for those that look away from the patch
    tr = [(1.0, 2.0), (0.0, 1.0), (0.5, 1.5), (down(1.0), up(1.0)), (up(1.0), 2.0), (0.0, down(1.0)), (2.0, 0.5), (NAN, 2.0), (0.0, NAN),
          (NAN, NAN), (-INF, INF), (-2.0, 0.0), (-2.0, -1.0), (-1.0, 0.0), (-1.5, -0.5), (0.001, INF)]
    o = [(1, 1, 1)] * 11 + [(1, -1, 1)] * 4 + [(1, 1, 1)]
    c["range"] = _case([UNIT_QUAD], rays_of(o, (0, -1, 0)), t_range=tr)
    ys = [0.0005, down(0.001), 0.001, up(0.001), 0.002, 1.0, -0.5, 0.0]
    c["default_range"] = _case([UNIT_QUAD], rays_of([(1, y, 1) for y in ys], (0, -1, 0)))
    # coincident pairs in both orders of their materials; sphere records at the patch's t, one ulp below and one ulp above
    pairs = [R.quad((0, 0, 0), (2, 0, 0), (0, 0, 4), 0), R.quad((0, 0, 0), (2, 0, 0), (0, 0, 4), 1),
             R.quad((4, 0, 0), (2, 0, 0), (0, 0, 4), 1), R.quad((4, 0, 0), (2, 0, 0), (0, 0, 4), 0)]
    rays = rays_of([(1, 1, 1)] * 6 + [(5, 1, 1)] * 6, (0, -1, 0))
    ts, objs = [1.0, down(1.0), up(1.0), 1.0, 0.5, 2.0] * 2, [2, 2, 2, -1, 2, 2] * 2
    c["ties"] = _case(pairs, rays, sphere=_fabricated(12, ts, objs))
    c["ties_range"] = _case(pairs, rays, t_range=[(0.0, 1.5)] * 12, sphere=_fabricated(12, [1.0, down(1.0), up(1.0), 1.0, 3.0, 1.25] * 2, objs))
    # material -1 and >= 0, seen from the front and from behind
    mats = [R.quad((0, 0, 0), (2, 0, 0), (0, 0, 4), -1), R.quad((4, 0, 0), (2, 0, 0), (0, 0, 4), 0),
            R.triangle((8, 0, 0), (10, 0, 0), (8, 0, 4), 2), R.quad((12, 0, 0), (0, 0, 4), (2, 0, 0), 1)]
    c["materials"] = _case(mats, _both_sides([(x + 0.5, 1.0) for x in (0, 4, 8, 12, 16)]), recs=SPHERES + np.array([0, 0, 0, 50.0] + [0, 0, 50.0] + [0] * 9))
    # four sheets one under the other with the group words 1, 2, 0 and all ones
    sheets = [R.quad((0, -k, 0), (2, 0, 0), (0, 0, 4), k % 3, g) for k, g in enumerate((1, 2, 0, 0xFFFFFFFF))]
    words = [1, 2, 3, 0, 0xFFFFFFFF, 4, 0x80000000, 2, 1, 0]
    c["masks"] = _case(sheets, rays_of([(1, 1, 1)] * len(words), (0, -1, 0)), mask=np.array(words, dtype=np.uint32))
    c["mask_scalar"] = _case(sheets, rays_of([(1, 1, 1), (0.5, 1, 3), (9, 1, 9)], (0, -1, 0)), mask=2)
    c["mask_zero"] = _case(sheets, rays_of([(1, 1, 1), (0.5, 1, 3)], (0, -1, 0)), mask=0)
    # magnitudes of 1e-160 and 1e160: products underflow, det becomes infinite
    big = [R.quad((0, 0, 0), (1e100, 0, 0), (0, 0, 1e50), 0), R.quad((0, -1, 0), (1e-160, 0, 0), (0, 0, 1e160), 1),
           R.triangle((0, -2, 0), (1e-75, -2, 0), (0, -2, 1e-75), 2)]
    o = [(0.5e100, 1e160, 0.5e50), (0.5e100, 1, 0.5e50), (0.5e100, 1e-160, 0.5e50), (0.5e-160, 0, 0.5e160), (0.5e-160, 0, 0.5e160),
         (0.25e-75, -1.5, 0.25e-75), (0.25e-75, -1.5, 0.25e-75), (0.25e-75, -2 + 1e-160, 0.25e-75), (1e160, 1e160, 1e160), (1e-160, 1, 1e-160)]
    d = [(0, -1e160, 0), (0, -1e200, 0), (0, -1e-160, 0), (0, -1e-160, 0), (0, -1e160, 0), (0, -1e-160, 0), (0, -1e-250, 0), (0, -1e-160, 0),
         (-1e160, -1e160, -1e160), (1e-160, -1, 1e-160)]
    c["overflow"] = _case(big, rays_of(o, d))
    for k, n in enumerate((9, 63, 64, 65, 130)):
        c[f"soup{n}"] = _soup(n, 7100 + k, 120 if n == 9 else 250)
    c["room"] = _case(room_table(), pinhole_rays(15, 16), recs=ROOM_SPHERES, sphere="world")
    return c


BY_NAME = _build()
NAMES = list(BY_NAME)


def sphere_records(case):
    """The sphere records a merge of the case starts from: the fabricated ones, world_hit's, or None."""
    if isinstance(case["sphere"], str):
        return H.world_hit(case["recs"], case["rays"], case["t_range"])
    return case["sphere"]


def answer(name, variant=None):
    """What the restatement says of a case: hit alone, hit merged (where the case has sphere records) and the any-hit bits."""
    c = BY_NAME[name]
    args = (c["table"], c["rays"], c["t_range"], c["mask"])
    out = {"hit": R.hit(*args, variant=variant), "occluded": R.occluded(*args, variant=variant)}
    if c["sphere"] is not None:
        out["merge"] = R.hit(*args, merge=sphere_records(c), variant=variant)
    return out


def lists(n, seed=5):
    """Lists of length 1, 63, 64, 65 and 255 over n rays: unique entries in random order, a few of them outside [0, n)."""
    rng = np.random.default_rng(seed)
    out = {}
    for m in (1, 63, 64, 65, 255):
        inside = rng.permutation(n)[:min(m, n) - (0 if m == 1 else 3)]
        outside = np.array([] if m == 1 else [-1, n, n + 7], dtype=np.int64)
        more = np.arange(n + 100, n + 100 + m - inside.size - outside.size)       # a list longer than the batch: the rest lies outside too
        out[m] = rng.permutation(np.concatenate([inside, outside, more])).astype(np.int32)
        assert out[m].size == m and np.unique(out[m]).size == m
    return out


def assert_coverage():
    """Every case does what its name says, by the restatement alone."""
    with np.errstate(all="ignore"):
        assert [len(BY_NAME[k]["table"]) for k in ("one_quad", "ties", "soup9", "soup63", "soup64", "soup65", "soup130")] == [1, 4, 9, 63, 64, 65, 130]
        assert len(BY_NAME["parallel"]["table"]) == 2 and all(BY_NAME[k]["rays"].shape[0] <= 260 for k in NAMES)
        for k in NAMES:
            assert R.refusal(BY_NAME[k]["table"], BY_NAME[k]["recs"].shape[0]) is None, k
        # the unit patches: the edges and corners are hit exactly, one ulp outside is a miss, from both sides
        for name, n_grid in (("one_quad", 25), ("one_triangle", 25)):
            c, a = BY_NAME[name], answer(name)["hit"]
            half = c["rays"].shape[0] // 2
            o, d = tuple(c["rays"][:, k] for k in range(3)), tuple(c["rays"][:, 3 + k] for k in range(3))
            _, t, an, bn, det = R.pair(c["table"][0], o, d)
            assert (t[np.isfinite(t)] == 1.0).all() and (det == 8.0).all()
            assert (an == 0).any() and (bn == 0).any() and ((an == det) & (bn == det)).any() and ((an < 0) & (an > -1e-300)).any()
            f = H.fields(a["raw"])
            assert set(f["front_face"][:half][a["patch"][:half] >= 0]) == {0} and set(f["front_face"][half:][a["patch"][half:] >= 0]) == {1}
            for side in (0, half):
                got = (a["patch"][side:side + n_grid] >= 0).reshape(5, 5)
                if name == "one_quad":
                    want = np.zeros((5, 5), dtype=bool)
                    want[1:4, 1:4] = True                                       # x in {0, 1, 2} and z in {0, 2, 4}: the corners included
                else:
                    want = np.array([[xi in (1, 2, 3) and zi in (1, 2, 3) and x / 2 + z / 4 <= 1 for zi, z in enumerate(_ZS)] for xi, x in enumerate(_XS)])
                assert np.array_equal(got, want), (name, got)
                assert not (a["patch"][side + c["rays"].shape[0] // 2 - 5:side + half] >= 0)[:4].any()      # the far-off points but the last
            if name == "one_triangle":
                hyp = a["patch"][25:33] >= 0
                # on the hypotenuse an + bn == det; one ulp outside in x or in z the sum still ROUNDS to det (a tie to even) and the ray is
                # accepted -- "the sum rounded once" --; two ulps, or one in both, is outside
                assert list(hyp) == [True, True, True, True, True, False, False, False]
                assert ((an + bn) == det)[25:30].all() and a["patch"][half - 1] == -1 and c["rays"][half - 1, 0] == 1.75
            else:
                assert a["patch"][half - 1] == 0                                  # (1.75, 3.5): inside the quad, outside the triangle
        # parallel
        c, a = BY_NAME["parallel"], answer("parallel")
        o, d = tuple(c["rays"][:, k] for k in range(3)), tuple(c["rays"][:, 3 + k] for k in range(3))
        det = R.pair(c["table"][0], o, d)[4]
        assert (det[:5] == 0).all() and np.isnan(det[5:7]).all() and list(a["hit"]["patch"][:10]) == [-1] * 10
        assert list(a["hit"]["patch"][10:]) == [0, 0] and list(a["occluded"]) == [0] * 10 + [1, 1]
        # range
        a = answer("range")["hit"]["patch"]
        assert list(a >= 0) == [False, False, True, True, False, False, False, False, False, False, True, True, False, False, True, True]
        a = answer("default_range")["hit"]["patch"]
        assert list(a >= 0) == [False, False, False, True, True, True, False, False]
        assert H.fields(answer("default_range")["hit"]["raw"])["t"][3] == up(0.001)
        # ties
        a = answer("ties")
        assert list(a["hit"]["patch"]) == [0] * 6 + [2] * 6 and list(H.fields(a["hit"]["raw"])["object"]) == [0] * 6 + [1] * 6
        assert list(a["merge"]["patch"]) == [-1, -1, 0, 0, -1, 0, -1, -1, 2, 2, -1, 2]
        assert list(H.fields(a["merge"]["raw"])["object"]) == [2, 2, 0, 0, 2, 0, 2, 2, 1, 1, 2, 1]
        assert list(answer("ties_range")["merge"]["patch"]) == [-1, -1, 0, 0, 0, 0, -1, -1, 2, 2, 2, 2]
        # materials
        a = answer("materials")["hit"]
        f = H.fields(a["raw"])
        assert list(a["patch"]) == [0, 1, 2, 3, -1] * 2 and list(f["object"]) == [-1, 0, 2, 1, -1] * 2
        assert list(f["front_face"]) == [0, 0, 0, 1, 0, 1, 1, 1, 0, 0]
        # masks
        assert list(answer("masks")["hit"]["patch"]) == [0, 1, 0, -1, 0, 3, 3, 1, 0, -1]
        assert list(answer("mask_scalar")["hit"]["patch"]) == [1, 1, -1] and list(answer("mask_zero")["occluded"]) == [0, 0]
        # overflow
        c, a = BY_NAME["overflow"], answer("overflow")
        o, d = tuple(c["rays"][:, k] for k in range(3)), tuple(c["rays"][:, 3 + k] for k in range(3))
        dets = np.array([R.pair(p, o, d)[4] for p in c["table"]])
        assert np.isinf(dets).any() and (dets[2, 6] == 0) and c["rays"][6, 4] != 0 and (a["hit"]["patch"] >= 0).sum() >= 3
        assert ((np.abs(dets) > 0) & (np.abs(dets) < 2.3e-308)).any()              # a denormal det is a det
        # the soups
        for n in (63, 64, 65, 130):
            a = answer(f"soup{n}")["hit"]
            f, won = H.fields(a["raw"]), a["patch"][a["patch"] >= 0]
            kinds = {BY_NAME[f"soup{n}"]["table"][j]["kind"] for j in won}
            assert 3 * won.size >= a["patch"].size and np.unique(won).size >= 20 and kinds == {R.QUAD, R.TRIANGLE}, (n, won.size, np.unique(won).size)
            assert set(f["front_face"][a["patch"] >= 0]) == {0, 1}
        # the room: walls, the lamp, both boxes and all three spheres are seen
        a = answer("room")["merge"]
        f = H.fields(a["raw"])
        assert ROOM_LAMP in a["patch"] and (a["patch"] >= 6).any() and (a["patch"] >= 12).any() and (a["patch"] < 5).any()
        assert (a["patch"] < 0).sum() >= 6 and set(f["object"][a["patch"] < 0]) >= {0, 1, 2} and BY_NAME["room"]["rays"].shape[0] == 240
        assert BY_NAME["room"]["table"][ROOM_LAMP]["material"] == -1 and len(BY_NAME["room"]["table"]) == 18
        ls = lists(250)
        assert sorted(ls) == [1, 63, 64, 65, 255] and all(((v < 0) | (v >= 250)).any() for m, v in ls.items() if m > 1)
