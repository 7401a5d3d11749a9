"""Inputs of the photon-map tests (tests/test_photon_query.py on the CPU, tests/test_gpu_photon_query.py on the GPU): small synthetic
maps and queries from fixed seeds, one case per regime of include/tor_photons.h.  A case is a dict
    name, R, position, power, direction (or None), index (the build's list or None), points, normals (or None), radius (or None)
and CASES holds them all.  check_coverage() asserts on the CPU, through tests/photon_restatement.py alone, that every class of
event the cases were made for is present; its floors are half of what the committed cases give, so that an edit which empties a
class fails there and not silently."""
import numpy as np

import photon_restatement as pr

R = 0.25
H = float(pr.cell_size(R))
TWO30 = float(2 ** 30)


def _unit_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.sqrt((d * d).sum(axis=1))[:, None]


def _case(name, position, power, direction, points, normals=None, radius=None, index=None, r=R):
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    return {"name": name, "R": r, "position": f(position).reshape(-1, 3), "power": f(power).reshape(-1, 3),
            "direction": None if direction is None else f(direction).reshape(-1, 3), "index": index,
            "points": f(points).reshape(-1, 3), "normals": None if normals is None else f(normals).reshape(-1, 3),
            "radius": f(radius)}


def dense(n, seed, side=5.0, n_points=96):
    """n photons in a box of `side` cells around the origin (negative coordinates on every axis: floor is not truncation), a
    bucket table of the smallest sizes: neighbour cells share buckets, and the cells beyond the 27 are strangers in them."""
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) - 0.5) * side * H
    pw = rng.random((n, 3)) * 0.9
    dr = _unit_dirs(rng, n)
    pts = (rng.random((n_points, 3)) - 0.5) * (side + 1.0) * H
    nrm = _unit_dirs(rng, n_points)
    return _case(f"dense{n}", pos, pw, dr, pts, nrm)


def one_cell(n=300, seed=11):
    """Every photon in the one cell (3, -2, 5): a bucket far above a wave's width."""
    rng = np.random.default_rng(seed)
    corner = np.array([3.0, -2.0, 5.0]) * H
    pos = corner + (0.05 + 0.9 * rng.random((n, 3))) * H
    pw = rng.random((n, 3)) * 0.5
    pts = corner + (rng.random((64, 3)) * 3.0 - 1.0) * H
    return _case("one_cell", pos, pw, None, pts)


def sparse(n=5000, seed=12):
    """Photons spread over 200^3 cells: most buckets are empty, almost every photon has its cell to itself."""
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) - 0.5) * 200.0 * H
    pw = rng.random((n, 3))
    dr = _unit_dirs(rng, n)
    near = pos[rng.integers(0, n, 192)] + (rng.random((192, 3)) - 0.5) * 0.8 * R
    far = (rng.random((64, 3)) - 0.5) * 200.0 * H
    pts = np.concatenate([near, far])
    return _case("sparse", pos, pw, dr, pts, np.tile(np.array([0.0, 0.0, 1.0]), (len(pts), 1)))


def faces(seed=13):
    """Positions ON cell faces (multiples of h, both signs, zero and -0.0) and half a cell off them, queried from the faces and
    from just beside them."""
    rng = np.random.default_rng(seed)
    k = np.arange(-3, 4, dtype=np.float64)
    lattice = np.array([(a, b, c) for a in k for b in (-1.0, 0.0, 1.0) for c in (-2.0, 0.0)]) * H
    pos = np.concatenate([lattice, lattice + 0.5 * H, np.array([[-0.0, -0.0, -0.0], [-0.3 * H, -0.3 * H, -0.3 * H]])])
    pw = np.full((len(pos), 3), 0.25)
    pts = np.concatenate([lattice[::3], lattice[::3] + np.array([np.nextafter(0.0, 1.0), 0.0, 0.0]),
                          lattice[1::3] - 0.9 * R * np.array([1.0, 0.0, 0.0]), (rng.random((32, 3)) - 0.5) * 7.0 * H])
    return _case("faces", pos, pw, None, pts)


def range_edge():
    """Cells at +-2^30 (stored) and just beyond (dropped); queries whose own cell is out of range but which lie within R of a
    photon stored in the outermost cell, and queries so far out that nothing is converted."""
    e = TWO30
    pos = np.array([[e * H, 0.0, 0.0], [-e * H, 0.0, 0.0], [(e + 0.9) * H, 0.1, 0.1], [0.1, -(e - 0.1) * H, 0.1],
                    [(e + 1.5) * H, 0.0, 0.0], [0.0, 0.0, -(e + 0.5) * H], [0.0, (e + 2.5) * H, 0.0], [0.1, 0.1, (e + 0.5) * H]])
    pw = np.full((len(pos), 3), 0.5)
    pts = np.array([[(e + 1.2) * H, 0.1, 0.1], [(e + 0.95) * H, 0.1, 0.1], [e * H, 0.0, 0.0], [-(e + 0.2) * H, 0.0, 0.0],
                    [0.1, -(e + 0.05) * H, 0.1], [0.1, 0.1, (e + 1.1) * H], [(e + 2.5) * H, 0.0, 0.0], [(e + 4.0) * H, 0.0, 0.0],
                    [1e300, 0.0, 0.0], [np.inf, 0.0, 0.0], [0.0, -np.inf, 0.0], [0.0, 0.0, np.nan]])
    return _case("range_edge", pos, pw, None, pts)


def collide40(seed=14):
    """40 photons in 40 far-apart cells of a 128-bucket table: cells that share a bucket are strangers to each other."""
    rng = np.random.default_rng(seed)
    cell = rng.integers(-50000, 50000, (40, 3)).astype(np.float64)
    pos = (cell + 0.5) * H
    pw = np.full((40, 3), 0.75)
    pts = np.concatenate([pos + 0.3 * R, pos - np.array([0.0, 0.6 * R, 0.0])])
    return _case("collide40", pos, pw, None, pts)


def specials():
    """Powers and queries at the comparisons' edges, around one photon cluster at (0.125, 0.125, 0.125)."""
    c = np.array([0.125, 0.125, 0.125])
    down = np.array([0.0, 0.0, -1.0])
    pos = [c] * 9 + [c + 0.01] * 4
    pw = [[0.5, 0.5, 0.5], [3.0, 100.0, 0.3],                     # power * w above max_value
          [-0.0, 0.0, -0.0], [2.0 ** -38, 2.0 ** -37, 1.5 * 2.0 ** -37],   # below the quantum, the tie, just above it
          [np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -1e-300], [0.1, -np.inf, 0.1],   # dropped
          [1e300, 1e-300, 127.0],
          [0.25, 0.25, 0.25], [0.25, 0.25, 0.25], [0.25, 0.25, 0.25], [0.25, 0.25, 0.25]]
    dr = [down] * 9 + [down, [0.0, 0.0, 1.0], [np.nan, 0.0, -1.0], [1.0, 0.0, 0.0]]    # (the NaN direction is dropped)
    inside = np.nextafter(0.25, 0.0)
    pts = [c + [0.25, 0.0, 0.0], c + [inside, 0.0, 0.0], c - [0.0, 0.25, 0.0], c - [0.0, inside, 0.0], c, c + 0.05, c + 0.05,
           c + 0.05, c + 0.05, c + 0.05, c + 0.05, c + 0.05, c + 0.05, c + [0.1, 0.1, 0.1], c + [np.nan, 0.0, 0.0],
           c + [0.0, np.inf, 0.0], c + 0.2]
    up = [0.0, 0.0, 1.0]
    nrm = [up, up, up, up, up, up, up, up, up, up, up, [1.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [0.0, 1.0, 1e-300], up, up, [0.0, 0.0, -1.0]]
    rad = [R, R, R, R, R, 0.0, R, 2.0 * R, np.inf, -1.0, np.nan, R, R, 0.9 * R, R, R, R]
    return _case("specials", pos, pw, dr, pts, nrm, rad)


def listed(seed=15):
    """A build through a list: repeated entries (stored again), entries outside [0, n) (skipped), photons left out."""
    rng = np.random.default_rng(seed)
    n = 80
    pos = (rng.random((n, 3)) - 0.5) * 3.0 * H
    pw = rng.random((n, 3)) * 0.5
    dr = _unit_dirs(rng, n)
    index = np.concatenate([rng.integers(0, n, 70), [-1, n, n + 5, -(2 ** 31), 2 ** 31 - 1], [3, 3, 3]]).astype(np.int32)
    pts = (rng.random((70, 3)) - 0.5) * 4.0 * H
    return _case("listed", pos, pw, dr, pts, _unit_dirs(rng, 70), rng.random(70) * 1.5 * R, index=index)


CASES = [dense(0, 1), dense(1, 2, side=1.0), dense(63, 3), dense(64, 4), dense(65, 5), dense(257, 6), one_cell(), sparse(), faces(),
         range_edge(), collide40(), specials(), listed()]
BY_NAME = {c["name"]: c for c in CASES}


def stored(case, scale=1.0):
    return pr.store(case["position"], case["power"] * scale, case["direction"], case["R"], case["index"])


def check_coverage():
    """The classes of events the cases were made for, counted through the restatement; returns the counts."""
    got = {"shared": 0, "strangers": 0, "twice": 0, "on_boundary": 0, "just_inside": 0, "clamped": 0, "no_radius": 0, "flat_normal": 0,
           "dropped": 0, "edge_cells": 0, "outside_query_hits": 0, "negative_cells": 0, "face_photons": 0, "over_max": 0,
           "sub_quantum": 0, "big_bucket": 0, "empty_buckets": 0.0}
    for case in CASES:
        m = stored(case)
        ref, st = pr.walk(m, case["points"], case["normals"], case["radius"])
        assert not pr.mismatches(ref, pr.agree(m, case["points"], case["normals"], case["radius"])), case["name"]   # the walk IS exact
        for k in ("shared", "strangers", "twice"):
            got[k] += int((st[k] > 0).sum())
        got["dropped"] += m["dropped"]
        got["edge_cells"] += int((np.abs(m["cell"]) == pr.CELL_MAX).any(axis=1).sum())
        got["negative_cells"] += int((m["cell"] < 0).any(axis=1).sum())
        with np.errstate(invalid="ignore"):
            got["face_photons"] += int((m["position"] / m["h"] == np.floor(m["position"] / m["h"])).all(axis=1).sum())
        got["big_bucket"] = max(got["big_bucket"], m["largest"])
        if len(m["bucket"]) >= 1000:      # (of a map worth the name: a table for one photon is empty anyway)
            got["empty_buckets"] = max(got["empty_buckets"], 1.0 - len(set(m["bucket"].tolist())) / m["n_buckets"])
        _, own = pr.query_cells(case["points"], m["h"])
        with np.errstate(invalid="ignore"):
            out_of_range = (np.abs(pr.cells(case["points"], m["h"])) > pr.CELL_MAX).any(axis=1)
        got["outside_query_hits"] += int((out_of_range & (ref["count"] > 0)).sum())
        for rows, acc, a, d2, r2 in pr._pairs(m, case["points"], None, case["radius"], "constant", 1.0, chunk=1 << 20):
            got["on_boundary"] += int((d2 == r2[:, None]).sum())
            got["just_inside"] += int((acc & (d2 >= np.nextafter(np.nextafter(r2, 0.0), 0.0)[:, None])).sum())
            got["over_max"] += int((acc[..., None] & (m["power"][None] > 1.0)).sum())
            got["sub_quantum"] += int((acc[..., None] & (m["power"][None] > 0.0) & (m["power"][None] <= 2.0 ** -37)).sum())
        if case["radius"] is not None:
            with np.errstate(invalid="ignore"):
                got["clamped"] += int((case["radius"] > case["R"]).sum())
                got["no_radius"] += int((~(case["radius"] >= 0.0)).sum() + (case["radius"] == 0.0).sum())
        if case["normals"] is not None and m["direction"] is not None and len(m["position"]):
            dn = (m["direction"][None, :, :] * case["normals"][:, None, :])
            with np.errstate(invalid="ignore"):
                got["flat_normal"] += int((((dn[..., 0] + dn[..., 1]) + dn[..., 2]) == 0.0).sum())
    return got


# half of what the committed cases give (check_coverage() on this file as committed; test_photon_query.py prints the counts)
COVERAGE_FLOORS = {
    "shared": 203,             # queries with two distinct visited cells in one bucket (406)
    "strangers": 246,          # queries that meet a photon of a cell beyond their 27 in a walked bucket, within 4 R (493)
    "twice": 41,               # queries with an accepted photon whose bucket is walked for more than one cell (83)
    "on_boundary": 7,          # (query, photon) pairs with d2 == r2: rejected (15)
    "just_inside": 2,          # accepted pairs within two ulps of r2 (5)
    "clamped": 15,             # per-point radii above R (31)
    "no_radius": 1,            # per-point radii 0, negative or NaN (3)
    "flat_normal": 11,         # (query, photon) pairs with dir . n == 0: rejected (22)
    "dropped": 4,              # photons dropped: NaN, infinite, negative, cell beyond 2^30 (8)
    "edge_cells": 2,           # photons stored in a cell at +-2^30 (5)
    "outside_query_hits": 2,   # queries whose own cell is out of range and that accept a photon (4)
    "negative_cells": 2616,    # photons with a negative cell coordinate (5232)
    "face_photons": 22,        # photons on cell faces on every axis (45)
    "over_max": 16,            # accepted (pair, channel)s whose power is above max_value = 1 (32)
    "sub_quantum": 12,         # accepted (pair, channel)s with 0 < power <= 2^-37 (24)
    "big_bucket": 150,         # the largest bucket of any case (300: far above a wave's 64 lanes)
    "empty_buckets": 0.36,     # the share of empty buckets of the largest map (0.74)
}


def assert_coverage():
    got = check_coverage()
    short = {k: (got[k], floor) for k, floor in COVERAGE_FLOORS.items() if not got[k] >= floor}
    assert not short, f"classes of events the photon inputs no longer hold (got, floor): {short}"
    return got
