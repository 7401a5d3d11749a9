"""The heterogeneous-media queries without a GPU: the restatement of include/tor_grid.h (tests/grid_restatement.py), which the GPU
suite holds the kernels to bit for bit, is checked here against hand-worked rows, against the header's invariances, against the
homogeneous march (a constant grid is a homogeneous medium in its box) and against additivity along the ray; the named inputs do
what their names say; the restated variants are told apart by named cases; the grid-masked homogeneous march is the sub-table's;
the entries are declared, bound and built and refuse what the header says, in its order; and the Python glue runs against a
recording stand-in for the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grid_inputs as I
import grid_restatement as R
import media_inputs as MI
import media_restatement as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
_answers = {}


def _answer(name):
    if name not in _answers:
        _answers[name] = I.answer(I.BY_NAME[name])
    return _answers[name]


def test_a_inputs_do_what_their_names_say():
    got = I.assert_coverage()
    print(got)
    assert set(I.NAMES) == {"g1", "g2", "g357", "g64x3x2", "dyadic4", "axis", "box_small", "box_large", "box_offset", "zeros", "all_zero",
                            "moving", "negative_radius", "wave16", "edges", "clamp", "guard"}
    assert sorted(len(v[(v >= 0) & (v < 257)]) for v in I.lists().values()) == [1, 63, 64, 65, 255] and len(I.BY_NAME["wave16"]["rays"]) == 257
    # the searches that found the committed rows still find rows: 2000 rays with t_min within two ulps of a plane of the dyadic grid
    # (measured: tn < t on 100 of them, the depth changes without the guard on 43; asserted: less than half of that), and the clamp's
    hit, changed, rays, tr = I.search_guard(2000, 11)
    print(f"guard search: tn < t on {len(hit)} of 2000 rays, the depth changes on {len(changed)}")
    assert len(hit) >= 40 and len(changed) >= 20
    assert len(I.search_clamp(1 << 15, 5)) >= 50


# ---- hand-worked rows -----------------------------------------------------------------------------------------------------------

def test_b_march_by_hand():
    """A ball of radius 2 at the origin, sigma 2; a 2 x 1 x 1 grid on [-1, 1]^3 with densities 0.5 (x < 0) and 1.5 (x >= 0): local
    extinction 1 and 3.  A ray along +x from x = -4 with |d| = 2: in the box from t = 1.5 to 2.5, the plane x = 0 at t = 2."""
    recs = [I._sphere((0, 0, 0), 2.0)]
    grid = R.make_grid(recs, [0], 0, np.asarray([0.5, 1.5]).reshape(2, 1, 1), [-1, -1, -1, 1, 1, 1])
    ray = [[-4.0, 0.5, -0.5, 2.0, 0, 0, 0.0]]
    m = R.march(recs, [0], [2.0], grid, ray * 6, [INF, 0.5, 1.0, 2.5, 4.0, 0.0])
    # depth 1 * 1 + 3 * 1 = 4; tau 0.5: half way through the first cell; tau 1.0 = the first step exactly: no collision there
    # (strict <), one at the plane in the second cell, rem = 0 < step; tau 2.5: 1.5 into the second cell's 3: half way
    assert m["status"].tolist() == [0, 1, 1, 1, 0, 1] and m["depth"].tolist() == [4.0, 0.5, 1.0, 2.5, 4.0, 0.0]
    assert m["t"].tolist() == [INF, 1.75, 2.0, 2.25, INF, 1.5] and m["cell"].tolist() == [-1, 0, 1, 1, -1, 0]
    assert m["rho"].tolist() == [0, 1.0, 3.0, 3.0, 0, 1.0] and m["active"].tolist() == [0, 1, 1, 1, 0, 1]
    # a range that ends inside the second cell, and one that starts there
    m = R.march(recs, [0], [2.0], grid, ray * 2, INF, [[0.0, 2.25], [2.25, INF]])
    assert m["depth"].tolist() == [2.5, 1.5] and m["t"].tolist() == [2.25, INF]
    # the medium's index is the active bit; the grid rides the centre: the same ray against a ball (and box) shifted by (10, 0, 0)
    recs3 = [I._sphere((0, 9, 9), 1.0), I._sphere((3, 3, 3), 1.0), I._sphere((10, 0, 0), 2.0)]
    g2 = R.make_grid(recs3, [0, 1, 2], 2, np.asarray([0.5, 1.5]).reshape(2, 1, 1), [-1, -1, -1, 1, 1, 1])
    m = R.march(recs3, [0, 1, 2], [9.0, 9.0, 2.0], g2, [[6.0, 0.5, -0.5, 2.0, 0, 0, 0.0]], 2.5)
    assert m["status"][0] == 1 and m["t"][0] == 2.25 and m["active"][0] == 4 and m["cell"][0] == 1
    # the default box is the bounding cube of the sphere: radius 2 -> [-2, 2]^3, h = 2; the sphere clips the corners
    g3 = R.make_grid(recs, [0], 0, np.ones((2, 2, 2)))
    assert g3["lo"] == [-2.0] * 3 and g3["hi"] == [2.0] * 3
    m = R.march(recs, [0], [2.0], g3, [[-4.0, 0.0, 0.0, 1.0, 0, 0, 0.0]], INF)
    assert m["depth"][0] == 8.0                                                     # the chord 4, sigma 2, density 1
    # refusals, nothing to meet, lists
    m = R.march(recs, [0], [2.0], grid, [[-4.0, 3.0, 0, 2.0, 0, 0, 0.0]] * 3, [1.0, np.nan, -1.0])
    assert m["status"].tolist() == [0, -1, -1] and m["t"].tolist() == [INF, 0.0, 0.0] and m["cell"].tolist() == [-1, -1, -1]
    into = {k: np.full(4, 7, dtype=v.dtype) for k, v in m.items()}
    got = R.march(recs, [0], [2.0], grid, ray * 4, [INF, 0.5, 1.0, 2.5], index=[2, -1, 9, 0], into=into)
    assert got["depth"].tolist() == [4.0, 7.0, 1.0, 7.0] and got["cell"].tolist() == [-1, 7, 1, 7]


def test_b_lookup_by_hand():
    recs = [I._sphere((1, 0, 0), 2.0)]
    dens = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    grid = R.make_grid(recs, [0], 0, dens, [-1, -1, -1, 1, 1, 1])
    pts = [[1.5, 0.0, 0.9, 0], [0.0, -1.0, -1.0, 0], [2.0, 0, 0, 0], [1.0, 1.5, 0, 0], [9.0, 0, 0, 0], [np.nan, 0, 0, 0], [1.0, 0.0, 0.0, 0]]
    cell, value = R.density(recs, [0], grid, pts)
    # q = (0.5, 0, 0.9): ix 1, iy floor(1 / (2/3)) = 1, iz floor(1.9 / 0.5) = 3;  q = lo: cell 0;  q.x = hi: outside;  in the sphere
    # outside the box;  outside both;  NaN;  the centre: ix 1, iy 1, iz 2
    assert cell.tolist() == [(1 * 3 + 1) * 4 + 3, 0, -1, -1, -1, -1, (1 * 3 + 1) * 4 + 2]
    assert value.tolist() == [19.0, 0.0, 0.0, 0.0, 0.0, 0.0, 18.0]


# ---- invariances ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["g357", "dyadic4", "wave16", "edges"])
def test_c_invariant_under_permutation_of_the_rays_and_split_lists(name):
    c = I.BY_NAME[name]
    want = _answer(name)
    n = len(c["rays"])
    perm = np.random.default_rng(3).permutation(n)
    got = R.march(c["recs"], c["objects"], c["sigma"], c["grid"], c["rays"][perm], c["tau"][perm],
                  None if c["t_range"] is None else c["t_range"][perm])
    assert not R.mismatches(got, {k: v[perm] for k, v in want.items()})
    half = I.answer(c, index=perm[: n // 2])
    assert not R.mismatches(I.answer(c, index=perm[n // 2:], into=half), want)


def _bound(c, sum_n, depth, rho_max, t_max=INF):
    """The bound of the two comparisons below.  depth = sum_j rho_j * ((tn_j - t_j) * len): per step three roundings (2^-53 relative
    each), per addition one on a partial sum <= depth: (3 + sum_n) 2^-53 relative for at most sum_n steps; the reference march has
    its own 3 + 1.  That is (sum_n + 7) 2^-53 <= (sum_n + 8) 2^-52.  In exact arithmetic the pieces tn_j - t_j telescope, because
    t_{j+1} IS tn_j; the guard breaks that by at most its correction t - tn per step, a few ulps of t (the planes are correctly
    rounded quotients of nearby operands): sum_n * ulp(t1) * len * rho_max absolute, with t1 <= min(t_far, t_max) standing for the
    clipped t1, t_far the largest |t| inside the ball."""
    rays = c["rays"]
    d = rays[:, 3:6]
    ln = np.sqrt((d * d).sum(axis=1))
    rec = c["recs"][int(c["objects"][c["grid"]["medium"]])]
    t_far = (np.sqrt(((rays[:, 0:3] - rec[1:4]) ** 2).sum(axis=1)) + 2.0 * abs(rec[9])) / ln
    return (sum_n + 8) * 2.0 ** -52 * depth + sum_n * np.spacing(np.minimum(t_far, t_max)) * ln * rho_max


def test_c_a_constant_grid_is_the_one_cell_grid():
    """Constant density c on n cells against the 1 x 1 x 1 grid of density c on the same box, tau = inf: the same depth within
    _bound (derived there).  Measured while the definition was made, 1.7 x 10^5 rays, origins within 3 R, sum_n <= 48: 6.0e-16
    relative; here the largest ratio to the bound is printed."""
    worst = 0.0
    for dims, seed in (((3, 5, 7), 1), ((16, 16, 16), 2), ((64, 3, 2), 3), ((2, 2, 2), 4)):
        recs = [I._sphere((0.3, -0.2, 0.1), 1.5)]
        box = [-1.0, -0.8, -0.9, 0.9, 1.1, 0.7]
        rays = MI._rays(seed, 300, centre=(0.3, -0.2, 0.1), reach=4.0, spread=1.5)
        fine = dict(recs=np.asarray(recs), objects=[0], grid=R.make_grid(recs, [0], 0, np.full(dims, 0.7), box), rays=rays)
        one = R.make_grid(recs, [0], 0, np.full((1, 1, 1), 0.7), box)
        a = R.march(recs, [0], [1.3], fine["grid"], rays, INF)
        b = R.march(recs, [0], [1.3], one, rays, INF)
        tol = _bound(fine, sum(dims), b["depth"], 1.3 * 0.7)
        err = np.abs(a["depth"] - b["depth"])
        assert (b["depth"] > 0).sum() >= 100 and (err <= tol).all(), (dims, float((err / np.maximum(tol, 1e-300)).max()))
        assert ((a["depth"] > 0) == (b["depth"] > 0)).all()
        worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
        # ... and the one-cell grid on the sphere's cube IS the homogeneous medium of sigma * c, to the bit at tau = inf with one step
        cube = R.make_grid(recs, [0], 0, np.full((1, 1, 1), 1.0))
        hom = MR.march(recs, [0], [1.3], rays, INF)
        g = R.march(recs, [0], [1.3], cube, rays, INF)
        inside = (hom["depth"] > 0)
        assert inside.sum() >= 100 and np.array_equal(MR.bits(g["depth"][inside]), MR.bits(hom["depth"][inside]))
    print(f"largest |depth - depth of the one-cell grid| / bound = {worst:.3f}")


def test_c_depth_is_additive_along_the_ray():
    """depth(a, b) + depth(b, c) against depth(a, c), tau = inf, within the bound of the constant-grid comparison: _bound with the
    grid's own sum_n = 3 + 5 + 7.  The two marches on the left take the steps of the whole march with the cell that holds b split in
    two: in units of 2^-53, sum_n + 3 for the whole and (sum_n + 1) + 3 and one addition for the split sum, 2 sum_n + 8 together,
    which is (sum_n + 4) 2^-52 and inside _bound's (sum_n + 8) 2^-52.  t1 is at most c, so the absolute term takes ulp(min(t_far, c))."""
    c = I.BY_NAME["g357"]
    n = len(c["rays"])
    g = np.random.default_rng(5)
    a_, c_ = np.zeros(n), g.uniform(3.0, 12.0, n)
    b_ = g.uniform(0.2, 0.8, n) * c_
    args = (c["recs"], c["objects"], c["sigma"], c["grid"], c["rays"], INF)
    whole = R.march(*args, np.stack([a_, c_], axis=1))["depth"]
    left = R.march(*args, np.stack([a_, b_], axis=1))["depth"]
    right = R.march(*args, np.stack([b_, c_], axis=1))["depth"]
    tol = _bound(c, 3 + 5 + 7, whole, float(c["sigma"][0]) * 2.25, t_max=c_)
    err = np.abs((left + right) - whole)
    print(f"additivity: largest error / bound = {float((err[tol > 0] / tol[tol > 0]).max()):.3f}")
    assert (whole > 0).sum() >= 100 and ((left > 0) & (right > 0)).sum() >= 30 and (err <= tol).all()


# ---- the restated variants: which inputs tell them apart ----------------------------------------------------------------------------

VARIANT_CASES = {"no_guard": "guard", "x_fastest": "g357", "no_entry_clamp": "box_small", "incremental_planes": "g357",
                 "rem_le_step": "edges", "no_collision_clamp": "clamp", "box_in_world": "moving"}


@pytest.mark.parametrize("variant", [v for v in R.VARIANTS if v != "tie_high_axis"])
def test_d_each_variant_is_told_apart_by_a_named_case(variant):
    assert set(VARIANT_CASES) | {"tie_high_axis"} == set(R.VARIANTS)
    c = I.BY_NAME[VARIANT_CASES[variant]]
    got, want = I.answer(c, variant=variant), _answer(c["name"])
    assert R.mismatches(got, want), variant
    if variant == "rem_le_step":
        row = I.EDGE_ROWS["tau_equals_step"]
        assert got["cell"][row] == (0 * 4 + 2) * 4 + 2 and want["cell"][row] == (1 * 4 + 2) * 4 + 2
    if variant == "x_fastest":
        assert (got["rho"] != want["rho"]).sum() >= 30
    if variant == "box_in_world":
        assert R.mismatches(I.answer(I.BY_NAME["box_offset"], variant=variant), _answer("box_offset"))
    if variant == "no_guard":
        assert got["depth"][0] != want["depth"][0]


def test_d_the_tie_order_cannot_be_observed():
    """tie_high_axis differs from the definition on NO row, and cannot: at an exact tie the two orders visit other cells in between,
    but every step between tied planes has tn - t == 0, so step == 0, D does not change and rem < 0 never holds (a collision needs
    rem < step); after the tied moves both walks stand in the same cell at the same t.  Leaving the grid in one of the tied moves
    ends either walk with the same D.  Shown here on every committed case and on the dyadic grid with a distinct density per cell,
    where every crossing of the diagonals is a tie and tau is finite.  The header fixes an order all the same: the kernel and the
    restatement must walk the same cells for their step counts and loads to be comparable."""
    for c in I.CASES:
        assert not R.mismatches(I.answer(c, variant="tie_high_axis"), _answer(c["name"])), c["name"]
    recs, dens, grid = I._dyadic_parts()
    d = I.BY_NAME["dyadic4"]
    rays = np.concatenate([d["rays"][:20]] * 6)
    tau = np.repeat([0.0, 0.3, 0.9, 1.7, 2.9, INF], 20)
    a = R.march(recs, [0], [1.0], grid, rays, tau)
    b = R.march(recs, [0], [1.0], grid, rays, tau, variant="tie_high_axis")
    assert (a["status"] == 1).sum() >= 60 and not R.mismatches(b, a)


def test_d_the_grid_masked_homogeneous_march_is_the_sub_tables():
    """march_with_grids (the table with the grid media removed, bits mapped back) against media_restatement's march on the FULL table
    with the grid media's boundary spheres moved out of every ray's way (has_m false): the same answers, bit for bit."""
    for name, grid_media in (("nested3", [1]), ("row64", [0, 5, 63]), ("two_overlap", [0, 1]), ("coincident", [2])):
        c = MI.BY_NAME[name]
        away = c["recs"].copy()
        for m in grid_media:
            away[int(c["objects"][m]), 1:7] = 1.0e6
        want = MR.march(away, c["objects"], c["sigma"], c["rays"], c["tau"], c["t_range"])
        got = R.march_with_grids(c["recs"], c["objects"], c["sigma"], grid_media, c["rays"], c["tau"], c["t_range"])
        assert not MR.march_mismatches(got, want), name
        full = MI.answer(c)
        assert MR.march_mismatches(got, full), name                                # ... and it is not the full table's
        for m in grid_media:
            assert not ((got["active"] >> np.uint64(m)) & np.uint64(1)).any()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_e_the_entries_are_declared_bound_and_built(tor):
    src = open(os.path.join(ROOT, "include", "tor_grid.h")).read()
    render = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    assert '#include "tor_grid.h"' in render and render.index('#include "tor_phase.h"') < render.index('#include "tor_grid.h"')
    L = tor.lib()
    assert tor.GRID_SYMBOLS == ["tor_scene_media_grid", "tor_media_grid_info", "tor_media_grid_march_device", "tor_media_grid_march_host",
                                "tor_media_grid_density_device", "tor_media_grid_density_host"]
    for name in tor.GRID_SYMBOLS:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_grid.h"
        assert hasattr(L, name) and getattr(L, name).argtypes == tor._grid_signatures()[name]
        assert name not in tor.EXPORTED_SYMBOLS and name not in tor._signatures() and name not in tor.MEDIA_SYMBOLS + tor.PHASE_SYMBOLS
    assert sorted(tor.GRID_SYMBOLS) == sorted(set(re.findall(r"TOR_API\s+int\s+(tor_\w+)\s*\(", src))) == sorted(tor._GRID_SIGNATURES)
    assert re.search(r"#define TOR_GRID_MAX_DIM 1024\b", src) and tor.GRID_MAX_DIM == R.GRID_MAX_DIM == 1024
    assert re.search(r"#define TOR_GRID_MAX_CELLS 16777216\b", src) and tor.GRID_MAX_CELLS == R.GRID_MAX_CELLS == 2 ** 24
    for name in ("set_media_grid", "media_grids", "media_grid_info", "march_media_grid", "media_density", "transmittance"):
        assert callable(getattr(tor.Context, name))
    assert issubclass(tor.GridMarch, tor.MediaMarch)
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert mk.count("tor_grid.hip") == 2 and mk.count("tor_grid.h ") == 1            # SRCS and ASM_SRCS; HDRS
    assert "-ffp-contract=off" in mk
    for word in ("(the guard)", "Termination", "In bounds", "nx + ny + nz", "rem < step", "ties to the lower axis", "OFFSETS FROM THE SPHERE'S CENTRE",
                 "Planes come from the index each time"):
        assert word in src, word
    hip = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "tor_grid.hip")).read().split("#include <hip/hip_runtime.h>")[1]
    for fn in ("log", "exp", "atan2", "pow", "sin", "cos"):                          # the library takes none
        assert not re.search(r"\b(__builtin_|std::|::)?" + fn + r"[a-z0-9]*\s*\(", hip), fn
    assert "__shared__" not in hip and "atomic" not in hip
    media = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "tor_media.hip")).read()
    assert "grid_mask" in media and "(grid_mask >> m) & 1ull" in media


def test_e_refusals_that_need_no_device(tor):
    """The checks that come before any device work, in the header's order; nothing is written.  (None of them reads the context, so a
    non-NULL pointer stands in for one; those that do -- no scene, no table, the medium, its grid, the grid's own -- are in the GPU
    suite.)"""
    L = tor.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.cast((C.c_char * 64)(), C.c_void_p)
    err = lambda: L.tor_last_error().decode()
    assert L.tor_scene_media_grid(None, 0, 1, 1, 1, None, p) == -1 and "tor_scene_media_grid: ctx is NULL" in err()
    assert L.tor_media_grid_info(None, 0, p, p, p) == -1 and "tor_media_grid_info: ctx or dims is NULL" in err()
    assert L.tor_media_grid_info(ctx, 0, None, p, p) == -1 and "ctx or dims is NULL" in err()
    for f, tail, name in ((L.tor_media_grid_march_device, (None,), "tor_media_grid_march_device"),
                          (L.tor_media_grid_march_host, (), "tor_media_grid_march_host")):
        assert f(None, 1, p, p, p, 0, None, 1, p, p, p, p, p, p, *tail) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, None, None, 0, None, -1, None, None, None, None, None, None, *tail) == -1 and "n_rays < 0" in err()
        assert f(ctx, 1, None, None, None, 0, None, -1, None, None, None, None, None, None, *tail) == -1 and "n_list < 0" in err()
        assert f(ctx, 2, None, None, None, 0, None, 1, None, None, None, None, None, None, *tail) == -1 and "without a list" in err()
        for hole in range(6):                                                        # rays, tau, status, t, depth, active
            a = [p] * 6
            a[hole] = None
            assert f(ctx, 1, a[0], None, a[1], -5, None, 1, a[2], a[3], a[4], a[5], None, None, *tail) == -1 and "NULL rays, tau" in err(), hole
    for f, tail, name in ((L.tor_media_grid_density_device, (None,), "tor_media_grid_density_device"),
                          (L.tor_media_grid_density_host, (), "tor_media_grid_density_host")):
        assert f(None, 1, p, 0, None, 1, p, p, *tail) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, 0, None, -1, None, None, *tail) == -1 and "n_rays < 0" in err()
        assert f(ctx, 1, None, 0, None, -1, None, None, *tail) == -1 and "n_list < 0" in err()
        assert f(ctx, 2, None, 0, None, 1, None, None, *tail) == -1 and "without a list" in err()
        for hole in range(3):                                                        # points, cell, density
            a = [p] * 3
            a[hole] = None
            assert f(ctx, 1, a[0], -5, None, 1, a[1], a[2], *tail) == -1 and "NULL points, cell or density" in err(), hole
    assert all(v == 0.0 for v in buf)


# ---- Python glue on a recording library -----------------------------------------------------------------------------------------------

class _Recorder:
    """A stand-in for the loaded library (the pattern of tests/test_media_query.py): every tor_* entry records (name, args) and
    returns 0; tor_media_grid_info also answers with `mask`, the word of the media that have a grid."""

    def __init__(self, note=b"media grid march: medium 1, 2x3x4", mask=0):
        self.calls, self.note, self.mask = [], note, mask

    def __getattr__(self, name):
        if not name.startswith("tor_"):
            raise AttributeError(name)
        if name == "tor_last_note":
            return lambda: self.note
        if name == "tor_last_error":
            return lambda: b""

        def entry(*args):
            self.calls.append((name, tuple((a.value or 0) if isinstance(a, C.c_void_p) else a for a in args)))
            if name == "tor_media_grid_info" and args[4] is not None and args[4].value:
                C.cast(args[4], C.POINTER(C.c_uint64))[0] = self.mask
            return 0
        return entry


def test_f_python_glue_on_a_recording_library(tor):
    ctx = object.__new__(tor.Context)
    ctx._h = C.c_void_p(16)
    saved = tor._lib
    rays = np.zeros((5, 7))
    try:
        rec = tor._lib = _Recorder()
        assert ctx.media_grids() == [] and rec.calls == []                          # no grid was ever set: the library is not asked
        ctx.set_media([3, 1], [0.5, 2.0])
        assert ctx.media_grids() == [] and len(rec.calls) == 1
        dens = np.arange(24.0).reshape(2, 3, 4)
        ctx.set_media_grid(1, dens)
        ctx.set_media_grid(0, dens[:, :, ::2], box=[-1, -2, -3, 1, 2, 3])            # not contiguous: copied
        (_, _), (n1, a1), (n2, a2) = rec.calls
        assert n1 == n2 == "tor_scene_media_grid" and a1[:5] == (16, 1, 2, 3, 4) and a1[5] is None and a1[6] == dens.ctypes.data
        assert a2[:5] == (16, 0, 2, 3, 2) and a2[5] not in (0, None) and a2[6] not in (0, dens.ctypes.data)
        for bad in (lambda: ctx.set_media_grid(0, np.zeros((2, 2))), lambda: ctx.set_media_grid(0, np.zeros((2, 0, 2))),
                    lambda: ctx.set_media_grid(0, dens, box=[0, 0, 0, 1, 1])):
            with pytest.raises(ValueError):
                bad()
        rec = tor._lib = _Recorder(mask=0b10)
        assert ctx.media_grids() == [1] and rec.calls[0][0] == "tor_media_grid_info"
        assert ctx.media_grid_info(1)[2] == 0b10
        # the march
        rec = tor._lib = _Recorder()
        m = ctx.march_media_grid(rays, 1.5, 1)
        (name, a), = rec.calls
        assert name == "tor_media_grid_march_host" and a[0] == 16 and a[1] == 5 and a[2] == rays.ctypes.data and a[3] == 0 and a[5] == 1
        assert a[6] == 0 and a[7] == 5 and len(a) == 14
        assert a[8:14] == (m.status.ctypes.data, m.t.ctypes.data, m.depth.ctypes.data, m.active.ctypes.data, m.rho.ctypes.data, m.cell.ctypes.data)
        assert isinstance(m, tor.MediaMarch) and m.medium == 1 and m.mode == "medium 1, 2x3x4" and m.cell.dtype == np.int32
        assert (m.cell == -1).all() and m.active.dtype == np.int64
        rec = tor._lib = _Recorder()
        again = ctx.march_media_grid(rays, np.arange(5.0), 1, t_range=np.zeros((5, 2)), index=[4, 0], out=m)
        (name, a), = rec.calls
        assert a[3] != 0 and a[6] not in (0, 16) and a[7] == 2 and again.cell is m.cell and again.t is m.t
        plain = tor.MediaMarch(*(np.zeros(5),) * 5, "")
        for bad in (lambda: ctx.march_media_grid(rays, np.zeros(4), 1), lambda: ctx.march_media_grid(rays, 1.0, 1, out=plain),
                    lambda: ctx.march_media_grid(rays, None, 1), lambda: ctx.march_media_grid(np.zeros((5, 6)), 1.0, 1)):
            with pytest.raises(ValueError):
                bad()
        # a GridMarch goes where a MediaMarch goes
        st = np.arange(20, dtype=np.uint64).reshape(5, 4)
        rec = tor._lib = _Recorder(b"media scatter: 2 media")
        ctx.scatter_media(rays, m, st, index=[1])
        ctx.sample_phase(rays, m, st, index=[1])
        ctx.phase(rays, m, np.ones((5, 7)))
        assert [n for n, _ in rec.calls] == ["tor_media_scatter_host", "tor_phase_sample_host", "tor_phase_eval_host"]
        assert rec.calls[0][1][3] == m.t.ctypes.data and rec.calls[0][1][4] == m.active.ctypes.data and rec.calls[2][1][3] == m.active.ctypes.data
        # the lookup
        rec = tor._lib = _Recorder(b"media grid density: medium 1, 2x3x4")
        pts = np.zeros((6, 4))
        cell, value = ctx.media_density(pts, 1, index=[5])
        (name, a), = rec.calls
        assert name == "tor_media_grid_density_host" and a[1] == 6 and a[2] == pts.ctypes.data and a[3] == 1 and a[5] == 1
        assert a[6:] == (cell.ctypes.data, value.ctypes.data) and cell.dtype == np.int32 and (cell == -1).all() and value.shape == (6,)
        rec = tor._lib = _Recorder()
        c2, v2 = ctx.media_density(pts, 1, out=(cell, value))
        assert c2 is cell and v2 is value and rec.calls[0][1][4] == 0
        for bad in (lambda: ctx.media_density(np.zeros((6, 3)), 1), lambda: ctx.media_density(pts, 1, out=(value, value))):
            with pytest.raises(ValueError):
                bad()
        # transmittance: the homogeneous depth, then each grid medium's, ascending
        rec = tor._lib = _Recorder(mask=0b11)
        tm = ctx.transmittance(np.zeros((3, 3)), np.ones((3, 3)), time=0.5)
        names = [n for n, _ in rec.calls]
        assert names == ["tor_media_march_host", "tor_media_grid_info", "tor_media_grid_march_host", "tor_media_grid_march_host"]
        assert [a[5] for n, a in rec.calls[2:]] == [0, 1] and (tm == 1.0).all()
        # removing a grid; a new table forgets them all, and then the library is not asked
        rec = tor._lib = _Recorder()
        ctx.set_media_grid(1, None)
        assert rec.calls[0][1][1:5] == (1, 0, 0, 0)
        ctx.set_media([3], [0.5])
        rec = tor._lib = _Recorder(mask=0b11)
        assert ctx.media_grids() == [] and rec.calls == []
        ctx.transmittance(np.zeros((3, 3)), np.ones((3, 3)))
        assert [n for n, _ in rec.calls] == ["tor_media_march_host"]                 # as before grids existed
    finally:
        tor._lib = saved
        ctx._h = C.c_void_p()


def test_f_bind_keeps_its_tables(tor):
    import types
    assert not set(tor.GRID_SYMBOLS) & (set(tor._SIGNATURES) | set(tor._PHASE_SIGNATURES))
    older = types.SimpleNamespace(tor_media_grid_info=types.SimpleNamespace(argtypes=None, restype=C.c_int))
    tor._bind(older, tor.GRID_SYMBOLS, skip_missing=True, table=tor._GRID_SIGNATURES)     # an A/B build older than the entries
    assert older.tor_media_grid_info.argtypes == tor._GRID_SIGNATURES["tor_media_grid_info"]
    with pytest.raises(AttributeError):
        tor._bind(older, tor.GRID_SYMBOLS, table=tor._GRID_SIGNATURES)


# ---- the statistics check holds for the definition ------------------------------------------------------------------------------------

def test_g_two_slabs_on_the_restatement(oracle):
    """4096 central rays through the unit ball of sigma 1 with the two-slab grid (density 0, then 2): every ray crosses one radius of
    each, depth 2, so the collision fraction is 1 - exp(-2) within 5 binomial standard errors (0.0267: grid_inputs.PHYSICS_TOL), and
    every collision lies in the dense slab."""
    c = I.physics_case()
    u, _ = MR.uniforms(oracle, MI.states(4096, 8), 1)
    m = R.march(c["recs"], c["objects"], c["sigma"], c["grid"], c["rays"], -np.log1p(-u[:, 0]))
    frac = float((m["status"] == 1).mean())
    print(f"collision fraction {frac:.4f}, expected {I.PHYSICS_P:.4f}: {(frac - I.PHYSICS_P) / (I.PHYSICS_TOL / 5):+.2f} standard errors")
    assert abs(I.PHYSICS_TOL - 0.0267) < 1e-4 and abs(frac - I.PHYSICS_P) <= I.PHYSICS_TOL
    assert (m["cell"][m["status"] == 1] == 1).all() and (m["rho"][m["status"] == 1] == 2.0).all()
    depth = R.march(c["recs"], c["objects"], c["sigma"], c["grid"], c["rays"], INF)["depth"]
    assert np.abs(depth - 2.0).max() <= 1e-12
