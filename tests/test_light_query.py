"""The direct-light sampling queries without a GPU: the entries exist and refuse what include/tor_lights.h says they refuse, and the
numpy restatement of the header's text (tests/light_restatement.py), which the GPU suite holds the kernels to bit for bit, is what
a direct-lighting integrator needs -- samples that land on the light, a density that integrates to the picked share, an unbiased
irradiance estimator, pick frequencies that follow the importance, a density query that agrees with the sampler in every bit and
exactly three draws per point.  Each check also shows that the shared inputs (tests/light_inputs.py) mean something."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import light_inputs as I
import light_restatement as LR
import nearest_restatement as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
STRATEGIES = (LR.BY_WEIGHT, LR.BY_SOLID_ANGLE)
_cases = {}


def _case(oracle, name, strategy):
    """Table, points, states and the restatement's sample: computed once, never changed."""
    key = (name, strategy)
    if key not in _cases:
        recs, lights, weights = I.table(name, oracle)
        pts = I.points(recs, lights)
        st = I.states(len(pts))
        _cases[key] = dict(recs=recs, lights=lights, weights=weights, pts=pts, st=st,
                           res=LR.sample(oracle, recs, lights, weights, pts, st, None, strategy))
    return _cases[key]


def test_the_entries_are_declared_bound_and_exported(tor):
    src = open(os.path.join(ROOT, "include", "tor_lights.h")).read()
    assert '#include "tor_lights.h"' in open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in tor.LIGHT_SYMBOLS:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_lights.h"
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
    assert sorted(tor.LIGHT_SYMBOLS) == sorted(set(re.findall(r"TOR_API\s+int\s+(tor_\w+)\s*\(", src)))
    assert (tor.LIGHT_BY_WEIGHT, tor.LIGHT_BY_SOLID_ANGLE) == (LR.BY_WEIGHT, LR.BY_SOLID_ANGLE)
    for method in ("set_lights", "sample_lights", "light_pdf", "trace_direct"):
        assert callable(getattr(tor.Context, method))
    mk = os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")
    assert open(mk).read().count("tor_lights.hip") == 2                   # SRCS and ASM_SRCS


def test_refusals_that_need_no_device(tor):
    """The checks that come before any device work: a NULL context is refused by every entry, nothing is touched."""
    L = tor.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.tor_scene_lights(None, 1, p, None) == -1 and b"tor_scene_lights" in L.tor_last_error()
    assert L.tor_light_sample_device(None, 1, p, p, None, 1, 1, p, p, p, None, None) == -1
    assert L.tor_light_sample_host(None, 1, p, p, None, 1, 1, p, p, p, None) == -1
    assert L.tor_light_pdf_device(None, 1, p, p, None, 1, 1, p, None) == -1
    assert L.tor_light_pdf_host(None, 1, p, p, None, 1, 1, p) == -1 and b"tor_light_pdf_host" in L.tor_last_error()
    assert all(v == 0.0 for v in buf)


def test_diffuse_objects_reads_the_material_kind(tor):
    recs, _, _ = I.table("three")
    assert tor.diffuse_objects(recs).tolist() == [True, False, True, True, True]
    assert tor.diffuse_objects(tor.Scene.from_records(recs)).tolist() == [True, False, True, True, True]


@pytest.mark.parametrize("name", I.TABLES)
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_the_inputs_take_every_branch(oracle, name, strategy):
    g = _case(oracle, name, strategy)
    pts, res, lights = g["pts"], g["res"], g["lights"]
    geo = LR.geometry(g["recs"], lights, pts)
    at = {k: len(pts) + v for k, v in I.SPECIAL.items()}
    assert len(pts) == 3 * 64 + 5
    assert geo["inside"][at["inside"], 0] and geo["d2"][at["inside"], 0] > 0
    assert geo["d2"][at["centre"], 0] == 0.0 and geo["inside"][at["centre"], 0]
    if name in ("one", "three"):
        assert geo["d2"][at["surface"], 0] == geo["R2"][0] and geo["inside"][at["surface"], 0]
    assert 0 < geo["m"][at["far"], 0] < 1e-12 and not geo["inside"][at["far"], 0]
    assert (geo["m"][at["overflow"]] == 0).all()
    assert np.isnan(geo["d2"][at["nan"]]).all() and geo["inside"][at["nan"]].all()
    if strategy == LR.BY_SOLID_ANGLE:                                     # every importance is 0: no sample, the state still advances
        assert res["light"][at["overflow"]] == -1 and res["pdf"][at["overflow"]] == 0 and (res["rays"][at["overflow"]] == 0).all()
    else:
        assert res["light"][at["overflow"]] >= 0 and np.isinf(res["pdf"][at["overflow"]])
    assert res["light"][at["nan"]] >= 0 and np.isnan(res["rays"][at["nan"], 3:6]).all() and np.isfinite(res["pdf"][at["nan"]])
    assert (res["light"][:-8] >= 0).all() and np.isin(res["light"][res["light"] >= 0], lights).all()
    if len(lights) > 1:
        assert len(np.unique(res["light"])) > min(len(lights), 8) // 2     # the picks spread over the table
    if name != "one":                                                     # a mover among the lights, and times outside its interval
        assert (g["recs"][lights, 0] == 1).any()


@pytest.mark.parametrize("name", I.TABLES)
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_samples_land_on_the_light(oracle, name, strategy):
    """Every sampled end point q = p + direction lies on its light: | |q - c| - R | <= 32 eps (|p| + |c| + dist), eps = 2^-53.

    The bound, from the operation count of include/tor_lights.h.  Relative to its own magnitude the centre c carries at most 4
    roundings, w = c - p one relative to |p| + |c|, d2 five and sd = sqrt(d2) three and a half; the axis a = w * (1 / sd) then
    about 6 eps per component, the frame vectors 4 more, e1 and e2 four each (k, sin2 twice, half for the square root, one for the
    sin / cos, one product), so dir is off by about 12 eps of a unit vector; t = sd * cos_t -+ sqrt(h) carries about 6 eps of
    dist, plus the rounding of h = R2 - d2 * sin2 -- about 4 eps R2 absolute, which the square root turns into a large error of t
    near a grazing sample but moves q along the tangent there: radially it costs 4 eps R2 / (2 R) = 2 eps R <= 2 eps (|p| + |c| +
    dist).  direction = dir * t and q = p + direction add one rounding each of dist and |p| + dist, the test's own |q - c| two
    of |p| + |c| + dist.  In all (12 + 6 + 1) eps dist + (1 + 1 + 2) eps (|p| + |c| + dist) + 4 eps |c| + 2 eps (...) <= 29 eps
    (|p| + |c| + dist): 32.  Measured on the restatement over the four tables and both strategies: worst 1.25 eps (|p| + |c| +
    dist) (table `many65`, by weight) -- the roundings rarely align."""
    g = _case(oracle, name, strategy)
    pts, res, recs = g["pts"], g["res"], g["recs"]
    ok = (res["light"] >= 0) & np.isfinite(res["rays"]).all(axis=1)
    assert ok.sum() >= len(pts) - 3                                       # all but the NaN point and the two without a finite sample
    worst = 0.0
    for i in np.nonzero(ok)[0]:
        rec = recs[res["light"][i]]
        c = np.array(N._centre(rec, pts[i, 3]), dtype=np.float64)
        q = pts[i, 0:3] + res["rays"][i, 3:6]
        dev = abs(np.sqrt(((q - c) ** 2).sum()) - abs(rec[9]))
        scale = np.sqrt((pts[i, 0:3] ** 2).sum()) + np.sqrt((c ** 2).sum()) + abs(res["dist"][i])
        worst = max(worst, dev / (EPS * scale))
        assert dev <= 32 * EPS * scale, (i, dev, scale)
        # ... and parameter 1.0 is `dist` away, within the roundings of the length
        assert abs(np.sqrt((res["rays"][i, 3:6] ** 2).sum()) - abs(res["dist"][i])) <= 32 * EPS * abs(res["dist"][i])
    print(f"{name} strategy {strategy}: worst | |q - c| - R | = {worst:.2f} eps (|p| + |c| + dist)")


@pytest.mark.parametrize("name", I.TABLES)
def test_the_density_integrates_to_the_picked_share(oracle, name):
    """pdf is constant over the cone, so its integral over the sampler's own strata -- the rings u1 in [k / K, (k + 1) / K), each
    of solid angle 2 pi (cos theta_k - cos theta_(k+1)) with the angles MEASURED on the sampled directions against the true axis --
    must be the picked share P.  The measured cosines carry about 16 eps absolute each (the 12 eps of dir above, the axis, the dot
    product), the sum telescopes to the first and the last, and P = pdf * 2 pi * (1 - cos theta_max) divides that by m: the
    tolerance is 64 eps / m relative (points with m >= 1e-6; at the far point the cancellation this test would suffer is what the
    header's m avoids)."""
    g = _case(oracle, name, LR.BY_SOLID_ANGLE)
    L = oracle.lib()
    pts, res, lights, recs = g["pts"], g["res"], g["lights"], g["recs"]
    geo = LR.geometry(recs, lights, pts)
    K = 16
    checked = 0
    for i in np.nonzero(res["light"] >= 0)[0][::7]:
        j = int(res["pick"][i])
        m, d2 = geo["m"][i, j], geo["d2"][i, j]
        if not (m >= 1e-6) or geo["inside"][i, j] or not np.isfinite(d2):
            continue
        w = np.array([geo["wx"][i, j], geo["wy"][i, j], geo["wz"][i, j]])
        axis = w / np.sqrt((w ** 2).sum())
        u1 = np.arange(K + 1) / K
        one = np.ones(K + 1)
        dirs, _ = LR.cone(L, w[0] * one, w[1] * one, w[2] * one, d2 * one, geo["R2"][j] * one, m * one, np.zeros(K + 1, dtype=bool),
                          u1, 0.37 * one)
        cos = dirs[0] * axis[0] + dirs[1] * axis[1] + dirs[2] * axis[2]
        assert (np.diff(cos) < 0).all()                                   # the rings nest
        integral = sum(res["pdf"][i] * RR_TWO_PI * (cos[k] - cos[k + 1]) for k in range(K))
        assert abs(integral - res["P"][i]) <= (64 * EPS / m) * res["P"][i], (i, integral, res["P"][i])
        checked += 1
    assert checked >= 5


RR_TWO_PI = 2.0 * 3.141592653589793


def test_the_irradiance_estimator_is_unbiased(oracle):
    """One unoccluded spherical light of radius R at distance d above a receiver whose normal points at its centre: the mean of
    cos / pdf over N samples is the sphere's form factor pi R^2 / d^2, within 5 standard errors of the samples' own variance.
    N = 4096, one fixed seed: 12288 draws, well under a second."""
    R, d, n = 0.75, 3.0, 4096
    recs = np.array([I._sphere((0.0, d, 0.0), R)])
    pts = np.zeros((n, 4))
    res = LR.sample(oracle, recs, [0], None, pts, I.states(n, 0xBEEF), None, LR.BY_SOLID_ANGLE)
    assert (res["light"] == 0).all() and (res["P"] == 1.0).all()
    cos = res["rays"][:, 4] / np.sqrt((res["rays"][:, 3:6] ** 2).sum(axis=1))      # the normal is +y
    est = cos / res["pdf"]
    mean, se = est.mean(), est.std(ddof=1) / np.sqrt(n)
    want = np.pi * R * R / (d * d)
    print(f"irradiance: mean {mean:.6f}, want {want:.6f}, standard error {se:.2e}")
    assert se > 0 and abs(mean - want) <= 5 * se


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_pick_frequencies_follow_the_importance(oracle, strategy):
    """The three-light table from one point, N = 4096 states: light j is picked with frequency I_j / T within 5 binomial standard
    errors, and the light of weight 0 never."""
    recs, lights, weights = I.table("three")
    n = 4096
    pts = np.tile(np.array([[0.5, 0.5, 0.25, 0.6]]), (n, 1))
    res = LR.sample(oracle, recs, lights, weights, pts, I.states(n, 0xF00D), None, strategy)
    geo = LR.geometry(recs, lights, pts[:1])
    imp, _, T = LR.importances(geo, weights, strategy)
    share = imp[0] / T[0]
    assert share[2] == 0 and 0.05 < share[0] < 0.95
    for j in range(3):
        freq = (res["pick"] == j).mean()
        assert abs(freq - share[j]) <= 5 * np.sqrt(share[j] * (1 - share[j]) / n), (j, freq, share[j])
    assert not (res["pick"] == 2).any() and not (res["light"] == lights[2]).any()
    assert np.array_equal(res["P"], share[res["pick"]])


@pytest.mark.parametrize("name", I.TABLES)
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_sample_and_pdf_agree_in_every_bit(oracle, name, strategy):
    g = _case(oracle, name, strategy)
    res = g["res"]
    back = LR.pdf(g["recs"], g["lights"], g["weights"], g["pts"], res["light"], None, strategy)
    assert np.array_equal(back.view(np.uint64), res["pdf"].view(np.uint64))
    assert (back[res["light"] < 0] == 0).all() and (back[res["light"] >= 0] > 0).all()
    # an object that is no light, and the light of weight 0, have density 0
    other = np.zeros(len(g["pts"]), dtype=np.int32)
    assert (LR.pdf(g["recs"], g["lights"], g["weights"], g["pts"], other, None, strategy) == 0).all()
    if name == "three":
        dark = np.full(len(g["pts"]), g["lights"][2], dtype=np.int32)
        assert (LR.pdf(g["recs"], g["lights"], g["weights"], g["pts"], dark, None, strategy) == 0).all()


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_every_listed_point_draws_exactly_three(oracle, strategy):
    g = _case(oracle, "three", strategy)
    L = oracle.lib()
    n = len(g["pts"])
    index = np.array([0, 5, n - 4, n - 1, -3, n + 7, 64], dtype=np.int32)   # the point without a sample among them, two entries skipped
    res = LR.sample(oracle, g["recs"], g["lights"], g["weights"], g["pts"], g["st"], index, strategy)
    want = g["st"].copy()
    for i in (0, 5, n - 4, n - 1, 64):
        for _ in range(3):
            L.oracle_rng_next(want[i].ctypes.data_as(C.POINTER(C.c_uint64)))
    assert np.array_equal(res["states"], want)
    listed = np.zeros(n, dtype=bool)
    listed[[0, 5, n - 4, n - 1, 64]] = True
    assert (res["light"][~listed] == -1).all() and (res["rays"][~listed] == 0).all() and (res["pdf"][~listed] == 0).all()
    if strategy == LR.BY_SOLID_ANGLE:
        assert res["light"][n - 4] == -1                                  # no sample, three draws all the same
    full = _case(oracle, "three", strategy)["res"]
    for k in ("rays", "pdf", "light", "dist"):
        assert np.array_equal(res[k][listed], full[k][listed], equal_nan=(k in ("rays", "dist")))
