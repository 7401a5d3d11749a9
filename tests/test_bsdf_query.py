"""The BSDF query without a GPU: the numpy restatement of include/tor_bsdf.h (tests/bsdf_restatement.py), which the GPU suite holds
the kernel to bit for bit, IS the density of the reference's scatter.  The only source of samples is bounce_restatement.scatter over
the CPU oracle's generator -- the restated Material.scatter that tests/test_bounce_query.py ties to the oracle's sample sums.

(a) histograms of the scattered directions against bin integrals of the restated density, four fuzz values x two incidences;
(b) the density integrates to 1 over the sphere, its gated integral is the share of rays the scatter did not absorb; (c) the same
for Lambertian, and the mean cosine 2/3; (d) value == albedo * pdf exactly; (e) kind and the zero cases of every named item;
(f) the round trip: a SCATTERED Metal ray has pdf > 0, an ABSORBED one pdf == 0; (g) the entries are declared, bound and exported,
and refuse what the header says they refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bounce_restatement as BR
import bsdf_inputs as I
import bsdf_restatement as R
import light_inputs as LI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.array([0.0, 0.0, 1.0])
INCIDENCES = {"slant": np.array([0.6, 0.0, -0.8]), "grazing": np.array([0.96, 0.0, -0.28])}
FUZZES = {0.05: I.F005, 0.3: I.F03, 0.9: I.F09, 1.0: I.F1}
N_SAMPLES = 20000          # 37 us per restated scatter: under a second per case
N_T, N_PHI = 8, 16         # 128 solid-angle bins in polar coordinates about the lobe's axis
MIN_EXPECTED = 25.0        # bins expected to hold fewer samples are pooled: the 5 sigma bound reads the binomial as a normal
_samples, _masses = {}, {}


def _frame(axis):
    """An orthonormal frame (e1, e2, a) about the direction `axis`."""
    a = axis / np.sqrt((axis * axis).sum())
    t = np.array([1.0, 0.0, 0.0]) if abs(a[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(a, t)
    e1 /= np.sqrt((e1 * e1).sum())
    return e1, np.cross(a, e1), a


def _axis_and_reach(obj, d_in):
    """The axis of the polar bins and the largest polar angle they cover: the reflected direction and asin(f / |r|) for a Metal
    (pi where the ball holds or touches the origin), the normal and pi / 2 for a Lambertian."""
    recs = I.scene()
    if recs[obj, 10] == I.LAMB:
        return Z, np.pi / 2.0
    r = I._reflect(d_in, Z)
    s = abs(recs[obj, 14]) / np.sqrt((r * r).sum())
    return r, (np.arcsin(s) if s < 1.0 else np.pi)


def _scattered(oracle, obj, d_in, seed):
    """N_SAMPLES draws of the restated scatter for one (incoming direction, record): (directions, status); computed once."""
    key = (obj, tuple(d_in), seed)
    if key not in _samples:
        n = N_SAMPLES
        rays_in, raw, _ = I.pack([obj] * n, np.tile(Z, (n, 1)), np.tile(d_in, (n, 1)), np.zeros((n, 3)))
        res = BR.scatter(oracle, I.scene(), rays_in, raw, LI.states(n, seed))
        _samples[key] = (res["rays"][:, 3:6].copy(), res["status"].copy())
    return _samples[key]


def _density(obj, d_in, w, gated=True):
    """The restated density at the unit directions w: through evaluate() (the gate, the kinds), or the bare Metal lobe."""
    n = len(w)
    if not gated:
        return R.metal_density(w, np.tile(d_in, (n, 1)), np.tile(Z, (n, 1)), np.full(n, I.scene()[obj, 14]))
    rays_in, raw, rays_out = I.pack([obj] * n, np.tile(Z, (n, 1)), np.tile(d_in, (n, 1)), w)
    res = R.evaluate(I.scene(), rays_in, raw, rays_out)
    assert (res["kind"] == R.DENSITY).all()
    return res["pdf"]


def _bin_masses(obj, d_in, sub, gated=True):
    """The integral of the density over each of the N_T x N_PHI polar bins about the axis (bin edges uniform in theta and phi):
    the midpoint rule on sub x sub cells per bin with the solid-angle element sin(theta), the cells uniform in phi and in v,
    theta = reach (1 - (1 - v)^2) -- the Metal density falls to 0 like a square root at the lobe's rim theta = reach, which the
    substitution turns into a parabola."""
    axis, reach = _axis_and_reach(obj, d_in)
    e1, e2, a = _frame(axis)
    edges = 1.0 - np.sqrt(1.0 - np.arange(N_T + 1) / N_T)                 # the bins' edges in v
    v = (edges[:-1, None] + (np.arange(sub) + 0.5)[None, :] * ((edges[1:] - edges[:-1]) / sub)[:, None]).reshape(-1)
    dv = np.repeat((edges[1:] - edges[:-1]) / sub, sub)
    th, dth = reach * (1.0 - (1.0 - v) ** 2), 2.0 * reach * (1.0 - v) * dv
    nt, nphi = N_T * sub, N_PHI * sub
    ph = (np.arange(nphi) + 0.5) * (2.0 * np.pi / nphi)
    T, P = np.meshgrid(th, ph, indexing="ij")
    w = (np.cos(T)[..., None] * a + np.sin(T)[..., None] * (np.cos(P)[..., None] * e1 + np.sin(P)[..., None] * e2)).reshape(-1, 3)
    w = w / np.sqrt((w * w).sum(axis=1))[:, None]
    cell = _density(obj, d_in, w, gated).reshape(nt, nphi) * np.sin(T) * dth[:, None] * (2.0 * np.pi / nphi)
    return cell.reshape(N_T, sub, N_PHI, sub).sum(axis=(1, 3))


def _converged_masses(obj, d_in, gated=True):
    """_bin_masses, the step halved until no bin moves by more than a tenth of its standard error at N_SAMPLES."""
    key = (obj, tuple(d_in), gated)
    if key not in _masses:
        sub, m = 8, _bin_masses(obj, d_in, 8, gated)
        while True:
            sub *= 2
            m2 = _bin_masses(obj, d_in, sub, gated)
            se = np.sqrt(np.maximum(m2, 1.0 / N_SAMPLES) / N_SAMPLES)
            done = (np.abs(m2 - m) <= 0.1 * se).all()
            m = m2
            if done or sub >= 128:
                assert done, "the bin integrals did not settle"
                break
        _masses[key] = m
    return _masses[key]


def _bin_counts(obj, d_in, dirs):
    """The samples per polar bin (N_T, N_PHI) and the number that fall outside the bins' reach."""
    axis, reach = _axis_and_reach(obj, d_in)
    e1, e2, a = _frame(axis)
    w = dirs / np.sqrt((dirs * dirs).sum(axis=1))[:, None]
    theta = np.arctan2(np.sqrt((w @ e1) ** 2 + (w @ e2) ** 2), w @ a)
    phi = np.mod(np.arctan2(w @ e2, w @ e1), 2.0 * np.pi)
    it, ip = np.floor(theta / reach * N_T).astype(int), np.minimum(np.floor(phi / (2.0 * np.pi) * N_PHI).astype(int), N_PHI - 1)
    inside = it < N_T
    counts = np.zeros((N_T, N_PHI))
    np.add.at(counts, (it[inside], ip[inside]), 1.0)
    return counts, int((~inside).sum())


def _worst_bin(counts, masses, absorbed):
    """The largest |frequency - integral| in standard errors sqrt(p (1 - p) / N) over the bins expected to hold MIN_EXPECTED
    samples, the pool of the others, and the absorbed share against 1 - the gated integral."""
    n = N_SAMPLES
    big = masses * n >= MIN_EXPECTED
    p = np.concatenate([masses[big], [masses[~big].sum()], [max(1.0 - masses.sum(), 0.0)]])
    k = np.concatenate([counts[big], [counts[~big].sum()], [absorbed]])
    se = np.sqrt(np.maximum(p * (1.0 - p), 1.0 / n) / n)              # (a pool or an absorbed share of 0: one sample is one sigma)
    assert k.sum() == n and len(p) <= 130
    return float((np.abs(k / n - p) / se).max())


@pytest.mark.parametrize("incidence", sorted(INCIDENCES))
@pytest.mark.parametrize("fuzz", sorted(FUZZES))
def test_a_histogram_of_the_scatter_against_the_density(oracle, fuzz, incidence):
    """Every bin's frequency lies within 5 standard errors of the bin integral of the restated density (128 bins: a false alarm
    below 1e-4 per case; the seeds are fixed).  The absorbed rays are one more bin, against 1 - the gated integral."""
    obj, d_in = FUZZES[fuzz], INCIDENCES[incidence]
    dirs, status = _scattered(oracle, obj, d_in, 0xA000 + obj)
    kept = status == BR.SCATTERED
    assert ((status == BR.ABSORBED) | kept).all()
    counts, outside = _bin_counts(obj, d_in, dirs[kept])
    assert outside == 0                                                    # no accepted direction leaves the lobe
    worst = _worst_bin(counts, _converged_masses(obj, d_in), int((~kept).sum()))
    print(f"fuzz {fuzz} {incidence}: worst bin {worst:.2f} sigma, absorbed {(~kept).mean():.5f}")
    assert worst <= 5.0


@pytest.mark.parametrize("fuzz", sorted(FUZZES))
def test_b_the_density_integrates_to_one_and_its_gated_integral_is_the_kept_share(oracle, fuzz):
    """Over the whole sphere (no gate) the Metal density integrates to 1 for fuzz <= 1, to 1e-4: the midpoint rule on 512 x 1024
    cells, second order: its error is a third of what the last halving moved the sum by, and that is below 3e-5 (asserted).  The gated integral equals the restated scatter's share
    of rays that were not absorbed within 5 binomial standard errors."""
    obj = FUZZES[fuzz]
    for name, d_in in INCIDENCES.items():
        total = _bin_masses(obj, d_in, 64, gated=False).sum()
        assert abs(total - _bin_masses(obj, d_in, 32, gated=False).sum()) < 3e-5
        gated = _bin_masses(obj, d_in, 64).sum()
        _, status = _scattered(oracle, obj, d_in, 0xA000 + obj)
        kept = (status == BR.SCATTERED).mean()
        se = np.sqrt(max(gated * (1.0 - gated), 1.0 / N_SAMPLES) / N_SAMPLES)
        print(f"fuzz {fuzz} {name}: integral {total:.6f}, gated {gated:.6f}, kept {kept:.6f} +- {se:.6f}")
        assert abs(total - 1.0) < 1e-4
        assert gated <= total + 1e-12 and abs(kept - gated) <= 5.0 * se


def test_c_lambertian_histogram_and_mean_cosine(oracle):
    """(a) for Lambertian.scatter: cos / pi about the normal; and the mean cosine of the samples is 2/3 within 5 standard errors
    (the cosine's variance under cos / pi is 1/2 - 4/9)."""
    for obj in (I.FLOOR, I.RED):
        d_in = INCIDENCES["slant"]
        dirs, status = _scattered(oracle, obj, d_in, 0xC000 + obj)
        assert (status == BR.SCATTERED).all()
        counts, outside = _bin_counts(obj, d_in, dirs)
        masses = _converged_masses(obj, d_in)
        assert outside == 0 and abs(masses.sum() - 1.0) < 1e-4
        worst = _worst_bin(counts, masses, 0)
        cos = dirs[:, 2] / np.sqrt((dirs * dirs).sum(axis=1))
        print(f"object {obj}: worst bin {worst:.2f} sigma, mean cosine {cos.mean():.5f}")
        assert worst <= 5.0
        assert abs(cos.mean() - 2.0 / 3.0) <= 5.0 * np.sqrt((0.5 - 4.0 / 9.0) / N_SAMPLES)


def _everything(oracle):
    g = I.all_items(oracle)
    if "res" not in g:
        g["res"] = R.evaluate(g["recs"], *g["items"])
    return g


def test_d_value_is_albedo_times_pdf_exactly(oracle):
    g = _everything(oracle)
    res, raw = g["res"], g["items"][1]
    obj = raw.view(np.int32)[:, 14].astype(np.int64)
    dense = res["kind"] == R.DENSITY
    assert dense.sum() > 400 and (res["pdf"][dense] > 0).sum() > 250
    with np.errstate(all="ignore"):
        want = g["recs"][obj[dense], 11:14] * res["pdf"][dense][:, None]
    assert R.same_bits(res["value"][dense], want).all()
    assert (res["value"][~dense] == 0).all() and (res["pdf"][~dense] == 0).all()
    assert not np.isnan(res["pdf"]).any() and (res["pdf"] >= 0).all()


NAMED = {  # name: (kind, is pdf > 0)
    "reflect": (R.DENSITY, True), "reflect_scaled": (R.DENSITY, True), "below_metal": (R.DENSITY, False),
    "below_lambertian": (R.DENSITY, False), "tangent_zero": (R.DENSITY, False), "tangent_minus_zero": (R.DENSITY, False),
    "tangent_metal": (R.DENSITY, False), "tiny": (R.DENSITY, True), "tiny_lambertian": (R.DENSITY, True),
    "underflow": (R.DENSITY, False), "overflow": (R.DENSITY, False), "overflow_lambertian": (R.DENSITY, False),
    "zero_out": (R.DENSITY, False), "nan_out": (R.DENSITY, False), "nan_out_lambertian": (R.DENSITY, False),
    "inf_out": (R.DENSITY, False), "inf_out_lambertian": (R.DENSITY, False), "nan_in": (R.DENSITY, False),
    "zero_in": (R.DENSITY, False), "grazing": (R.DENSITY, True), "grazing_wide": (R.DENSITY, True),
    "normal_incidence": (R.DENSITY, True), "normal_incidence_off": (R.DENSITY, True), "nonunit_normal": (R.DENSITY, False),
    "nonunit_normal_lambertian": (R.DENSITY, True), "zero_normal": (R.DENSITY, False), "zero_normal_lambertian": (R.DENSITY, False),
    "nan_normal": (R.DENSITY, False), "object_minus_one": (R.NONE, False), "object_past_the_end": (R.NONE, False),
    "object_int_min": (R.NONE, False), "glass": (R.DELTA, False), "mirror": (R.DELTA, False), "denormal_fuzz": (R.DENSITY, False),
    "fuzz_1e-100": (R.DENSITY, None), "fuzz_1e-100_axis": (R.DENSITY, True), "fuzz_1e-8": (R.DENSITY, True),
    "negative_fuzz": (R.DENSITY, True), "holds_origin": (R.DENSITY, True), "holds_origin_axis": (R.DENSITY, True),
    "touches_origin": (R.DENSITY, True), "mover": (R.DENSITY, True), "red": (R.DENSITY, True),
    "lo_zero": (R.DENSITY, True), "gate_underflows": (R.DENSITY, False),
    "rim_inside": (R.DENSITY, True), "rim_exact": (R.DENSITY, False), "rim_outside": (R.DENSITY, False),
}


def test_e_kind_and_zero_cases_of_the_named_items(oracle):
    g = _everything(oracle)
    res = g["res"]
    assert sorted(g["names"]) == sorted(NAMED)
    for name, (kind, positive) in NAMED.items():
        k = g["names"][name]
        assert res["kind"][k] == kind, name
        if positive is not None:                                           # (fuzz_1e-100 off the axis: left to the rounding of w x r)
            assert (res["pdf"][k] > 0) == positive, (name, res["pdf"][k])
        if not res["pdf"][k] > 0:
            assert res["pdf"][k] == 0 and (res["value"][k] == 0).all(), name
    # the rim at normal incidence: s2 is the double just below f * f, f * f itself, the double just above
    _, s2 = I._rim(0.3, np.array([0.0, 0.0, -1.0]), Z)
    ff = 0.3 * 0.3
    assert s2["rim_inside"] == np.nextafter(ff, 0.0) and s2["rim_exact"] == ff and s2["rim_outside"] == np.nextafter(ff, 1.0)
    # the closed forms on the axis: b = 1, s2 = 0, q = f: f (3 + f^2) / (2 pi f^3); the Lambertian value on its own
    k = g["names"]["reflect"]
    assert abs(res["pdf"][k] - 0.3 * 3.09 / (2.0 * np.pi * 0.027)) < 1e-12 * res["pdf"][k]
    k = g["names"]["holds_origin_axis"]                                    # b = 1, q = 1.5: (2.5)^3 / (4 pi 1.5^3)
    assert abs(res["pdf"][k] - 2.5 ** 3 / (4.0 * np.pi * 1.5 ** 3)) < 1e-14
    k = g["names"]["red"]
    w = np.array([0.5, 1.0, 0.1]) / np.sqrt(1.26)
    assert abs(res["pdf"][k] - (w @ np.array([1.0, 2.0, 2.0]) / 3.0) / np.pi) < 1e-15
    # lo == 0 exactly takes the form of the ball that holds the origin, which here differs from the other in the last bits
    w = np.array([20.0, 0.0, 21.0]) * (1.0 / np.sqrt(20.0 * 20.0 + 0.0 * 0.0 + 21.0 * 21.0))
    h = 1.0 * 1.0 - ((-w[0]) * (-w[0]))
    q = np.sqrt(h)
    assert w[2] - q == 0.0
    k, hi = g["names"]["lo_zero"], w[2] + q
    assert res["pdf"][k] == (hi * hi * hi) / (4.0 * R.PI * 1.0) != (q * (3.0 * w[2] * w[2] + h)) / (2.0 * R.PI * 1.0)
    # a length of `out` changes nothing but roundings
    a, b = res["pdf"][g["names"]["normal_incidence"]], res["pdf"][g["names"]["reflect"]]
    assert abs(a - b) < 1e-13 * a


def test_f_round_trip_scattered_has_a_density_absorbed_has_none(oracle):
    """Every SCATTERED ray of the restated scatter has pdf > 0 under the restated density for the same (in, record), every ABSORBED
    one pdf == 0 -- on the objects whose lobe float64 resolves (bsdf_inputs.RESOLVED: |fuzz| >= 1e-8)."""
    g = _everything(oracle)
    t0, status = g["trip"]
    pdf, kind = g["res"]["pdf"][t0:], g["res"]["kind"][t0:]
    assert len(status) == I.N_TRIP and (kind == R.DENSITY).all()
    assert (status == BR.SCATTERED).sum() >= 100 and (status == BR.ABSORBED).sum() >= 10
    assert (pdf[status == BR.SCATTERED] > 0).all() and (pdf[status == BR.ABSORBED] == 0).all()
    # and in the histograms' samples, by the thousand
    for fuzz, obj in FUZZES.items():
        d_in = INCIDENCES["grazing"]
        dirs, st = _scattered(oracle, obj, d_in, 0xA000 + obj)
        p = _density(obj, d_in, dirs)
        assert (p[st == BR.SCATTERED] > 0).all() and (p[st == BR.ABSORBED] == 0).all(), fuzz


def test_g_the_entries_are_declared_bound_and_exported(tor):
    src = open(os.path.join(ROOT, "include", "tor_bsdf.h")).read()
    assert '#include "tor_bsdf.h"' in open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    assert tor.BSDF_SYMBOLS == ["tor_bsdf_eval_device", "tor_bsdf_eval_host"]
    for name in tor.BSDF_SYMBOLS:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_bsdf.h"
        assert hasattr(L, name) and getattr(L, name).argtypes == tor._signatures()[name]
    assert sorted(tor.BSDF_SYMBOLS) == sorted(set(re.findall(r"TOR_API\s+int\s+(tor_\w+)\s*\(", src)))
    assert (tor.BSDF_NONE, tor.BSDF_DENSITY, tor.BSDF_DELTA) == (R.NONE, R.DENSITY, R.DELTA) == (0, 1, 2)
    assert re.search(r"TOR_BSDF_NONE = 0, TOR_BSDF_DENSITY = 1, TOR_BSDF_DELTA = 2", src)
    assert callable(tor.Context.bsdf) and callable(tor.glossy_objects)
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert mk.count("tor_bsdf.hip") == 2 and mk.count("tor_bsdf.h ") == 1          # SRCS and ASM_SRCS; HDRS
    assert "-ffp-contract=off" in mk
    glossy = tor.glossy_objects(I.scene())
    want = np.zeros(14, dtype=bool)
    want[[I.DENORMAL, I.F1E100, I.F1E8, I.F005, I.F03, I.F09, I.F1, I.FNEG, I.F15, I.MOVER]] = True
    assert glossy.dtype == bool and np.array_equal(glossy, want)
    assert np.array_equal(tor.glossy_objects(tor.Scene.from_records(I.scene())), want)
    assert not (glossy & tor.diffuse_objects(I.scene())).any()


def test_g_refusals_that_need_no_device(tor):
    """The checks that come before any device work, in the header's order; nothing is written.  (None of them reads the context, so
    a non-NULL pointer stands in for one.)"""
    L = tor.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.cast((C.c_char * 64)(), C.c_void_p)
    err = lambda: L.tor_last_error().decode()
    dev, host = L.tor_bsdf_eval_device, L.tor_bsdf_eval_host
    assert dev(None, 1, p, p, p, None, 1, p, p, p, None) == -1 and "tor_bsdf_eval_device" in err()
    assert host(None, 1, p, p, p, None, 1, p, p, p) == -1 and "tor_bsdf_eval_host" in err()
    assert dev(ctx, -1, None, p, p, None, -1, p, p, p, None) == -1 and "n_list" not in err()          # n before n_list
    assert dev(ctx, 1, None, p, p, None, -1, p, p, p, None) == -1 and "n_list < 0" in err()           # n_list before the NULLs
    assert dev(ctx, 2, None, p, p, None, 1, p, p, p, None) == -1 and "without a list" in err()        # the list before the NULLs
    for hole in range(5):                                                  # NULL in, hits, out, value or pdf with work to do
        a = [p] * 5
        a[hole] = None
        assert dev(ctx, 1, a[0], a[1], a[2], None, 1, a[3], a[4], None, None) == -1 and "NULL" in err()
        assert host(ctx, 1, a[0], a[1], a[2], None, 1, a[3], a[4], None) == -1 and "NULL" in err()
    assert all(v == 0.0 for v in buf)
