"""The phase-function queries without a GPU: the restatement of include/tor_phase.h (tests/phase_restatement.py), which the GPU suite
holds the kernels to bit for bit, is checked here against hand-worked rows and the header's invariances; the named inputs do what
their names say and the crafted generator states put the chosen words where they say; each restated variant is told apart by a
named case; the entries are declared, bound, built and refuse what the header says, in its order; the Python glue runs against a
recording stand-in for the library; and the physics checks of the GPU suite are shown to hold for the definition itself."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import media_restatement as MR
import phase_inputs as I
import phase_restatement as R
import radiance_restatement as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_want = {}


def _answer(oracle, name):
    if name not in _want:
        details = {}
        _want[name] = (I.answer(oracle, I.BY_NAME[name], details=details), I.evaluation(I.BY_NAME[name]), details)
    return _want[name]


def test_a_inputs_do_what_their_names_say(oracle):
    got = I.assert_coverage(oracle)
    print(got)
    assert set(I.NAMES) == {"one", "one_isotropic", "two_overlap", "nested3", "row64", "sigma0", "moving", "crafted", "fallback"}
    assert sorted(len(v[(v >= 0) & (v < 257)]) for v in I.lists().values()) == [1, 63, 64, 65, 255]
    found = I.search_clamp(4096, 3)                               # the search that found CLAMP_G still finds cases, on both sides
    assert sum(1 for r in found if r[2] < -1.0) >= 100 and sum(1 for r in found if r[2] > 1.0) >= 100
    assert all(r[1] in (0.0, I.U_MAX) for r in found)
    assert I.CLAMP_G[0][:2] == (0.3, 0.0)                         # g = 0.3 at u_cos = 0: the committed row below -1


def test_a_the_generators_step_is_inverted(oracle):
    """unstep undoes step; a crafted state gives the oracle's generator the chosen word at the chosen position."""
    L = oracle.lib()
    g = np.random.default_rng(1)
    for _ in range(200):
        s = tuple(int(v) for v in g.integers(0, 1 << 64, size=4, dtype=np.uint64))
        assert I.step(I.unstep(s))[1] == s and I.unstep(I.step(s)[1]) == s
    for position in range(3):
        for word in (0, I.ALL_ONES, 1 << 62, 0x123456789abcdef0):
            s = I.state_with(position, word, (0xdeadbeef, 0x0123456789))
            assert I.outputs(s)[position] == word
            st = np.asarray([s], dtype=np.uint64)
            us = [L.oracle_rng_uniform01(RR._ptr(st, 0)) for _ in range(3)]
            assert us[position] == I.uniform_of(word) and us == [I.uniform_of(o) for o in I.outputs(s)]
    assert I.U_MAX == 1.0 - 2.0 ** -52


# ---- hand-worked rows -----------------------------------------------------------------------------------------------------------

def test_b_rows_by_hand(oracle):
    sincos = lambda phi: MR._sincos(oracle.lib(), phi)
    # g = 0: the evaluation is albedo / FOUR_PI and the density 1 / FOUR_PI, whatever the directions
    value, pdf = R.eval_row([0.5], [[0.9, 0.6, 0.3]], [0.0], [0.3, -2.0, 1.0], 1, [1e150, 3.0, -4.0])
    assert pdf == 1.0 / R.FOUR_PI and value == [(0.5 * a) * (1.0 / R.FOUR_PI) / 0.5 for a in (0.9, 0.6, 0.3)]
    assert R.hg(0.0, 0.37) == R.hg(-0.0, -1.0) == 1.0 / R.FOUR_PI
    # forward and backward values of HG in closed form: (1 +- g) / (FOUR_PI (1 -+ g)^2)
    for g in (0.3, -0.7, 0.99):
        assert R.hg(g, 1.0) == pytest.approx((1 + g) / (R.FOUR_PI * (1 - g) ** 2), rel=1e-12)
        assert R.hg(g, -1.0) == pytest.approx((1 - g) / (R.FOUR_PI * (1 + g) ** 2), rel=1e-12)
    # the all-zero state: u = 0 three times; mu = -1 for any g != 0 (after the clamp), +1 for g = 0; phi = 0
    for g in (0.3, 0.99, -0.99, -0.7, 2.0 ** -20, -(2.0 ** -20)):
        assert R.cosine(g, 0.0)[0] == -1.0, g
    assert R.cosine(0.0, 0.0)[0] == 1.0 and R.cosine(-0.0, 0.0)[0] == 1.0 and R.cosine(0.0, 0.5)[0] == 0.0
    ray = [1.0, 2.0, 3.0, 0.0, 0.0, 2.0, 0.25]
    out, att, pdf = R.sample_row([0.5], [[0.9, 0.6, 0.3]], [0.3], ray, 1.5, 1, 0.0, 0.0, 0.0, sincos)
    assert out == [1.0, 2.0, 6.0, 0.0, 0.0, -1.0, 0.25] and pdf == R.hg(0.3, -1.0)      # straight back, from o + t d
    assert att == [(0.5 * a) * pdf / (0.5 * pdf) for a in (0.9, 0.6, 0.3)]
    # a quarter turn of the azimuth around +z at mu = 0 (g = 0, u_cos = 0.5): b1 = x, b2 = y; v = y to within the sin / cos
    out, att, pdf = R.sample_row([1.0], [[1.0, 1.0, 1.0]], [0.0], [0, 0, 0, 0, 0, 1.0, 0], 0.0, 1, 0.0, 0.5, 0.25, sincos)
    assert abs(out[3]) < 1e-15 and out[4] == 1.0 and out[5] == 0.0 and pdf == 1.0 / R.FOUR_PI
    # refusals: the zeros, for the word 0, a bit at n_media, sigma 0 alone, a zero and an overflowing direction
    for A, d in ((0, [0, 0, 1.0]), (2, [0, 0, 1.0]), (1, [0.0, 0.0, 0.0]), (1, [1e160, 0, 0]), (1, [1e-170, 0, 0])):
        assert R.sample_row([0.5], [[1, 1, 1]], [0.3], [0, 0, 0] + d + [0], 1.0, A, 0.3, 0.3, 0.3, sincos) == R.ZERO_ROW
    assert R.sample_row([0.0], [[1, 1, 1]], [0.3], [0, 0, 0, 0, 0, 1.0, 0], 1.0, 1, 0.3, 0.3, 0.3, sincos) == R.ZERO_ROW
    # the mixture: two media, the density is the sigma-weighted mean, the value the sigma * albedo-weighted one
    sg, al, gs = [1.0, 3.0], [[1.0, 0.0, 0.5], [0.0, 1.0, 0.5]], [0.0, 0.5]
    value, pdf = R.eval_row(sg, al, gs, [0, 0, 1.0], 3, [0, 0, 1.0])
    p0, p1 = R.hg(0.0, 1.0), R.hg(0.5, 1.0)
    assert pdf == (1.0 * p0 + 3.0 * p1) / 4.0 and value[0] == (1.0 * p0) / 4.0 and value[1] == (0.0 + 3.0 * p1) / 4.0


def test_b_where_the_fallback_decides(oracle):
    """uniform01 keeps 52 bits: its largest value is 1 - 2^-52, and fl((1 - 2^-52) rho) < rho for every normal rho (the exact
    product lies between one and two ulps of rho below rho).  acc ends at rho to the bit (the same sums in the same order), so
    for a normal rho `x < acc` holds at the last active medium at the latest and the fallback decides nothing.  For a subnormal
    rho below 2^-1023 the product rounds back to rho, and the fallback decides: the case `fallback`."""
    g = np.random.default_rng(2)
    rho = np.concatenate([g.uniform(1e-3, 1e3, 100000), 2.0 ** g.integers(-40, 40, 1000), np.nextafter(2.0 ** g.integers(-40, 40, 1000), np.inf),
                          [2.2250738585072014e-308, 1.7976931348623157e308]])
    assert (I.U_MAX * rho < rho).all()
    sub = 2.0 ** -1030
    assert I.U_MAX * sub == sub and R.select([sub, 0.0], 3, I.U_MAX, sub) == (0, True)   # ... and skips the medium of sigma 0
    assert R.select([sub, 0.0], 3, I.U_MAX, sub, "no_fallback") == (-1, True) and R.select([sub], 1, 0.5, sub) == (0, False)
    assert R.select([0.1, 0.2, 0.3], 7, I.U_MAX, (0.1 + 0.2) + 0.3) == (2, False)
    want = _answer(oracle, "fallback")[0]
    for name, i in I.FALLBACK_ROWS.items():
        assert want["pdf"][i] > 0 and np.allclose(want["attenuation"][i], [0.9, 0.5, 0.1], rtol=1e-9, atol=0), name   # (subnormal products)


# ---- invariances --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_overlap", "row64", "crafted"])
def test_c_invariant_under_permutation_of_the_rays_and_split_lists(oracle, name):
    c = I.BY_NAME[name]
    want, wev, _ = _answer(oracle, name)
    n = len(c["rays"])
    perm = np.random.default_rng(3).permutation(n)
    p = dict(c, rays=c["rays"][perm], t=c["t"][perm], active=c["active"][perm], states=c["states"][perm], out=c["out"][perm])
    got = I.answer(oracle, p)
    assert not R.mismatches({k: v[np.argsort(perm)] for k, v in got.items()}, want)
    ev = I.evaluation(p)
    assert not R.mismatches({k: v[np.argsort(perm)] for k, v in ev.items()}, wev, keys=("value", "pdf"))
    first = I.answer(oracle, c, index=np.arange(0, n, 2))
    assert (first["rays"][1::2] == 0).all() and np.array_equal(first["states"][1::2], c["states"][1::2])
    both = I.answer(oracle, dict(c, states=first["states"]), index=np.arange(1, n, 2), into=first)
    assert not R.mismatches(both, want)
    ev2 = I.evaluation(c, index=np.arange(1, n, 2), into=I.evaluation(c, index=np.arange(0, n, 2)))
    assert not R.mismatches(ev2, wev, keys=("value", "pdf"))


def test_c_the_table_order_matters_only_where_sums_round(oracle):
    """Reversing the table (and the bits of every word with it) keeps the answer where one medium is active, and moves it by
    rounding alone where several are: 0.1 + 0.2 + 0.3 sums differently from the other end."""
    c = I.BY_NAME["nested3"]
    want, wev, _ = _answer(oracle, "nested3")
    M = 3
    rev = lambda v: sum(((int(v) >> m) & 1) << (M - 1 - m) for m in range(M)) | (int(v) >> M << M)
    r = dict(c, sigma=c["sigma"][::-1], albedo=c["albedo"][::-1], g=c["g"][::-1], active=np.asarray([rev(v) for v in c["active"]], dtype=np.uint64))
    ev = I.evaluation(r)
    pop = np.array([bin(int(v) & 7).count("1") for v in c["active"]])
    single = (pop == 1) & (wev["pdf"] > 0)
    assert single.sum() >= 20 and MR.same_bits(ev["pdf"][single], wev["pdf"][single]).all()
    assert MR.same_bits(ev["value"][single], wev["value"][single]).all()
    several = (pop == 3) & (wev["pdf"] > 0)
    assert several.sum() >= 20 and not MR.same_bits(ev["value"][several], wev["value"][several]).all()
    assert np.allclose(ev["value"][several], wev["value"][several], rtol=1e-14, atol=0) and np.allclose(ev["pdf"], wev["pdf"], rtol=1e-14, atol=0)


# ---- the variants -----------------------------------------------------------------------------------------------------------------

VARIANT_CASES = {"no_clamp": "crafted", "x_le_acc": "crafted", "no_fallback": "fallback", "descending": "nested3",
                 "no_copysign": "one", "mu_from_dot": "two_overlap"}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_d_each_variant_is_told_apart_by_a_named_case(oracle, variant):
    assert set(VARIANT_CASES) == set(R.VARIANTS)
    c = I.BY_NAME[VARIANT_CASES[variant]]
    want = _answer(oracle, c["name"])[0]
    got = I.answer(oracle, c, variant=variant)
    bad = R.mismatches(got, want)
    assert bad, variant
    differ = lambda row: not MR.same_bits(got["rays"][row], want["rays"][row]).all() or not MR.same_bits(got["pdf"][row], want["pdf"][row]).all()
    if variant == "no_clamp":
        assert differ(I.CRAFTED_ROWS["u_cos_zero_g_lo"]) and differ(I.CRAFTED_ROWS["all_zero_first_medium"])
        ev = I.evaluation(I.BY_NAME["one"], variant=variant)           # the evaluation's clamp: dot(w, v) passes 1 by rounding
        assert R.mismatches(ev, _answer(oracle, "one")[1], keys=("value", "pdf"))
    if variant == "x_le_acc":
        assert differ(I.CRAFTED_ROWS["u_sel_on_boundary"]) or differ(I.CRAFTED_ROWS["u_sel_on_second_boundary"])
    if variant == "no_copysign":
        for name in ("minus_z", "minus_z_long", "negative_zero_z", "near_minus_z"):
            assert differ(I.DIRECTION_ROWS[name]), name
        assert not differ(I.DIRECTION_ROWS["plus_z"])
    if variant == "no_fallback":
        for name, i in I.FALLBACK_ROWS.items():
            assert differ(i) and got["pdf"][i] == 0 and want["pdf"][i] > 0, name
    if variant == "descending":
        assert R.mismatches(I.evaluation(c, variant=variant), _answer(oracle, c["name"])[1], keys=("value", "pdf"))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_e_the_entries_are_declared_bound_and_built(tor):
    src = open(os.path.join(ROOT, "include", "tor_phase.h")).read()
    render = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    assert '#include "tor_phase.h"' in render and render.index('#include "tor_media.h"') < render.index('#include "tor_phase.h"')
    L = tor.lib()
    assert tor.PHASE_SYMBOLS == ["tor_scene_media_phase", "tor_phase_eval_device", "tor_phase_eval_host", "tor_phase_sample_device",
                                 "tor_phase_sample_host"]
    for name in tor.PHASE_SYMBOLS:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_phase.h"
        assert hasattr(L, name) and getattr(L, name).argtypes == tor._phase_signatures()[name]
        assert name not in tor.EXPORTED_SYMBOLS and name not in tor._signatures() and name not in tor.MEDIA_SYMBOLS
    assert sorted(tor.PHASE_SYMBOLS) == sorted(set(re.findall(r"TOR_API\s+int\s+(tor_\w+)\s*\(", src)))
    media = open(os.path.join(ROOT, "include", "tor_media.h")).read()
    assert sorted(tor.MEDIA_SYMBOLS) == sorted(set(re.findall(r"TOR_API\s+int\s+(tor_\w+)\s*\(", media))) and len(tor.MEDIA_SYMBOLS) == 7
    assert re.search(r"#define TOR_PHASE_G_MAX 0\.99\b", src) and tor.PHASE_G_MAX == R.G_MAX == 0.99
    assert re.search(r"#define TOR_PHASE_G_MIN \(1\.0 / 1048576\.0\)", src) and tor.PHASE_G_MIN == R.G_MIN == 2.0 ** -20 == 1.0 / 1048576.0
    for name in ("set_media_phase", "sample_phase", "phase", "trace_media", "trace_media_direct"):
        assert callable(getattr(tor.Context, name))
    assert "trace_media_direct" in tor.integrators.INTEGRATORS
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert mk.count("tor_phase.hip") == 2 and mk.count("tor_phase.h ") == 1          # SRCS and ASM_SRCS; HDRS
    for word in ("clamp1", "copysign", "Termination", "chosen = last", "exactly three outputs", "x < acc", "not dot(w, v)"):
        assert word in src, word
    hip = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "tor_phase.hip")).read().split("#include <hip/hip_runtime.h>")[1]
    for fn in ("log", "exp", "atan2", "pow", "sin", "cos"):                          # the library takes none (sincos_2pi is its own)
        assert not re.search(r"\b(__builtin_|std::|::)?" + fn + r"[a-z0-9]*\s*\(", hip), fn
    assert "__shared__" not in hip and "atomic" not in hip


def test_e_refusals_that_need_no_device(tor):
    """The checks that come before any device work, in the header's order; nothing is written.  (None of them reads the context, so a
    non-NULL pointer stands in for one; those that do -- no scene, no table, the count, the values of g -- are in the GPU suite.)"""
    L = tor.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.cast((C.c_char * 64)(), C.c_void_p)
    err = lambda: L.tor_last_error().decode()
    assert L.tor_scene_media_phase(None, 1, p) == -1 and "tor_scene_media_phase: ctx is NULL" in err()
    for f, tail, name in ((L.tor_phase_eval_device, (None,), "tor_phase_eval_device"), (L.tor_phase_eval_host, (), "tor_phase_eval_host")):
        assert f(None, 1, p, p, p, None, 1, p, p, *tail) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, None, None, None, -1, None, None, *tail) == -1 and "n_rays < 0" in err()
        assert f(ctx, 1, None, None, None, None, -1, None, None, *tail) == -1 and "n_list < 0" in err()
        assert f(ctx, 2, None, None, None, None, 1, None, None, *tail) == -1 and "without a list" in err()
        for hole in range(5):                                                        # in, active, out, value, pdf
            a = [p] * 5
            a[hole] = None
            assert f(ctx, 1, a[0], a[1], a[2], None, 1, a[3], a[4], *tail) == -1 and "NULL in, active, out" in err(), hole
    for f, tail, name in ((L.tor_phase_sample_device, (None,), "tor_phase_sample_device"), (L.tor_phase_sample_host, (), "tor_phase_sample_host")):
        assert f(None, 1, p, p, p, p, None, 1, p, p, p, *tail) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, None, None, None, None, -1, None, None, None, *tail) == -1 and "n_rays < 0" in err()
        assert f(ctx, 1, None, None, None, None, None, -1, None, None, None, *tail) == -1 and "n_list < 0" in err()
        assert f(ctx, 2, None, None, None, None, None, 1, None, None, None, *tail) == -1 and "without a list" in err()
        for hole in range(6):                                                        # rays, t, active, rng, rays_out, att (pdf may be NULL)
            a = [p] * 6
            a[hole] = None
            assert f(ctx, 1, a[0], a[1], a[2], a[3], None, 1, a[4], a[5], None, *tail) == -1 and "NULL rays, t, active" in err(), hole
    assert all(v == 0.0 for v in buf)


# ---- Python glue on a recording library -----------------------------------------------------------------------------------------------

class _Recorder:
    """A stand-in for the loaded library (the pattern of tests/test_media_query.py): every tor_* entry records (name, args) and
    returns 0."""

    def __init__(self, note=b"phase sample: 2 media"):
        self.calls, self.note = [], note

    def __getattr__(self, name):
        if not name.startswith("tor_"):
            raise AttributeError(name)
        if name == "tor_last_note":
            return lambda: self.note
        if name == "tor_last_error":
            return lambda: b""

        def entry(*args):
            self.calls.append((name, tuple((a.value or 0) if isinstance(a, C.c_void_p) else a for a in args)))
            return 0
        return entry


def test_f_python_glue_on_a_recording_library(tor):
    ctx = object.__new__(tor.Context)
    ctx._h = C.c_void_p(16)
    saved = tor._lib
    rays = np.zeros((5, 7))
    try:
        rec = tor._lib = _Recorder()
        ctx.set_media([3, 1], [0.5, 2.0])
        ctx.set_media_phase([0.3, -0.7])
        ctx.set_media_phase()
        (_, _), (n1, a1), (n2, a2) = rec.calls
        assert n1 == n2 == "tor_scene_media_phase" and a1[0] == 16 and a1[1] == 2 and a1[2] not in (0, 16) and a2[1:] == (2, None)
        st = np.arange(20, dtype=np.uint64).reshape(5, 4)
        march = tor.MediaMarch(np.zeros(5, dtype=np.int32), np.zeros(5), np.zeros(5), np.zeros(5, dtype=np.int64), np.zeros(5), "")
        rec = tor._lib = _Recorder()
        new, att = ps = ctx.sample_phase(rays, march, st, index=[1])
        (name, a), = rec.calls
        assert name == "tor_phase_sample_host" and a[0] == 16 and a[1] == 5 and a[2] == rays.ctypes.data and a[3] == march.t.ctypes.data
        assert a[4] == march.active.ctypes.data and a[5] == ps.rng.ctypes.data != st.ctypes.data and a[7] == 1
        assert a[8:11] == (new.ctypes.data, att.ctypes.data, ps.pdf.ctypes.data) and len(a) == 11
        assert new.shape == (5, 7) and att.shape == (5, 3) and ps.pdf.shape == (5,) and ps.rays is new and ps.attenuation is att
        assert ps.mode == "2 media" and isinstance(ps, tuple) and len(ps) == 2
        rec = tor._lib = _Recorder()
        again = ctx.sample_phase(rays, (np.zeros(5), np.zeros(5, dtype=np.int64)), st, out=ps)
        assert rec.calls[0][1][8] == new.ctypes.data and again.pdf is ps.pdf and rec.calls[0][1][6] == 0 and rec.calls[0][1][7] == 5
        for bad in (lambda: ctx.sample_phase(rays, (np.zeros(4), np.zeros(5, dtype=np.int64)), st),
                    lambda: ctx.sample_phase(rays, march, st, out=(new, att)), lambda: ctx.sample_phase(rays, march, st[:4]),
                    lambda: ctx.sample_phase(np.zeros((5, 6)), march, st)):
            with pytest.raises(ValueError):
                bad()
        rec = tor._lib = _Recorder(b"phase eval: 2 media")
        out = np.ones((5, 7))
        ev = ctx.phase(rays, march, out, index=[4, 0])
        (name, a), = rec.calls
        assert name == "tor_phase_eval_host" and a[1] == 5 and a[2] == rays.ctypes.data and a[3] == march.active.ctypes.data
        assert a[4] == out.ctypes.data and a[5] not in (0, 16) and a[6] == 2 and a[7:] == (ev.value.ctypes.data, ev.pdf.ctypes.data)
        assert ev.value.shape == (5, 3) and ev.pdf.shape == (5,) and ev.mode == "2 media"
        rec = tor._lib = _Recorder(b"phase eval: 2 media")
        ev2 = ctx.phase(rays, np.zeros(5, dtype=np.int64), out, out=ev)
        assert ev2.value is ev.value and rec.calls[0][1][5] == 0
        for bad in (lambda: ctx.phase(rays, np.zeros(4, dtype=np.int64), out), lambda: ctx.phase(rays, march, np.ones((4, 7))),
                    lambda: ctx.phase(rays, march, out, out=ps), lambda: ctx.phase(rays, None, out)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(ValueError, match="lamp_mask"):
            ctx.trace_media_direct(rays, st, np.zeros((4, 3)), None)
    finally:
        tor._lib = saved
        ctx._h = C.c_void_p()


def test_f_bind_keeps_its_table_and_lib_binds_the_phase_entries_after_it(tor):
    import types
    assert not set(tor.PHASE_SYMBOLS) & set(tor._SIGNATURES) and sorted(tor._PHASE_SIGNATURES) == sorted(tor.PHASE_SYMBOLS)
    older = types.SimpleNamespace(tor_phase_eval_host=types.SimpleNamespace(argtypes=None, restype=C.c_int))
    tor._bind(older, tor.PHASE_SYMBOLS, skip_missing=True, table=tor._PHASE_SIGNATURES)   # an A/B build older than the entries
    assert older.tor_phase_eval_host.argtypes == tor._PHASE_SIGNATURES["tor_phase_eval_host"]
    with pytest.raises(AttributeError):
        tor._bind(older, tor.PHASE_SYMBOLS, table=tor._PHASE_SIGNATURES)


# ---- the physics checks hold for the definition ------------------------------------------------------------------------------------------

V_NORM_MEASURED = 6.7e-16      # the largest |v.v - 1| the restatement gives over the committed inputs (printed below)


@pytest.mark.parametrize("g", [0.7, 0.3, -0.99])
def test_g_physics_on_the_restatement(oracle, g):
    """4096 draws from one medium.  The cosine of Henyey-Greenstein has mean g and second moment (1 + 2 g^2) / 3, so variance
    (1 - g^2) / 3: the mean of mu lies within 5 sqrt((1 - g^2) / 3 / 4096) of g.  The share of mu in each of 8 equal bins of
    [-1, 1] lies within 5 sqrt(p (1 - p) / 4096) of the closed-form p = CDF(hi) - CDF(lo).  v . b1 = st cos(phi) has mean 0 and
    variance E[1 - mu^2] / 2 = (1 - g^2) / 3: its mean lies within 5 sqrt((1 - g^2) / 3 / 4096) of 0."""
    c = I.physics_case(g)
    details = {}
    a = I.answer(oracle, c, details=details)
    mu = np.asarray([details[i]["mu"] for i in range(4096)])
    se = math.sqrt((1.0 - g * g) / 3.0 / 4096)
    print(f"g = {g}: mean mu {mu.mean():.5f} ({(mu.mean() - g) / se:+.2f} standard errors)")
    assert abs(mu.mean() - g) <= 5.0 * se
    edges = np.linspace(-1.0, 1.0, 9)
    p = I.hg_cdf(g, edges[1:]) - I.hg_cdf(g, edges[:-1])
    assert abs(p.sum() - 1.0) < 1e-12
    frac = np.histogram(mu, bins=edges)[0] / 4096.0
    assert (np.abs(frac - p) <= 5.0 * np.sqrt(p * (1.0 - p) / 4096)).all(), (frac, p)
    vb1 = np.asarray([R.dot(details[i]["v"], details[i]["b1"]) for i in range(4096)])
    assert abs(vb1.mean()) <= 5.0 * se
    assert np.abs(I.cosines(c, a) - mu).max() <= 4 * 9.4e-16


def test_g_the_direction_is_unit_and_the_density_is_the_evaluations(oracle):
    """|v . v - 1| over every sampled row of the committed inputs: the largest value measured is V_NORM_MEASURED = 6.7e-16 (the
    trial behind the definition saw 1.4e-15 over 2 x 10^6 draws per g); asserted: 4 times the measured value, 2.7e-15.  The density
    the sampler returns against the evaluation of the sampled ray: hg is evaluated at the cosine that was drawn, the evaluation
    sees dot(w, v) of the direction that was built; the two differ by at most 9.4e-16 (measured by that trial; 4 times that
    allowed), and |d ln hg / d mu| = 3 |g| / (1 + g^2 - 2 g mu) <= 3 |g| / (1 - |g|)^2, so the relative difference of the densities
    is at most 3 |g| / (1 - |g|)^2 * 4e-15 with |g| the table's largest.  Measured: at most 0.09 of that bound; for g = 0 the two
    are equal in every bit (hg does not depend on mu)."""
    worst_norm, worst = 0.0, 0.0
    for name in I.NAMES:
        c = I.BY_NAME[name]
        a = _answer(oracle, name)[0]
        ok = a["pdf"] > 0
        v = a["rays"][ok, 3:6]
        norm = np.abs(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2] - 1.0).max()
        worst_norm = max(worst_norm, float(norm))
        ev = R.evaluate(c["sigma"], c["albedo"], c["g"], c["rays"], c["active"], a["rays"])
        gmax = float(np.abs(c["g"]).max())
        tol = 3.0 * gmax / (1.0 - gmax) ** 2 * 4e-15
        rel = np.abs(ev["pdf"][ok] - a["pdf"][ok]) / a["pdf"][ok]
        worst = max(worst, float((rel / tol).max()) if tol > 0 else 0.0)
        assert (rel <= tol).all(), (name, float(rel.max()), tol)
        assert np.allclose(ev["value"][ok], a["attenuation"][ok] * a["pdf"][ok][:, None], rtol=tol + 1e-15, atol=0)   # value = att * pdf
    print(f"largest |v.v - 1| = {worst_norm:.3e}; largest density difference / its bound = {worst:.3f}")
    assert worst_norm <= 4 * V_NORM_MEASURED
