"""The participating-media queries without a GPU: the restatement of include/tor_media.h (tests/media_restatement.py), which the GPU
suite holds the kernels to bit for bit, is checked here against hand-worked cases, against the header's invariances and against
crossings_restatement's roots; the named inputs do what their names say; the restated mutants are told apart by named cases; the
entries are declared, bound and built and refuse what the header says, in its order; the Python glue runs against a recording
stand-in for the library; and the physics checks of the GPU suite are shown to hold for the definition itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crossings_restatement as X
import media_inputs as I
import media_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def test_a_inputs_do_what_their_names_say():
    got = I.assert_coverage()
    print(got)
    assert set(I.NAMES) == {"one", "two_overlap", "nested3", "row64", "coincident", "sigma0", "moving", "negative_radius", "edges",
                            "clamp"}
    assert sorted(len(v[(v >= 0) & (v < 257)]) for v in I.lists().values()) == [1, 63, 64, 65, 255]
    assert len(I.search_clamp(1 << 16, 5)) >= 100                # the search that found the committed case still finds cases


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------

def test_b_march_by_hand():
    ball = [I._sphere((0, 0, 0), 1.0)]
    ray = [[-6.0, 0, 0, 3.0, 0, 0, 0.0]]                          # central, |d| = 3: roots 5/3 and 7/3, chord 2 in the world
    m = R.march(ball, [0], [0.5], ray, INF)
    assert m["status"][0] == 0 and m["depth"][0] == 1.0 and m["t"][0] == INF and m["active"][0] == 0 and m["rho"][0] == 0
    m = R.march(ball, [0], [0.5], ray, 0.25)                      # a quarter of the way through: t = 5/3 + (0.25 / 0.5) / 3
    has, s0, s1 = R.roots(ball, [0], ray)
    assert m["status"][0] == 1 and m["t"][0] == s0[0, 0] + (0.25 / 0.5) / 3.0 and m["depth"][0] == 0.25
    assert m["active"][0] == 1 and m["rho"][0] == 0.5
    assert R.march(ball, [0], [0.5], ray, 1.0)["status"][0] == 0  # tau == the whole depth: strict <, no collision
    # two nested balls, sigma 1 and 2, along x from the centre with |d| = 1: depth 1 * 1 + ... = (1 + 2) * 1 + 1 * 1 = 4
    two = [I._sphere((0, 0, 0), 2.0), I._sphere((0, 0, 0), 1.0)]
    rays4 = [[0.0, 0, 0, 1.0, 0, 0, 0.0]] * 4
    m = R.march(two, [0, 1], [1.0, 2.0], rays4, [INF, 3.5, 3.0, 1.5])
    assert m["depth"].tolist() == [4.0, 3.5, 3.0, 1.5] and m["status"].tolist() == [0, 1, 1, 1]
    assert m["t"].tolist() == [INF, 1.5, 1.0, 0.5] and m["active"].tolist() == [0, 1, 1, 3] and m["rho"].tolist() == [0, 1.0, 1.0, 3.0]
    # (tau = 3.0 is the inner step exactly: no collision there; the outer shell collides at once, rem = 0 < step, at t = 1.0)
    # a range: t_max inside the inner ball
    m = R.march(two, [0, 1], [1.0, 2.0], rays4[:1], INF, [[0.25, 0.75]])
    assert m["depth"][0] == 1.5 and m["t"][0] == 0.75
    # nothing to do, and the refusals
    m = R.march(two, [0, 1], [1.0, 2.0], [[5.0, 0, 0, 1.0, 0, 0, 0.0]] * 3, [1.0, np.nan, -1.0])
    assert m["status"].tolist() == [0, -1, -1] and m["depth"].tolist() == [0, 0, 0] and m["t"].tolist() == [INF, 0.0, 0.0]
    # lists: entries outside [0, n) are skipped, unlisted rays keep what `into` holds
    into = {k: np.full(4, 7, dtype=v.dtype) for k, v in m.items()}
    got = R.march(two, [0, 1], [1.0, 2.0], rays4, [INF, 3.5, 3.0, 1.5], index=[2, -1, 9, 0], into=into)
    assert got["depth"].tolist() == [4.0, 7.0, 3.0, 7.0] and got["status"].tolist() == [0, 7, 1, 7]


def test_b_scatter_and_uniforms_by_hand(oracle):
    sigma, albedo = [1.0, 3.0], [[1.0, 0.0, 0.5], [0.0, 1.0, 0.5]]
    rays = np.array([[1.0, 2.0, 3.0, 0.5, 0.0, -1.0, 0.25]] * 5)
    st = I.states(5)
    active = np.array([3, 1, 0, 4, 2], dtype=np.uint64)
    s = R.scatter(oracle, sigma, albedo, rays, np.full(5, 2.0), active, st)
    assert s["attenuation"].tolist() == [[0.25, 0.75, 0.5], [1.0, 0.0, 0.5], [0, 0, 0], [0, 0, 0], [0.0, 1.0, 0.5]]
    assert (s["rays"][[0, 1, 4], 0:3] == [2.0, 2.0, 1.0]).all() and (s["rays"][[0, 1, 4], 6] == 0.25).all()
    assert (s["rays"][[2, 3]] == 0).all()                                           # no active medium / a bit at n_media
    v = s["rays"][[0, 1, 4], 3:6]
    assert np.allclose((v * v).sum(axis=1), 1.0, atol=1e-15)
    u, after = R.uniforms(oracle, st, 2)
    assert np.array_equal(after, s["states"]) and (after != st).any(axis=1).all()   # exactly two outputs, sampled or not
    assert np.array_equal(R.bits(s["rays"][0, 5]), R.bits(u[0, 1] * 2.0 + -1.0))     # z is the second draw
    u3, _ = R.uniforms(oracle, st, 3)
    assert np.array_equal(u3[:, :2], u) and (u3 >= 0).all() and (u3 < 1).all()


# ---- invariances ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_overlap", "nested3", "row64", "edges"])
def test_c_invariant_under_permutation_of_the_rays_and_split_lists(name):
    c = I.BY_NAME[name]
    want = I.answer(c)
    n = len(c["rays"])
    perm = np.random.default_rng(3).permutation(n)
    got = R.march(c["recs"], c["objects"], c["sigma"], c["rays"][perm], c["tau"][perm], None if c["t_range"] is None else c["t_range"][perm])
    assert not R.march_mismatches(got, {k: v[perm] for k, v in want.items()})
    half = I.answer(c, index=perm[: n // 2])
    assert not R.march_mismatches(I.answer(c, index=perm[n // 2:], into=half), want)


def test_c_the_table_order_matters_only_where_sums_round():
    """0.1 / 0.2 / 0.3: the table order sums ((0.1 + 0.2) + 0.3) = 0.6000000000000001, the reversed table ((0.3 + 0.2) + 0.1) = 0.6, so
    the reversed table gives other bits where all three overlap.  (0.3 + (0.2 + 0.1) would not show it: it is the same two
    additions, commuted.)  A table of two media adds its two sigmas once, either way round: the reversed table gives the same
    answer, the active bits swapped."""
    assert (0.1 + 0.2) + 0.3 != (0.3 + 0.2) + 0.1 and (0.1 + 0.2) + 0.3 == 0.3 + (0.2 + 0.1)
    c = I.BY_NAME["nested3"]
    want = I.answer(c)
    rev = R.march(c["recs"], c["objects"][::-1], c["sigma"][::-1], c["rays"], c["tau"], c["t_range"])
    three = want["active"] == 7
    assert three.sum() >= 5 and (rev["rho"][three] != want["rho"][three]).all() and (rev["active"][three] == 7).all()
    assert R.march_mismatches(rev, want)
    for name in ("two_overlap", "sigma0"):
        c = I.BY_NAME[name]
        want = I.answer(c)
        rev = R.march(c["recs"], c["objects"][::-1], c["sigma"][::-1], c["rays"], c["tau"], c["t_range"])
        swap = ((want["active"] & np.uint64(1)) << np.uint64(1)) | (want["active"] >> np.uint64(1))
        assert not R.march_mismatches(rev, dict(want, active=swap)), name


def test_c_the_events_are_crossings_roots():
    """The march's roots are crossings_restatement.all_roots' (unclipped: the widest range), and every t a march ends at short of
    t_max lies between two consecutive events, in a medium."""
    for name in ("two_overlap", "row64", "moving", "negative_radius"):
        c = I.BY_NAME[name]
        n = len(c["rays"])
        has, s0, s1 = R.roots(c["recs"], c["objects"], c["rays"])
        wide = np.stack([np.full(n, -INF), np.full(n, INF)], axis=1)
        allr = X.all_roots(c["recs"], c["rays"], wide)
        for m, j in enumerate(c["objects"]):
            fin = has[:, m] & np.isfinite(s0[:, m]) & np.isfinite(s1[:, m])
            assert np.array_equal(R.bits(allr[fin, 2 * j]), R.bits(s0[fin, m])) and np.array_equal(R.bits(allr[fin, 2 * j + 1]), R.bits(s1[fin, m]))
            assert (np.isinf(allr[~has[:, m], 2 * j])).all()
        a = I.answer(c)
        col = a["status"] == 1
        for i in np.nonzero(col)[0]:
            inside = [m for m in range(len(c["objects"])) if has[i, m] and s0[i, m] <= a["t"][i] <= s1[i, m]]
            assert inside, (name, i)


# ---- the restated mutants: which inputs tell them apart ----------------------------------------------------------------------------

MUTANT_CASES = {"s0_strict": "edges", "rem_le": "edges", "rho_descending": "nested3", "shift32": "row64", "no_rho_guard": "one",
                "skip_s1": "two_overlap", "no_clamp": "clamp"}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_d_each_mutant_is_told_apart_by_a_named_case(variant):
    c = I.BY_NAME[MUTANT_CASES[variant]]
    assert R.march_mismatches(I.answer(c, variant=variant), I.answer(c)), variant
    if variant == "s0_strict":
        row = I.EDGE_ROWS["on_boundary"]
        assert I.answer(c, variant=variant)["depth"][row] != I.answer(c)["depth"][row]
    if variant == "rem_le":
        row = I.EDGE_ROWS["tau_equals_step"]
        assert I.answer(c, variant=variant)["status"][row] == 1 and I.answer(c)["status"][row] == 0


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_e_the_entries_are_declared_bound_and_built(tor):
    src = open(os.path.join(ROOT, "include", "tor_media.h")).read()
    render = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    assert '#include "tor_media.h"' in render and render.index('#include "tor_photons.h"') < render.index('#include "tor_media.h"')
    L = tor.lib()
    assert tor.MEDIA_SYMBOLS == ["tor_scene_media", "tor_media_march_device", "tor_media_march_host", "tor_media_scatter_device",
                                 "tor_media_scatter_host", "tor_rng_uniform_device", "tor_rng_uniform_host"]
    for name in tor.MEDIA_SYMBOLS:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_media.h"
        assert hasattr(L, name) and getattr(L, name).argtypes == tor._signatures()[name]
        assert name not in tor.EXPORTED_SYMBOLS
    assert sorted(tor.MEDIA_SYMBOLS) == sorted(set(re.findall(r"TOR_API\s+int\s+(tor_\w+)\s*\(", src)))
    assert re.search(r"#define TOR_MEDIA_MAX 64\b", src) and tor.MEDIA_MAX == R.MEDIA_MAX == 64
    assert re.search(r"#define TOR_UNIFORM_MAX_DRAWS 16\b", src) and tor.UNIFORM_MAX_DRAWS == 16
    assert (tor.MEDIA_REFUSED, tor.MEDIA_ESCAPED, tor.MEDIA_COLLIDED) == (R.REFUSED, R.ESCAPED, R.COLLIDED)
    for name in ("set_media", "march_media", "scatter_media", "uniform", "transmittance", "trace_media"):
        assert callable(getattr(tor.Context, name))
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert mk.count("tor_media.hip") == 2 and mk.count("tor_media.h ") == 1          # SRCS and ASM_SRCS; HDRS
    assert "-ffp-contract=off" in mk
    for word in ("(0.0, +inf)", "2 * n_media + 1", "rem < step", "Termination", "random_unit_vector"):
        assert word in src, word
    for fn in ("log", "exp", "atan2"):                                               # the library takes neither
        assert not re.search(r"\b(__builtin_|std::|::)?" + fn + r"[a-z0-9]*\s*\(", open(os.path.join(
            ROOT, "trace-of-radiance_amd", "csrc", "tor_media.hip")).read().split("#include <hip/hip_runtime.h>")[1]), fn


def test_e_refusals_that_need_no_device(tor):
    """The checks that come before any device work, in the header's order; nothing is written.  (None of them reads the context, so a
    non-NULL pointer stands in for one; the refusals that do -- no scene, no table, the table's own -- are in the GPU suite.)"""
    L = tor.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.cast((C.c_char * 64)(), C.c_void_p)
    err = lambda: L.tor_last_error().decode()
    assert L.tor_scene_media(None, 1, p, p, p) == -1 and "tor_scene_media: ctx is NULL" in err()
    for f, tail, name in ((L.tor_media_march_device, (None,), "tor_media_march_device"), (L.tor_media_march_host, (), "tor_media_march_host")):
        assert f(None, 1, p, p, p, None, 1, p, p, p, p, p, *tail) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, None, None, None, -1, None, None, None, None, None, *tail) == -1 and "n_rays < 0" in err()
        assert f(ctx, 1, None, None, None, None, -1, None, None, None, None, None, *tail) == -1 and "n_list < 0" in err()
        assert f(ctx, 2, None, None, None, None, 1, None, None, None, None, None, *tail) == -1 and "without a list" in err()
        for hole in range(6):                                                        # rays, tau, status, t, depth, active
            a = [p] * 6
            a[hole] = None
            assert f(ctx, 1, a[0], None, a[1], None, 1, a[2], a[3], a[4], a[5], None, *tail) == -1 and "NULL rays, tau" in err(), hole
    for f, tail, name in ((L.tor_media_scatter_device, (None,), "tor_media_scatter_device"), (L.tor_media_scatter_host, (), "tor_media_scatter_host")):
        assert f(None, 1, p, p, p, p, None, 1, p, p, *tail) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, None, None, None, None, -1, None, None, *tail) == -1 and "n_rays < 0" in err()
        assert f(ctx, 1, None, None, None, None, None, -1, None, None, *tail) == -1 and "n_list < 0" in err()
        assert f(ctx, 2, None, None, None, None, None, 1, None, None, *tail) == -1 and "without a list" in err()
        for hole in range(6):                                                        # rays, t, active, rng, rays_out, att
            a = [p] * 6
            a[hole] = None
            assert f(ctx, 1, a[0], a[1], a[2], a[3], None, 1, a[4], a[5], *tail) == -1 and "NULL rays, t, active" in err(), hole
    for f, tail, name in ((L.tor_rng_uniform_device, (None,), "tor_rng_uniform_device"), (L.tor_rng_uniform_host, (), "tor_rng_uniform_host")):
        assert f(None, 1, p, None, 1, 1, p, *tail) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, None, -1, 0, None, *tail) == -1 and "n_rays < 0" in err()
        assert f(ctx, 1, None, None, -1, 0, None, *tail) == -1 and "n_list < 0" in err()
        assert f(ctx, 2, None, None, 1, 0, None, *tail) == -1 and "without a list" in err()      # the list before n_draws
        for k in (0, -1, 17):
            assert f(ctx, 1, None, None, 1, k, None, *tail) == -1 and "n_draws must be" in err()  # n_draws before the NULLs
        assert f(ctx, 1, None, None, 1, 16, p, *tail) == -1 and "NULL rng or out" in err()
        assert f(ctx, 1, p, None, 1, 1, None, *tail) == -1 and "NULL rng or out" in err()
    assert all(v == 0.0 for v in buf)


# ---- Python glue on a recording library -----------------------------------------------------------------------------------------------

class _Recorder:
    """A stand-in for the loaded library (the pattern of tests/test_photon_query.py): every tor_* entry records (name, args) and
    returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("tor_"):
            raise AttributeError(name)
        if name == "tor_last_note":
            return lambda: b"media march: 2 media"
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
        ctx.set_media([3, 1], [0.5, 2.0], [[1, 0, 0], [0, 1, 0]])
        ctx.set_media([], [])
        (n0, a0), (n1, a1), (n2, a2) = rec.calls
        assert n0 == n1 == n2 == "tor_scene_media" and a0[1] == 2 and a0[4] == 0 and a1[4] not in (0, 16) and a2[1] == 0
        for bad in (lambda: ctx.set_media([1], [1.0, 2.0]), lambda: ctx.set_media([1, 2], [1.0, 2.0], [[1, 1, 1]])):
            with pytest.raises(ValueError):
                bad()
        rec = tor._lib = _Recorder()
        m = ctx.march_media(rays, 1.5)
        (name, a), = rec.calls
        assert name == "tor_media_march_host" and a[0] == 16 and a[1] == 5 and a[2] == rays.ctypes.data and a[3] == 0 and a[5] == 0 and a[6] == 5
        assert a[7:12] == (m.status.ctypes.data, m.t.ctypes.data, m.depth.ctypes.data, m.active.ctypes.data, m.rho.ctypes.data)
        assert m.status.dtype == np.int32 and m.active.dtype == np.int64 and m.mode == "2 media" and m.t.shape == (5,)
        rec = tor._lib = _Recorder()
        again = ctx.march_media(rays, np.arange(5.0), t_range=np.zeros((5, 2)), index=[4, 0], out=m)
        (name, a), = rec.calls
        assert a[3] != 0 and a[5] not in (0, 16) and a[6] == 2 and again.t is m.t
        with pytest.raises(ValueError):
            ctx.march_media(rays, np.zeros(4))
        with pytest.raises(ValueError):
            ctx.march_media(rays, 1.0, out=tor.MediaMarch(*(np.zeros(4),) * 5, ""))
        with pytest.raises(ValueError):
            ctx.march_media(rays, None)
        rec = tor._lib = _Recorder()
        st = np.arange(20, dtype=np.uint64).reshape(5, 4)
        new, att = sc = ctx.scatter_media(rays, m, st, index=[1])
        (name, a), = rec.calls
        assert name == "tor_media_scatter_host" and a[2] == rays.ctypes.data and a[3] == m.t.ctypes.data and a[4] == m.active.ctypes.data
        assert a[5] == sc.rng.ctypes.data != st.ctypes.data and a[7] == 1 and a[8] == new.ctypes.data and a[9] == att.ctypes.data
        assert new.shape == (5, 7) and att.shape == (5, 3) and sc.rays is new and sc.attenuation is att
        rec = tor._lib = _Recorder()
        ctx.scatter_media(rays, (np.zeros(5), np.zeros(5, dtype=np.int64)), st, out=sc)
        assert rec.calls[0][1][8] == new.ctypes.data
        with pytest.raises(ValueError):
            ctx.scatter_media(rays, (np.zeros(4), np.zeros(5, dtype=np.int64)), st)
        rec = tor._lib = _Recorder()
        u, after = ctx.uniform(st, 3, index=[0, 2])
        (name, a), = rec.calls
        assert name == "tor_rng_uniform_host" and a[1] == 5 and a[2] == after.ctypes.data != st.ctypes.data and a[4] == 2 and a[5] == 3
        assert a[6] == u.ctypes.data and u.shape == (5, 3) and after.dtype == np.uint64 and np.array_equal(after, st)
        for bad in (lambda: ctx.uniform(st, 0), lambda: ctx.uniform(st, 17), lambda: ctx.uniform(st.astype(np.float64), 1),
                    lambda: ctx.uniform(st[:, :3], 1), lambda: ctx.uniform(st, 2, out=np.zeros((5, 3)))):
            with pytest.raises(ValueError):
                bad()
        rec = tor._lib = _Recorder()
        tm = ctx.transmittance(np.zeros((3, 3)), np.ones((3, 3)), time=0.5)
        (name, a), = rec.calls
        assert name == "tor_media_march_host" and a[1] == 3 and a[3] != 0 and (tm == 1.0).all()      # exp(-0) of the recorder's zeros
    finally:
        tor._lib = saved
        ctx._h = C.c_void_p()


# ---- the physics checks hold for the definition ------------------------------------------------------------------------------------------

def test_g_physics_on_the_restatement(oracle):
    rays, _ = I.physics_rays(4096, 31)
    u, _ = R.uniforms(oracle, I.states(4096, 8), 1)
    m = R.march(I.PHYSICS_RECS, [0], [0.5], rays, -np.log1p(-u[:, 0]))
    frac = float((m["status"] == 1).mean())
    print(f"collision fraction {frac:.4f}, expected {I.PHYSICS_P:.4f}: {(frac - I.PHYSICS_P) / (I.PHYSICS_TOL / 5):+.2f} standard errors")
    assert abs(I.PHYSICS_TOL - 0.0377) < 1e-4 and abs(frac - I.PHYSICS_P) <= I.PHYSICS_TOL
    rays, b = I.physics_rays(4096, 32, b_max=0.9)
    m = R.march(I.PHYSICS_RECS, [0], [0.75], rays, INF)
    want = 0.75 * 2.0 * np.sqrt(1.0 - b * b)
    rel = np.abs(m["depth"] - want) / want
    print(f"largest relative error of the depth against the chord: {rel.max():.3e}")
    assert rel.max() <= 1e-9
