"""The photon-map queries without a GPU: the numpy restatement of include/tor_photons.h (tests/photon_restatement.py), which the GPU
suite holds the kernels to bit for bit, is checked here against hand-worked cases, against its integer twin and against the
header's invariances; the coverage proof of the 27 cells is tried on adversarial pairs; the entries are declared, bound and
exported and refuse what the header says, in its order; build_photons and gather_photons run against a recording stand-in for
the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import photon_inputs as I
import photon_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the inputs hold what they were made for --------------------------------------------------------------------------------

def test_a_inputs_cover_their_classes():
    got = I.assert_coverage()          # (also: the restated 27-cell walk equals brute force on every case)
    print(got)
    counts = sorted(len(c["position"]) for c in I.CASES)
    assert {0, 1, 63, 64, 65, 257}.issubset(counts) and counts[-1] >= 5000
    m = I.stored(I.BY_NAME["collide40"])
    assert m["n_buckets"] == 128 and len(m["position"]) == 40 and len({tuple(c) for c in m["cell"]}) == 40
    far = np.abs(m["cell"][:, None, :] - m["cell"][None, :, :]).max(axis=2)
    assert (far[~np.eye(40, dtype=bool)] > 2).all()                       # far apart: no two of them are neighbours
    assert len(set(m["bucket"].tolist())) < 40                            # ... and some share a bucket
    assert I.stored(I.BY_NAME["one_cell"])["largest"] == 300
    assert I.stored(I.BY_NAME["dense0"])["n_buckets"] == 16 and I.stored(I.BY_NAME["dense0"])["largest"] == 0


# ---- hand-worked cases ------------------------------------------------------------------------------------------------------

def test_b_cell_and_bucket_by_hand():
    h = R.cell_size(0.25)
    assert h == 0.25 + 0.25 * 2.0 ** -20 and R.cell_size(1.0) == 1.0 + 2.0 ** -20
    c = R.cells([[0.0, -0.0, 0.1], [-1e-9, h, -h], [2.5 * h, -2.5 * h, np.nextafter(h, 0.0)]], h)
    assert c.tolist() == [[0.0, 0.0, 0.0], [-1.0, 1.0, -1.0], [2.0, -3.0, 0.0]]           # floor, not truncation
    assert [R.n_buckets(n) for n in (0, 1, 8, 9, 40, 64, 65, 2 ** 25, 2 ** 25 + 1, 2 ** 30)] == \
        [16, 16, 16, 32, 128, 128, 256, 2 ** 26, 2 ** 26, 2 ** 26]
    # the hash in Python integers: (uint32)(-1) = 0xFFFFFFFF, products wrap
    want = ((0xFFFFFFFF * 73856093) & 0xFFFFFFFF) ^ ((2 * 19349663) & 0xFFFFFFFF) ^ (((-3) & 0xFFFFFFFF) * 83492791 & 0xFFFFFFFF)
    assert int(R.bucket([[-1, 2, -3]], 1 << 20)[0]) == want & ((1 << 20) - 1)
    assert int(R.bucket([[0, 0, 0]], 16)[0]) == 0 and int(R.bucket([[1, 0, 0]], 16)[0]) == 73856093 & 15


def test_b_gather_by_hand():
    """One photon at distance 1/8 of a query with R = 1/4: w = 1 - (1/64) / (1/16) = 3/4."""
    m = R.store([[0.125, 0.0, 0.0]], [[0.5, 2.0, 2.0 ** -37]], [[0.0, 0.0, -1.0]], 0.25)
    x = [[0.0, 0.0, 0.0]]
    g = R.agree(m, x, kernel="epanechnikov")
    assert g["count"].tolist() == [1] and g["sums"].tolist() == [[0.375, 1.0, 0.0]]       # 2 * 3/4 clamped to 1; 0.75 * 2^-37 -> 0
    g = R.agree(m, x, kernel="constant", max_value=128.0)
    assert g["sums"].tolist() == [[0.5, 2.0, 0.0]]                                        # the tie 2^-37 rounds to even: 0
    g = R.agree(m, x, kernel="constant", max_value=0.25)
    assert g["sums"].tolist() == [[0.25, 0.25, 0.0]]
    up, side = [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0]]
    assert R.agree(m, x, up)["count"].tolist() == [1] and R.agree(m, x, side)["count"].tolist() == [0]      # dir . n == 0 rejects
    assert R.agree(m, x, [[0.0, 0.0, -1.0]])["count"].tolist() == [0] and R.agree(m, x, [[np.nan, 0, 1]])["count"].tolist() == [0]
    assert R.agree(m, x, radius=[0.125])["count"].tolist() == [0]                         # d2 == r2 rejects
    assert R.agree(m, x, radius=[np.nextafter(0.125, 1.0)])["count"].tolist() == [1]
    for r, n in ((0.0, 0), (-1.0, 0), (np.nan, 0), (np.inf, 1), (100.0, 1)):
        assert R.agree(m, x, radius=[r])["count"].tolist() == [n], r
    # unlisted points keep what `into` holds; listed ones are overwritten, zeros included
    into = {"sums": np.full((2, 3), 7.0), "count": np.array([5, 6], dtype=np.int32)}
    g = R.agree(m, [[0.0, 0.0, 0.0], [9.0, 9.0, 9.0]], index=[1, 5, -1], into=into)
    assert g["sums"].tolist() == [[7.0, 7.0, 7.0], [0.0, 0.0, 0.0]] and g["count"].tolist() == [5, 0]


def test_b_store_by_hand():
    c = I.BY_NAME["specials"]
    m = I.stored(c)
    assert R.info(m) == {"stored": 8, "dropped": 5, "n_buckets": 32, "largest_bucket": 8}
    assert np.signbit(m["power"][2, 0]) and m["power"][2, 0] == 0.0                       # -0.0 passes
    e = I.stored(I.BY_NAME["range_edge"])
    assert R.info(e)["stored"] == 5 and R.info(e)["dropped"] == 3
    assert np.abs(e["cell"]).max(axis=1).tolist() == [2 ** 30] * 5                        # (floor(-(2^30 - 0.1)) = -2^30)
    li = I.BY_NAME["listed"]
    ml = I.stored(li)
    assert len(ml["position"]) == 73 and ml["n_buckets"] == 256 and ml["dropped"] == 0    # 78 list slots: 5 skipped, not counted
    assert (ml["position"][-3:] == li["position"][3]).all()                               # a repeated entry is stored again


# ---- invariances ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dense65", "one_cell", "specials", "listed", "range_edge"])
def test_c_invariant_under_permutation_and_split(name):
    c = I.BY_NAME[name]
    rng = np.random.default_rng(7)
    for kernel in ("constant", "epanechnikov"):
        for mv in (0.25, 1.0, 128.0):
            m = I.stored(c)
            want = R.agree(m, c["points"], c["normals"], c["radius"], kernel, mv)
            n = len(c["position"])
            perm = rng.permutation(n)
            index = None
            if c["index"] is not None:      # the same list, in the permuted numbering (entries out of range stay out of range)
                old = c["index"].astype(np.int64)
                index = np.where((old >= 0) & (old < n), np.argsort(perm)[np.clip(old, 0, n - 1)], -1)
            mp = R.store(c["position"][perm], c["power"][perm], None if c["direction"] is None else c["direction"][perm], c["R"], index)
            assert not R.mismatches(R.agree(mp, c["points"], c["normals"], c["radius"], kernel, mv), want)
            # the queries split into two calls through lists, each writing into the other's result
            k = len(c["points"])
            first = rng.permutation(k)[: k // 2]
            rest = np.setdiff1d(np.arange(k), first)
            half = R.agree(m, c["points"], c["normals"], c["radius"], kernel, mv, index=first)
            both = R.agree(m, c["points"], c["normals"], c["radius"], kernel, mv, index=rest, into=half)
            assert not R.mismatches(both, want)


def test_c_answer_does_not_depend_on_the_bucket_count():
    c = I.BY_NAME["dense257"]
    m = I.stored(c)
    want, _ = R.walk(m, c["points"], c["normals"])
    for nb in (16, 1 << 20):
        m2 = dict(m, n_buckets=nb, bucket=R.bucket(m["cell"], nb))
        got, _ = R.walk(m2, c["points"], c["normals"])
        assert not R.mismatches(got, want)


# ---- the coverage proof, tried -----------------------------------------------------------------------------------------------

def test_d_the_27_cells_hold_every_accepted_photon():
    """~10^5 adversarial (photon, query) pairs per radius: the photon anywhere in range, the query at a distance just around R
    along an axis, a diagonal or a random direction, and at offsets of one ulp; every pair the brute-force test accepts must have
    cells that differ by at most 1 on every axis, and the query's quotient must lie below 2^30 + 3."""
    rng = np.random.default_rng(2024)
    n = 100000
    total = 0
    for radius in (0.25, 1.0, 3.0, 1e-3, 7.3e5, 2.0 ** -500, 1.0 / 3.0):
        Rr = np.float64(radius)
        h = R.cell_size(Rr)
        scale = np.where(rng.random(n) < 0.5, 2.0 ** 30, 10.0 ** rng.uniform(-3, 9, n)).clip(max=2.0 ** 30)
        k = np.rint((rng.random((n, 3)) * 2 - 1) * scale[:, None])                      # a cell ...
        frac = rng.choice([0.0, 1.0, 0.5, 1e-9, 1 - 1e-9, 2.0 ** -30], size=(n, 3)) * (rng.random((n, 3)) < 0.7) + \
            rng.random((n, 3)) * 1e-3
        p = (k + np.minimum(frac, 1.0)) * h                                             # ... and a place in it, faces preferred
        d = rng.normal(size=(n, 3))
        d[: n // 3] = np.sign(d[: n // 3]) * (rng.random((n // 3, 3)) < 0.5)            # axes and diagonals
        norm = np.sqrt((d * d).sum(axis=1))
        d = d / np.where(norm > 0, norm, 1.0)[:, None]
        dist = Rr * (1.0 - rng.choice([0.0, 2.0 ** -52, 2.0 ** -40, 2.0 ** -21, 2.0 ** -20, 1e-3, 0.3], size=n))
        x = p + d * dist[:, None]
        x = np.where(rng.random((n, 3)) < 0.3, np.nextafter(x, np.where(rng.random((n, 3)) < 0.5, np.inf, -np.inf)), x)
        cp, cx = R.cells(p, h), R.cells(x, h)
        stored = (np.abs(cp) <= R.CELL_MAX).all(axis=1)
        e = p - x
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        acc = stored & (d2 < Rr * Rr)
        total += int(acc.sum())
        assert (np.abs(cp[acc] - cx[acc]) <= 1.0).all(), radius
        assert (np.abs(x[acc] / h) < R.CELL_MAX + 3).all(), radius
        assert (np.abs(e[acc]) < Rr).all(), radius                                       # step 1 of the proof: no slack at all
    assert total >= 100000, total


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

def test_e_the_entries_are_declared_bound_and_exported(tor):
    src = open(os.path.join(ROOT, "include", "tor_photons.h")).read()
    render = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    assert '#include "tor_photons.h"' in render and "tor_photons_" not in re.sub(r"/\*.*?\*/", "", render, flags=re.S)
    L = tor.lib()
    assert tor.PHOTON_SYMBOLS == ["tor_photons_build_device", "tor_photons_build_host", "tor_photons_gather_device",
                                  "tor_photons_gather_host", "tor_photons_info"]
    for name in tor.PHOTON_SYMBOLS:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_photons.h"
        assert hasattr(L, name) and getattr(L, name).argtypes == tor._signatures()[name]
        assert name not in tor.EXPORTED_SYMBOLS
    assert sorted(tor.PHOTON_SYMBOLS) == sorted(set(re.findall(r"TOR_API\s+int\s+(tor_\w+)\s*\(", src)))
    assert tor.PHOTON_KERNELS == R.KERNELS == {"constant": 0, "epanechnikov": 1}
    assert re.search(r"TOR_PHOTON_KERNEL_CONSTANT = 0, TOR_PHOTON_KERNEL_EPANECHNIKOV = 1", src)
    for name in ("build_photons", "gather_photons", "photons_info", "trace_photons", "trace_photon_map"):
        assert callable(getattr(tor.Context, name))
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert mk.count("tor_photons.hip") == 2 and mk.count("tor_photons.h ") == 1        # SRCS and ASM_SRCS; HDRS
    assert "-ffp-contract=off" in mk
    for word in ("27 neighbouring cells", "2^17", "73856093u", "quantize36"):
        assert word in src


def test_e_refusals_that_need_no_device(tor):
    """The checks that come before any device work, in the header's order; nothing is written.  (None of them reads the context, so
    a non-NULL pointer stands in for one; the refusals that do -- no map built, normals without directions -- are in the GPU suite.)"""
    L = tor.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.cast((C.c_char * 64)(), C.c_void_p)
    err = lambda: L.tor_last_error().decode()
    bd, bh = L.tor_photons_build_device, L.tor_photons_build_host
    for f, tail in ((bd, (None,)), (bh, ())):
        name = "tor_photons_build_device" if f is bd else "tor_photons_build_host"
        assert f(None, 1, p, p, p, None, 1, 0.25, *tail) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, None, None, None, 5, float("nan"), *tail) == -1 and "< 0" in err()             # counts before the list
        assert f(ctx, 1, None, None, None, None, -1, float("nan"), *tail) == -1 and "< 0" in err()
        assert f(ctx, 2 ** 30 + 1, None, None, None, None, 2 ** 30 + 1, 0.25, *tail) == -1 and "above 2^30" in err()
        assert f(ctx, 2, None, None, None, None, 1, float("nan"), *tail) == -1 and "without a list" in err()   # the list before the radius
        for bad in (0.0, -0.25, float("nan"), float("inf"), 1.7976931348623157e308):                         # (the largest double: h overflows)
            assert f(ctx, 1, None, None, None, None, 1, bad, *tail) == -1 and "radius" in err(), bad           # the radius before the NULLs
        assert f(ctx, 1, None, p, p, None, 1, 0.25, *tail) == -1 and "NULL position or power" in err()
        assert f(ctx, 1, p, None, p, None, 1, 0.25, *tail) == -1 and "NULL position or power" in err()
    gd, gh = L.tor_photons_gather_device, L.tor_photons_gather_host
    for f, tail in ((gd, (None,)), (gh, ())):
        name = "tor_photons_gather_device" if f is gd else "tor_photons_gather_host"
        assert f(None, 1, p, None, None, None, 1, 1, 1.0, p, p, *tail) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, None, None, None, -1, 7, 0.0, None, None, *tail) == -1 and "n_list" not in err()   # n before n_list
        assert f(ctx, 1, None, None, None, None, -1, 7, 0.0, None, None, *tail) == -1 and "n_list < 0" in err()
        assert f(ctx, 2, None, None, None, None, 1, 7, 0.0, None, None, *tail) == -1 and "without a list" in err()
        for k in (-1, 2, 7):
            assert f(ctx, 1, None, None, None, None, 1, k, 0.0, None, None, *tail) == -1 and "kernel must be" in err()   # before max_value
        for mv in (0.0, -1.0, 128.5, float("nan"), float("inf")):
            assert f(ctx, 1, None, None, None, None, 1, 1, mv, None, None, *tail) == -1 and "max_value" in err(), mv   # before the NULLs
        for hole in range(3):
            a = [p] * 3
            a[hole] = None
            assert f(ctx, 1, a[0], None, None, None, 1, 0, 1.0, a[1], a[2], *tail) == -1 and "NULL point, sums or count" in err()
    assert L.tor_photons_info(None, p) == -1 and "ctx is NULL" in err()
    assert L.tor_photons_info(ctx, None) == -1 and "out is NULL" in err()
    assert all(v == 0.0 for v in buf)


# ---- Python glue on a mocked context ------------------------------------------------------------------------------------------

def test_f_photon_gather_irradiance_and_budget(tor):
    sums = np.array([[0.5, 0.25, 0.0], [0.0, 0.0, 0.0]])
    count = np.array([3, 0], dtype=np.int32)
    g = tor.PhotonGather(sums, count, 0.25, 0.5, 1, 1.0, "photons gather")
    want = sums / 0.25 * 2.0 / (np.pi * 0.25) / 1000.0
    assert np.allclose(g.irradiance(1000), want, rtol=1e-15) and (g.irradiance(1000)[1] == 0).all()
    g0 = tor.PhotonGather(sums, count, 4.0, np.array([0.5, np.nan]), 0, 1.0, "photons gather")
    assert np.allclose(g0.irradiance(10), sums / 4.0 / (np.pi * 0.25) / 10.0, rtol=1e-15)
    assert g.check_budget() == 3 and g.budget() == 2 ** 17 - 1
    big = tor.PhotonGather(sums, np.array([1024, 0], dtype=np.int32), 1.0, 0.5, 1, 128.0, "")
    assert big.budget() == 1023
    with pytest.raises(tor.TorError):
        big.check_budget()
    assert tor.PhotonGather(sums, np.array([1023, 0], dtype=np.int32), 1.0, 0.5, 1, 128.0, "").check_budget() == 1023


class _Recorder:
    """A stand-in for the loaded library (the pattern of tests/test_query_glue.py): every tor_* entry records (name, args, the
    float64 words behind the addresses in `peek`) and returns 0."""

    def __init__(self, peek):
        self.calls, self.peek = [], peek

    def __getattr__(self, name):
        if not name.startswith("tor_"):
            raise AttributeError(name)
        if name == "tor_last_note":
            return lambda: b"photons: recorded"
        if name == "tor_last_error":
            return lambda: b""

        def entry(*args):
            args = tuple((a.value or 0) if isinstance(a, C.c_void_p) else a for a in args)
            seen = {pos: np.frombuffer((C.c_char * (8 * words)).from_address(args[pos]), dtype=np.float64).copy()
                    for pos, words in self.peek.items() if args[pos] not in (0, 16)}
            self.calls.append((name, args, seen))
            return 0
        return entry


def test_f_python_glue_on_a_recording_library(tor):
    """build_photons and gather_photons on numpy operands without a GPU and without the library: the entry reached, every
    scalar, the power scale (exact, the largest finite channel into (1/2, 1]), NULL for absent arrays, and what PhotonGather keeps.
    (trace_photons and trace_photon_map step through the device whatever their operands are: their bookkeeping is checked in
    tests/test_gpu_photon_query.py.)"""
    ctx = object.__new__(tor.Context)
    ctx._h = C.c_void_p(16)
    saved = tor._lib
    pos = np.arange(12, dtype=np.float64).reshape(4, 3)
    pw = np.array([[3.0, 0.5, 0.0], [np.nan, 1.0, 2.0], [np.inf, 0.25, 6.0], [-1.0, 0.0, 0.125]])
    try:
        rec = tor._lib = _Recorder({3: 12})
        pm = ctx.build_photons(pos, pw, radius=0.5, index=[2, 0, 7])
        (name, a, seen), = rec.calls
        assert name == "tor_photons_build_host" and a[0] == 16 and a[1] == 4 and a[4] == 0 and a[5] not in (0, 16) and a[6] == 3 and a[7] == 0.5
        assert pm.scale == 0.125 and pm.radius == 0.5 and ctx._photon_scale == 0.125          # 6.0 = 0.75 * 2^3 -> 2^-3
        want = pw * 0.125
        assert np.array_equal(R.bits(seen[3][~np.isnan(seen[3])]), R.bits(want.reshape(-1)[~np.isnan(want.reshape(-1))]))
        assert np.array_equal(pw[0], [3.0, 0.5, 0.0])                                          # the caller's array is not written
        for top, scale in ((1.0, 1.0), (0.5, 2.0), (0.75, 1.0), (1.0000001, 0.5), (2.0 ** -40, 2.0 ** 40), (0.0, 1.0)):
            tor._lib = _Recorder({})
            assert ctx.build_photons(pos, np.full((4, 3), top), pos, radius=1.0).scale == scale, top
        rec = tor._lib = _Recorder({})
        pts = np.zeros((5, 3))
        g = ctx.gather_photons(pts, radius=[0.25, 2.0, -1.0, np.nan, 1.0], kernel="constant", max_value=0.5)
        (name, a, _), = rec.calls
        assert name == "tor_photons_gather_host" and a[1] == 5 and a[3] == 0 and a[4] != 0 and a[5] == 0 and a[6] == 5
        assert a[7] == 0 and a[8] == 0.5 and a[9] == g.sums.ctypes.data and a[10] == g.count.ctypes.data
        assert g.scale == 1.0 and g.kernel == 0 and g.max_value == 0.5 and g.sums.shape == (5, 3) and g.count.dtype == np.int32
        assert g.radius[:3].tolist() == [0.25, 1.0, -1.0] and g.radius[4] == 1.0               # min(radius, R) as the library takes it
        rec = tor._lib = _Recorder({})
        again = ctx.gather_photons(pts, normals=pts, index=np.array([4, 1]), out=g)
        (name, a, _), = rec.calls
        assert a[3] != 0 and a[4] == 0 and a[5] not in (0, 16) and a[6] == 2 and a[7] == 1 and a[8] == 1.0 and again.sums is g.sums
        assert again.radius == 1.0
        rec = tor._lib = _Recorder({})
        with pytest.raises(ValueError):
            ctx.gather_photons(pts, out=tor.PhotonGather(np.zeros((4, 3)), np.zeros(4, dtype=np.int32), 1.0, 1.0, 1, 1.0, ""))
        with pytest.raises(ValueError):
            ctx.gather_photons(pts, normals=np.zeros((4, 3)))
        with pytest.raises(KeyError):
            ctx.gather_photons(pts, kernel="gaussian")
        with pytest.raises(ValueError):
            ctx.build_photons(pos, pw)
        assert rec.calls == []
    finally:
        tor._lib = saved
        ctx._h = C.c_void_p()
