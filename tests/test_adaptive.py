"""Adaptive sampling without a GPU: the three entry points are declared, exported and bound, every argument check that needs
no device answers TOR_ERR_INVALID_ARGUMENT, Adaptive refuses pixel seeding and bad host lists, and the numpy restatement of
the convergence test is the documented formula."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tor_render_accumulate_list_device", "tor_adaptive_select_device", "tor_resolve_counts_device")


def _err(tor):
    return tor.lib().tor_last_error().decode()


def test_new_symbols_are_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in NEW:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
        assert name in tor.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    for meth in ("accumulate_list_device", "adaptive_select_device", "resolve_counts_device"):
        assert callable(getattr(tor.Context, meth))
    for meth in ("step", "run", "counts", "image", "to_canvas", "state", "from_state", "validate_list"):
        assert callable(getattr(tor.Adaptive, meth))
    assert L.tor_version() == b"tor_mi355x 0.6 (gfx950)"


def test_accumulate_list_rejects_without_a_device(tor):
    L, cam, opt = tor.lib(), tor.camera(), tor.make_options(seeding=tor.SEED_SAMPLE)
    buf = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    for first, n in ((-1, 4), (0, 0), ((1 << 17) - 4, 5)):
        rc = L.tor_render_accumulate_list_device(None, C.byref(cam), 8, 8, buf, 4, first, n, 50, C.byref(opt), buf, buf, None)
        assert rc == tor.ERR_INVALID_ARGUMENT and "2^17" in _err(tor), (first, n)
    rc = L.tor_render_accumulate_list_device(None, C.byref(cam), 8, 8, buf, -1, 0, 4, 50, C.byref(opt), buf, buf, None)
    assert rc == tor.ERR_INVALID_ARGUMENT and "n_list" in _err(tor)
    rc = L.tor_render_accumulate_list_device(None, C.byref(cam), 8, 8, buf, 65, 0, 4, 50, C.byref(opt), buf, buf, None)
    assert rc == tor.ERR_INVALID_ARGUMENT and "above the shard's 64 pixels" in _err(tor)
    shard = tor.make_options(seeding=tor.SEED_SAMPLE, shard_index=1, shard_count=2, row_tile=1)  # rows 1, 3, 5, 7: 32 pixels
    rc = L.tor_render_accumulate_list_device(None, C.byref(cam), 8, 8, buf, 33, 0, 4, 50, C.byref(shard), buf, buf, None)
    assert rc == tor.ERR_INVALID_ARGUMENT and "above the shard's 32 pixels" in _err(tor)
    for args in ((None, buf, buf, buf), (buf, None, buf, buf), (buf, buf, None, buf), (buf, buf, buf, None)):
        ctx, lst, sums, mom = args
        rc = L.tor_render_accumulate_list_device(ctx, C.byref(cam), 8, 8, lst, 4, 0, 4, 50, C.byref(opt), sums, mom, None)
        assert rc == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)


def test_select_and_resolve_counts_reject_without_a_device(tor):
    L = tor.lib()
    b = C.c_void_p(16)
    n = C.c_int32(-5)
    sel = L.tor_adaptive_select_device
    for n_in, total, at, rt in ((-1, 8, 0.0, 0.1), (4, 1, 0.0, 0.1), (4, 0, 0.0, 0.1), (4, (1 << 17) + 1, 0.0, 0.1),
                                (4, 8, -1e-9, 0.1), (4, 8, 0.0, -0.5), (4, 8, math.nan, 0.1), (4, 8, 0.0, math.nan)):
        assert sel(b, b, b, b, n_in, total, at, rt, C.c_void_p(32), b, C.byref(n), None) == tor.ERR_INVALID_ARGUMENT, (n_in, total, at, rt)
    sel(b, b, b, b, 4, 1, 0.0, 0.1, C.c_void_p(32), b, C.byref(n), None)
    assert "two samples" in _err(tor)
    assert sel(None, b, b, b, 4, 8, 0.0, 0.1, C.c_void_p(32), b, C.byref(n), None) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
    assert sel(b, b, b, b, 4, 8, 0.0, 0.1, C.c_void_p(32), b, None, None) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
    assert sel(b, b, b, C.c_void_p(32), 4, 8, 0.0, 0.1, C.c_void_p(32), b, C.byref(n), None) == tor.ERR_INVALID_ARGUMENT
    assert "alias" in _err(tor)
    assert n.value == -5  # nothing was written
    rc = L.tor_resolve_counts_device
    assert rc(None, b, b, 4, 2.2, b, None) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
    assert rc(b, b, None, 4, 2.2, b, None) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
    assert rc(b, b, b, -1, 2.2, b, None) == tor.ERR_INVALID_ARGUMENT


def test_context_methods_raise_on_a_null_context(tor):
    ctx = object.__new__(tor.Context)  # a context whose creation never happened (no device here)
    ctx._h = C.c_void_p()
    cam, opt = tor.camera(), tor.make_options(seeding=tor.SEED_SAMPLE)
    for call in (lambda: ctx.accumulate_list_device(cam, 8, 8, 16, 4, 0, 4, 50, opt, 16, 16),
                 lambda: ctx.adaptive_select_device(16, 16, 16, 4, 8, 0.0, 0.1, 32, 16),
                 lambda: ctx.resolve_counts_device(16, 16, 4, 2.2, 16)):
        with pytest.raises(tor.TorError) as e:
            call()
        assert e.value.code == tor.ERR_INVALID_ARGUMENT and "NULL" in str(e.value)


def test_adaptive_refuses_pixel_seeding_and_bad_policy(tor):
    with pytest.raises(tor.TorError) as e:
        tor.Adaptive(None, tor.camera(), 8, 8, 50, tor.make_options(seeding=tor.SEED_PIXEL))
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "SEED_SAMPLE" in str(e.value)
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    for kw in ({"abs_tol": -1.0}, {"rel_tol": math.nan}, {"min_samples": 1}, {"pass_samples": 0}, {"max_samples": (1 << 17) + 1}):
        with pytest.raises(tor.TorError) as e:
            tor.Adaptive(None, tor.camera(), 8, 8, 50, opt, **kw)
        assert e.value.code == tor.ERR_INVALID_ARGUMENT, kw


@pytest.mark.parametrize("bad", [[3, 2, 5], [1, 4, 4, 9], [-1, 3], [0, 64], [0.5, 2.0], [[1, 2]]])
def test_adaptive_refuses_bad_host_lists(tor, bad):
    with pytest.raises(tor.TorError) as e:
        tor.Adaptive.validate_list(np.array(bad), 64)
    assert e.value.code == tor.ERR_INVALID_ARGUMENT
    # ... and a checkpoint carrying one is refused before any device work
    state = {"samples": 16, "list": np.array(bad), "sums": None, "moments": None, "counts": None}
    with pytest.raises(tor.TorError):
        tor.Adaptive.from_state(None, tor.camera(), 8, 8, 50, tor.make_options(seeding=tor.SEED_SAMPLE), state)


def test_adaptive_accepts_good_host_lists(tor):
    assert tor.Adaptive.validate_list(np.array([], dtype=np.int64), 64).dtype == np.int32
    got = tor.Adaptive.validate_list([0, 5, 17, 63], 64)
    assert got.dtype == np.int32 and got.tolist() == [0, 5, 17, 63]


def _scalar_active(S, M, n, abs_tol, rel_tol):
    """The documented test, one channel at a time with Python floats (IEEE float64, one rounding per operation)."""
    for c in range(3):
        mean = S[c] / n
        var = (M[c] - S[c] * S[c] / n) / (n - 1)
        se = math.sqrt(max(0.0, var) / n)
        if not se <= abs_tol + rel_tol * mean:
            return True
    return False


def test_numpy_restatement_is_the_documented_formula(tor):
    rng = np.random.default_rng(7)
    npix, n = 4000, 48
    q = np.round(rng.random((n, npix, 3)) ** rng.uniform(0.5, 8.0, size=(1, npix, 1)) * 2.0 ** 36) / 2.0 ** 36  # samples in [0, 1], 2^-36 grid
    q[:, :200] = rng.choice([0.25, 0.5, 0.75, 1.0], size=(1, 200, 3))  # constant pixels whose squares lie on the grid: zero variance
    q[:, 200:220] = 0.0       # black pixels
    S = q.sum(axis=0)
    M = (np.round(q * q * 2.0 ** 36) / 2.0 ** 36).sum(axis=0)
    pix = np.sort(rng.choice(npix, size=npix // 2, replace=False))
    pix = np.concatenate((np.arange(220), pix[pix >= 220]))
    for abs_tol, rel_tol in ((0.0, 0.05), (1e-3, 0.0), (2e-3, 0.02), (0.0, 0.0)):
        got = tor.adaptive_select_host(S, M, pix, n, abs_tol, rel_tol)
        want = [int(p) for p in pix if _scalar_active(S[p], M[p], n, abs_tol, rel_tol)]
        assert got.dtype == np.int32 and got.tolist() == want, (abs_tol, rel_tol)
        assert 0 < len(want) < len(pix) or (abs_tol, rel_tol) == (0.0, 0.0)
    # zero variance converges even at zero tolerance (se = 0 <= 0); black pixels too
    assert set(tor.adaptive_select_host(S, M, np.arange(220), n, 0.0, 0.0).tolist()) == set()
    # the boundary is inclusive: se == abs_tol converges, the next float64 below does not
    S1, M1 = np.array([[4.0, 4.0, 4.0]]), np.array([[3.0, 3.0, 3.0]])
    se = math.sqrt(max(0.0, (3.0 - 4.0 * 4.0 / 8) / 7) / 8)
    assert tor.adaptive_select_host(S1, M1, [0], 8, se, 0.0).tolist() == []
    assert tor.adaptive_select_host(S1, M1, [0], 8, np.nextafter(se, 0.0), 0.0).tolist() == [0]
