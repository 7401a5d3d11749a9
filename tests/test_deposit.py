"""Exact sample deposits without a GPU: tor_deposit_device is declared, exported and bound with a matching signature, every refusal
answers TOR_ERR_INVALID_ARGUMENT with its reason in the documented order, and the restatement the GPU tests compare against
(tests/deposit_restatement.py: a float64 and an integer statement of the definition) is held to hand-worked cases and to its
invariance under permutation.  Last, the inputs of tests/test_gpu_deposit.py (tests/deposit_inputs.py) are shown to mean
something, from the restatement alone.

Every floor of MEASURED is half of what the committed generator gave (seed 5, max_value = 1); the measured value stands in the
table."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import deposit_inputs as I
import deposit_restatement as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -36
# share: (measured, floor = measured / 2)
MEASURED = {"in_run": (0.5822, 0.2911), "rejected": (0.014886, 0.007443), "outside": (0.024674, 0.012337), "ties": (0.16808, 0.08404)}


def _err(tor):
    return tor.lib().tor_last_error().decode()


def test_new_symbol_is_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    name = "tor_deposit_device"
    assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
    assert name in tor.EXPORTED_SYMBOLS
    decl = re.search(r"TOR_API\s+int\s+" + name + r"\s*\(([^;]*)\);", src).group(1)
    assert len(decl.split(",")) == len(L.tor_deposit_device.argtypes) == 13
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "ctx", "n", "d_color", "d_pixel", "d_index", "n_index", "max_value", "npix", "d_sums", "d_moments", "d_counts", "d_rejected",
        "hip_stream"]
    kw = inspect.signature(tor.Context.deposit).parameters
    assert list(kw) == ["self", "colors", "pixels", "sums", "moments", "counts", "index", "max_value", "rejected"]
    assert kw["max_value"].default == 1.0 and kw["moments"].default is None and kw["rejected"].default is None
    fk = inspect.signature(tor.Film.__init__).parameters
    assert list(fk)[:8] == ["self", "ctx", "nrows", "ncols", "moments", "counts", "max_value", "device"]
    assert fk["moments"].default is False and fk["counts"].default is False and fk["max_value"].default == 1.0
    for m in ("deposit", "add_pass", "image", "noise", "state", "from_state", "rejected", "check_budget"):
        assert callable(getattr(tor.Film, m)), m
    assert list(inspect.signature(tor.Film.add_pass).parameters) == ["self", "cam", "k", "tracer", "chunk_pixels"]
    assert list(inspect.signature(tor.Film.deposit).parameters) == ["self", "pixels", "colors", "index"]
    assert tor.DEPOSIT_MAX_VALUE == D.MAX_VALUE == 128.0
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*tor_deposit\.hip", mk, re.M) and re.search(r"^ASM_SRCS = .*tor_deposit\.hip", mk, re.M)


def test_refusals_need_no_device_and_come_in_order(tor):
    L = tor.lib()
    b = C.c_void_p(16)  # never dereferenced: every call below fails its checks, or has nothing to do, before any device work
    fn = L.tor_deposit_device

    def call(ctx=b, n=4, color=b, pixel=b, index=None, n_index=0, max_value=1.0, npix=8, sums=b):
        return fn(ctx, n, color, pixel, index, n_index, max_value, npix, sums, None, None, None, None)

    def refused(word, **kw):
        rc = call(**kw)
        msg = _err(tor)
        assert rc == tor.ERR_INVALID_ARGUMENT, (word, kw, rc)
        assert msg.startswith("tor_deposit_device:") and word in msg, (word, msg)

    refused("ctx is NULL", ctx=None)
    refused("n < 0 or n_index < 0", n=-1)
    refused("n < 0 or n_index < 0", index=b, n_index=-1)
    refused("n < 0 or n_index < 0", n_index=-5)
    for kw in (dict(color=None), dict(pixel=None), dict(sums=None), dict(index=b, n_index=2, sums=None)):
        refused("NULL color, pixel or sums", **kw)
    for npix in (0, -1, -2 ** 40):
        refused("npix < 1", npix=npix)
    for mv in (0.0, -0.0, -1.0, math.nan, math.inf, -math.inf, np.nextafter(128.0, math.inf), 129.0, 1e300):
        refused("max_value must lie in (0, 128]", max_value=mv)
    # the documented order: the counts, then the arrays, then npix, then max_value
    refused("n < 0 or n_index < 0", n=-1, color=None, npix=0, max_value=math.nan)
    refused("NULL color, pixel or sums", color=None, npix=0, max_value=math.nan)
    refused("npix < 1", npix=0, max_value=math.nan)
    refused("max_value", max_value=math.nan)
    # nothing to do is no error, whatever the arrays: n == 0, and a list with n_index == 0 -- but the other checks still hold
    assert call(n=0, color=None, pixel=None, sums=None) == tor.OK
    assert call(index=b, n_index=0, color=None, pixel=None, sums=None) == tor.OK
    refused("npix < 1", n=0, npix=0)
    refused("max_value", index=b, n_index=0, max_value=200.0)
    # the largest and a tiny clamp are accepted
    assert call(n=0, max_value=128.0) == tor.OK and call(n=0, max_value=5e-324) == tor.OK


def test_context_deposit_and_film_reject_bad_arguments_before_the_library(tor):
    import torch
    ctx = object.__new__(tor.Context)  # a context whose creation never happened (no device here)
    ctx._h = C.c_void_p()
    with pytest.raises(ValueError, match="colors must be an .n, 3. float64 CUDA tensor"):
        ctx.deposit(torch.zeros((4, 3), dtype=torch.float64), torch.zeros(4, dtype=torch.int32), torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="colors must be"):
        ctx.deposit(np.zeros((4, 3)), np.zeros(4, dtype=np.int32), np.zeros((2, 3)))
    for mv in (0.0, -1.0, 128.5, math.nan):
        with pytest.raises(tor.TorError, match="max_value"):
            tor.Film(ctx, 4, 4, max_value=mv)


def _one(colors, pixels=None, npix=4, **kw):
    colors = np.array(colors, dtype=np.float64).reshape(-1, 3)
    pixels = np.zeros(len(colors), dtype=np.int32) if pixels is None else pixels
    return D.agree(colors, pixels, npix, **kw)


def test_hand_worked_values():
    # ties (j + 0.5) * 2^-36 round to even
    for j in range(12):
        want = (j if j % 2 == 0 else j + 1) * U
        r = _one([[(j + 0.5) * U, 0.0, 0.0]])
        assert r["sums"][0, 0] == want and r["counts"][0] == 1
    assert D.quantize36(0.49999 * U) == 0.0 and D.quantize36(0.50001 * U) == U and D.quantize36(1.25 * U) == U
    # -0.0 is accepted and deposits +0.0; a denormal is accepted and deposits 0
    r = _one([[-0.0, -0.0, -0.0], [5e-324, 2.0 ** -1030, 0.0]])
    assert r["rejected"] == 0 and r["counts"][0] == 2 and not D.bits(r["sums"]).any() and not D.bits(r["moments"]).any()
    # the clamp: max_value exactly, its successor, a huge value
    for mv in (0.25, 1.0, 4.0, 128.0):
        r = _one([[mv, np.nextafter(mv, np.inf), 1e300]], max_value=mv)
        assert (r["sums"][0] == mv).all() and (r["moments"][0] == mv * mv).all() and r["rejected"] == 0
        r = _one([[np.nextafter(mv, 0.0), 0.5 * mv, np.finfo(np.float64).max]], max_value=mv)
        assert r["sums"][0, 0] == mv and r["sums"][0, 1] == 0.5 * mv and r["sums"][0, 2] == mv   # (the predecessor rounds up to mv)
    # the moments are taken from the QUANTISED value: q = 2^-36 * round(c * 2^36), then quantize36(q * q)
    c = 0.3 + 0.4 * U
    q = round(c * 2.0 ** 36) * U
    r = _one([[c, 0.0, 0.0]])
    assert r["sums"][0, 0] == q and r["moments"][0, 0] == round(q * q * 2.0 ** 36) * U
    c = 100.0 + 0.4 * U                           # q = 100, q * q = 10000; the unquantised square would be 10000 + 80 units
    r = _one([[c, 0.0, 0.0]], max_value=128.0)
    assert r["sums"][0, 0] == 100.0 and r["moments"][0, 0] == 10000.0 and D.quantize36(c * c) == 10000.0 + 80 * U
    # one bad channel rejects the whole sample: nothing deposited, counted once
    for bad in (math.nan, math.inf, -math.inf, -1.0, -5e-324, -1e-300):
        for ch in range(3):
            col = [0.5, 0.25, 0.125]
            col[ch] = bad
            r = _one([col, [0.5, 0.5, 0.5]])
            assert r["rejected"] == 1 and r["counts"][0] == 1 and (r["sums"][0] == 0.5).all(), (bad, ch)
    assert _one([[math.nan, -1.0, math.inf]])["rejected"] == 1
    # pixels outside the film deposit nothing and are not counted, not even as rejected
    r = _one([[0.5, 0.5, 0.5], [math.nan, 0, 0], [0.25, 0.25, 0.25], [1, 1, 1]], pixels=np.array([-1, 4, I.INT32_MIN, 3], dtype=np.int32))
    assert r["rejected"] == 0 and r["counts"].tolist() == [0, 0, 0, 1] and r["sums"].sum() == 3.0
    # lists: out of range skipped, repeats deposit again, an empty list deposits nothing; buffers are added to, never cleared
    cols, pix = [[0.5, 0, 0], [0.25, 0, 0], [math.nan, 0, 0]], np.array([1, 2, 2], dtype=np.int32)
    r = _one(cols, pix, index=[1, 1, -1, 3, 0, 2, 2])
    assert r["sums"][:, 0].tolist() == [0, 0.5, 0.5, 0] and r["counts"].tolist() == [0, 1, 2, 0] and r["rejected"] == 2
    r2 = _one(cols, pix, index=[], into=r)
    assert not D.mismatches(r2, r)
    r3 = _one(cols, pix, into=r)
    assert r3["sums"][:, 0].tolist() == [0, 1.0, 0.75, 0] and r3["counts"].tolist() == [0, 2, 3, 0] and r3["rejected"] == 3


def test_the_restatement_asserts_the_exactness_bound():
    with pytest.raises(AssertionError, match="exactness bound"):
        D.deposit(np.full((9, 3), 128.0), np.zeros(9, dtype=np.int32), 1, max_value=128.0)      # 9 * 2^14 > 2^17
    D.agree(np.full((7, 3), 128.0), np.zeros(7, dtype=np.int32), 1, max_value=128.0)
    with pytest.raises(AssertionError):
        D.deposit(np.ones((1, 3)), np.zeros(1, dtype=np.int32), 1, max_value=129.0)


@pytest.mark.parametrize("max_value", I.MAX_VALUES)
def test_permutation_and_split_invariance_of_the_restatement(max_value):
    rng = np.random.default_rng(3)
    for name in I.CASES:
        c, p = I.case(name, max_value)
        want = D.agree(c, p, I.NPIX, max_value)
        for _ in range(3):
            o = rng.permutation(I.N)
            assert not D.mismatches(D.agree(c[o], p[o], I.NPIX, max_value), want), name
        cut = int(rng.integers(1, I.N))
        half = D.agree(c[:cut], p[:cut], I.NPIX, max_value)
        assert not D.mismatches(D.agree(c[cut:], p[cut:], I.NPIX, max_value, into=half), want), name
        assert not D.mismatches(D.agree(c, p, I.NPIX, max_value, index=rng.permutation(I.N)), want), name
    for name, idx in I.list_cases().items():
        c, p = I.case("runs", max_value)
        keep = idx[(idx >= 0) & (idx < I.N)]
        assert not D.mismatches(D.agree(c, p, I.NPIX, max_value, index=idx), D.agree(c[keep], p[keep], I.NPIX, max_value)), name


def test_the_gpu_inputs_mean_something():
    assert I.N == 64 * 9 + 37 and I.N > 2 * 256 and sum(I.RUN_LENGTHS) < I.N
    got = I.shares(1.0)
    print("measured shares:", {k: round(v, 4) for k, v in got.items()})
    for k, (measured, floor) in MEASURED.items():
        assert abs(floor - measured / 2) < 1e-3, k
        assert got[k] >= floor, (k, got[k], floor)
    # the runs case really holds its runs, aligned so that they cross a lane-64 and the workgroup-256 boundary
    _, p = I.case("runs", 1.0)
    at = 0
    for m, ln in enumerate(I.RUN_LENGTHS):
        assert (p[at:at + ln] == m * 7 + 3).all() and (at == 0 or p[at - 1] != p[at])
        at += ln
    assert 195 < 256 < 195 + 300 and 3 < 64 < 66
    # A B A B: no two neighbours share a pixel, yet lanes two apart do
    _, p = I.case("abab", 1.0)
    assert (p[1:] != p[:-1]).all() and (p[2:] == p[:-2]).all()
    # A A B B: runs of two, and four lanes on the same pixel again in another run
    _, p = I.case("aabb", 1.0)
    assert (p[0:I.N - 1:2] == p[1::2]).all() and (p[2:] != p[:-2]).all() and (p[4:] == p[:-4]).all()
    # the rejects case: heads, middles, tails and whole runs between two runs of one pixel
    c, p = I.case("rejects", 1.0)
    with np.errstate(invalid="ignore"):
        bad = (np.isnan(c) | np.isinf(c) | (c < 0)).any(axis=1)
    assert bad[0] and bad[24 + 11] and bad[48 + 23] and bad[72 + 8:72 + 16].all() and not bad[72 + 7] and p[72 + 7] == p[72 + 16]
    assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any() and ((c < 0) & np.isfinite(c)).any()
    # every max_value's cases hold values at, above and below the clamp, and stay inside the bound (the restatement asserts it)
    for mv in I.MAX_VALUES:
        c, p = I.case("values", mv)
        assert (c == mv).any() and (c > mv).any() and ((c < mv) & (c > 0)).any() and (np.signbit(c) & (c == 0)).any()
        for name in I.CASES:
            D.agree(*I.case(name, mv), I.NPIX, mv)
    e = I.case("edges", 1.0)[1]
    assert (e == -1).any() and (e == I.NPIX).any() and (e == I.INT32_MIN).any()
