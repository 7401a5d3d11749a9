"""The definition of tor_deposit_device (include/tor_render.h), restated twice in numpy -- what tests/test_gpu_deposit.py compares
the kernel with, bit for bit, and what tests/test_deposit.py holds to hand-worked cases.

  deposit()      float64: the quantiser as (x + 98304.0) - 98304.0, the sums with np.add.at (sequential, in entry order)
  deposit_int()  integers: rint(min(c, max_value) * 2^36) summed as int64, then scaled back by 2^-36 -- no float64 sum at all

Both assert that what they were given lies within the exactness bound (every sum below 2^17, every q * q below 2^15), so inputs
that pass are inside the bound by the reference statement alone; agree() asserts that the two statements give the same bits."""
import numpy as np

BIAS = 98304.0          # 1.5 * 2^16: ulp(x + BIAS) = 2^-36 for 0 <= x < 2^15
UNIT = 2.0 ** -36
SUM_BOUND = 2.0 ** 17
MAX_VALUE = 128.0


def quantize36(x):
    x = np.asarray(x, dtype=np.float64)
    return (x + BIAS) - BIAS


def _entries(n, index):
    if index is None:
        return np.arange(n, dtype=np.int64)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    return index[(index >= 0) & (index < n)]      # a listed entry outside [0, n) is skipped; a repeated one stays


def _select(colors, pixels, npix, max_value, index):
    """(clamped colours, pixels) of the accepted samples in deposit order, and the number of rejected ones."""
    assert 0.0 < max_value <= MAX_VALUE
    colors = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    pixels = np.asarray(pixels).reshape(-1).astype(np.int64)
    assert len(pixels) == len(colors)
    e = _entries(len(colors), index)
    c, p = colors[e], pixels[e]
    inside = (p >= 0) & (p < npix)                # a pixel outside the film: nothing deposited, nothing counted
    with np.errstate(invalid="ignore"):
        bad = (np.isnan(c) | np.isinf(c) | (c < 0.0)).any(axis=1)   # (-0.0 < 0.0 is false: accepted)
    ok = inside & ~bad
    return np.minimum(c[ok], max_value), p[ok], int((inside & bad).sum())


def _start(into, npix):
    if into is None:
        return (np.zeros((npix, 3)), np.zeros((npix, 3)), np.zeros(npix, dtype=np.int32), 0)
    return (np.array(into["sums"], dtype=np.float64).reshape(npix, 3), np.array(into["moments"], dtype=np.float64).reshape(npix, 3),
            np.array(into["counts"], dtype=np.int32).reshape(npix), int(into["rejected"]))


def deposit(colors, pixels, npix, max_value=1.0, index=None, into=None):
    """{"sums" (npix, 3), "moments" (npix, 3), "counts" (npix,) int32, "rejected" int}: `into` (a result of an earlier call; None:
    zeros) plus the deposit, in float64."""
    c, p, rej = _select(colors, pixels, npix, max_value, index)
    sums, moments, counts, rejected = _start(into, npix)
    q = quantize36(c)
    qq = q * q                                    # one rounding
    assert (qq < 2.0 ** 15).all(), "q * q leaves quantize36's exact range"
    np.add.at(sums, p, q)
    np.add.at(moments, p, quantize36(qq))
    np.add.at(counts, p, 1)
    assert sums.max(initial=0.0) < SUM_BOUND and moments.max(initial=0.0) < SUM_BOUND, "the inputs exceed the exactness bound"
    return {"sums": sums, "moments": moments, "counts": counts, "rejected": rejected + rej}


def deposit_int(colors, pixels, npix, max_value=1.0, index=None, into=None):
    """deposit() in integers: multiples of 2^-36 as int64, summed as int64, scaled back at the end."""
    c, p, rej = _select(colors, pixels, npix, max_value, index)
    sums, moments, counts, rejected = _start(into, npix)
    si, mi = np.rint(sums * 2.0 ** 36).astype(np.int64), np.rint(moments * 2.0 ** 36).astype(np.int64)
    assert np.array_equal(si * UNIT, sums) and np.array_equal(mi * UNIT, moments), "the starting sums are no multiples of 2^-36"
    qi = np.rint(c * 2.0 ** 36).astype(np.int64)  # (the scaling is exact: a power of two, no overflow after the clamp)
    q = qi.astype(np.float64) * UNIT              # exact: |qi| <= 2^43
    qq = q * q
    assert (qq < 2.0 ** 15).all(), "q * q leaves quantize36's exact range"
    np.add.at(si, p, qi)
    np.add.at(mi, p, np.rint(qq * 2.0 ** 36).astype(np.int64))
    np.add.at(counts, p, 1)
    assert si.max(initial=0) < 2 ** 53 and mi.max(initial=0) < 2 ** 53, "the inputs exceed the exactness bound"
    return {"sums": si.astype(np.float64) * UNIT, "moments": mi.astype(np.float64) * UNIT, "counts": counts, "rejected": rejected + rej}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def mismatches(got, want, fields=("sums", "moments", "counts", "rejected")):
    """The fields of two results that differ in any bit (float fields compared as int64 words: -0.0 is not 0.0)."""
    bad = []
    for f in fields:
        if f == "rejected":
            same = int(got[f]) == int(want[f])
        elif f == "counts":
            same = np.array_equal(np.asarray(got[f]).reshape(-1), np.asarray(want[f]).reshape(-1))
        else:
            same = np.array_equal(bits(got[f]).reshape(-1), bits(want[f]).reshape(-1))
        if not same:
            bad.append(f)
    return bad


def agree(colors, pixels, npix, max_value=1.0, index=None, into=None):
    """deposit(), after asserting that deposit_int() gives the same bits."""
    a = deposit(colors, pixels, npix, max_value, index, into)
    b = deposit_int(colors, pixels, npix, max_value, index, into)
    assert not mismatches(a, b), f"the two statements of the deposit disagree: {mismatches(a, b)}"
    return a
