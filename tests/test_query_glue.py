"""The Python query glue without a GPU and without the library: Context.hit, radiance, bounce, scatter, occluded, crossings and
nearest on numpy operands against a recording stand-in for the loaded library.  What is held, literally: which entry of the C ABI
a call reaches and with how many arguments, every scalar, what every address points at (NULL, a non-NULL list, the very array the
result exposes, or a copy of the caller's values), the time range for finite, partly infinite and all-NaN times, the result's
shapes, dtypes, initial contents and mode, who owns the arrays a step writes, and that a refused call raises before any entry runs.
Last, the ctypes signature of every exported symbol against a literal copy."""
import ctypes as C
import importlib
import math
import types

import numpy as np
import pytest

H = 16            # the context handle every call must pass on
INF, NAN = math.inf, math.nan
ALL = 0xFFFFFFFF


class Recorder:
    """Every tor_* attribute records (name, args) and returns 0.  `peek` maps an argument's position to the (shape, dtype) of the
    array behind it: read at call time, while the caller's temporaries are alive."""

    def __init__(self, note):
        self.calls, self.seen, self.peek, self.note = [], {}, {}, note

    def __getattr__(self, name):
        if not name.startswith("tor_"):
            raise AttributeError(name)
        if name == "tor_last_note":
            return lambda: self.note
        if name == "tor_last_error":
            return lambda: b""

        def entry(*args):
            args = tuple((a.value or 0) if isinstance(a, C.c_void_p) else a for a in args)
            self.calls.append((name, args))
            for pos, (shape, dtype) in self.peek.items():
                if pos < len(args) and args[pos] not in (0, 16) and int(np.prod(shape)):
                    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
                    self.seen[pos] = np.frombuffer((C.c_char * nbytes).from_address(args[pos]), dtype=dtype).reshape(shape).copy()
            return 0
        return entry


@pytest.fixture(scope="module")
def tor():
    return importlib.import_module("trace-of-radiance_amd")


@pytest.fixture
def glue(tor):
    """(ctx, run): run(note, method, peek, *a, **kw) -> (result, entry name, its arguments, the arrays seen behind `peek`)."""
    ctx = object.__new__(tor.Context)
    ctx._h = C.c_void_p(H)
    saved = tor._lib

    def run(note, method, peek, *a, **kw):
        rec = tor._lib = Recorder(note)
        rec.peek = peek
        try:
            res = getattr(ctx, method)(*a, **kw)
        finally:
            tor._lib = saved
        assert len(rec.calls) == 1, rec.calls
        name, args = rec.calls[0]
        assert args[0] == H
        return res, name, args, rec.seen

    def refused(exc, method, *a, worded=True, **kw):
        rec = tor._lib = Recorder(b"")
        try:
            with pytest.raises(exc) as e:
                getattr(ctx, method)(*a, **kw)
        finally:
            tor._lib = saved
        assert rec.calls == [], (method, rec.calls)
        if exc is ValueError and worded:
            assert str(e.value).startswith(f"Context.{method}:"), str(e.value)
    yield types.SimpleNamespace(run=run, refused=refused)
    tor._lib = saved
    ctx._h = C.c_void_p()                                     # (nothing for __del__ to destroy)


def _rays(n, cols=7, times=None):
    a = (np.arange(n * cols, dtype=np.float64).reshape(n, cols) + 1.0) / 8.0
    if times is not None:
        a[:, cols - 1] = times
    return a


def _states(n):
    return (np.arange(n * 4, dtype=np.uint64).reshape(n, 4) << np.uint64(40)) + np.uint64(0x8000000000000001)


def _addr(a):
    return a.ctypes.data


INDEXES = (None, [], [4, 1, 9])
MASKS = (None, 0x5, "u32", "i32")
MODES = (("auto", 0), ("brute", 1), ("blocks", 2))


def _mask(kind, n):
    """(the mask to pass, the words the library must see, the scalar word)"""
    if kind is None or isinstance(kind, int):
        return kind, None, (ALL if kind is None else kind)
    if kind == "u32":
        w = (np.arange(n, dtype=np.uint32) * np.uint32(0x01010101)) | np.uint32(0x80000000)
        return w, w, 0
    w = np.arange(n, dtype=np.int32) - 2                      # the first word is -2: 0xFFFFFFFE by its bits
    return w, w.view(np.uint32), 0


def _check_list(index, n, p_list, n_list, seen_list):
    if index is None:
        assert (p_list, n_list) == (0, n)
    elif not index:
        assert p_list != 0 and n_list == 0                    # an empty list is a list
    else:
        assert p_list not in (0, 16) and n_list == 3 and seen_list.tolist() == [4, 1, 9] and seen_list.dtype == np.int32


def _check_mask(kind, n, p_mask, word, seen):
    _, words, want_word = _mask(kind, n)
    assert word == want_word
    if words is None:
        assert p_mask == 0
    else:
        assert p_mask != 0
        if n:
            assert seen.dtype == np.uint32 and np.array_equal(seen, words)
            if kind == "i32":
                assert int(seen[0]) == 0xFFFFFFFE


def _listed_mode(n, index):
    return "blocks" if n and (index is None or index) else "nothing to do"


@pytest.mark.parametrize("n", (0, 1, 5))
@pytest.mark.parametrize("mask", MASKS)
def test_hit(glue, n, mask):
    rays = _rays(n)
    for with_range, (mode, m), time_range in ((False, MODES[0], None), (True, MODES[1], (0.25, 0.75)), (True, MODES[2], None)):
        t_range = np.tile([0.5, 2.5], (n, 1)) if with_range else None
        mk, _, _ = _mask(mask, n)
        peek = {2: ((n, 7), np.float64), 3: ((n, 2), np.float64), 8: ((n,), np.uint32)}
        res, name, a, seen = glue.run(b"hit: blocks", "hit", peek, rays, t_range, time_range, mode, mask=mk)
        assert name == ("tor_hit_host" if mask is None else "tor_hit_masked_host") and len(a) == (8 if mask is None else 10)
        assert a[1] == n and a[6] == m
        lo, hi = time_range if time_range else ((rays[:, 6].min(), rays[:, 6].max()) if n else (0.0, 0.0))
        assert (a[4], a[5]) == (lo, hi) and type(a[4]) is float and type(a[5]) is float
        if n == 0:
            assert a[2] == a[3] == a[7] == 0                  # an empty numpy call passes NULL for every array
        else:
            assert np.array_equal(seen[2], rays) and a[7] == _addr(res.raw)
            assert (a[3] == 0) if t_range is None else np.array_equal(seen[3], t_range)
        if mask is not None:
            _check_mask(mask, n, a[8], a[9], seen.get(8))
        assert res.raw.shape == (n, 8) and res.raw.dtype == np.float64 and not res.raw.any()
        assert res.p.shape == (n, 3) and res.normal.shape == (n, 3) and res.t.shape == (n,)
        assert res.object.shape == (n,) and res.object.dtype == np.int32 and res.front_face.shape == (n,)
        assert (n == 0 or np.shares_memory(res.object, res.raw)) and res.mode == "blocks"      # hit always takes the library's note


@pytest.mark.parametrize("times, want", (
    ([0.5, -1.0, 2.0, 0.25, 0.0], (-1.0, 2.0)),
    ([INF, 0.5, -INF, NAN, 0.125], (0.125, 0.5)),
    ([NAN] * 5, (0.0, 0.0)),
    ([INF, -INF, NAN, INF, NAN], (0.0, 0.0)),
))
def test_time_range_none_is_the_finite_min_and_max(glue, times, want):
    rays, pts, st = _rays(5, times=times), _rays(5, 4, times=times), _states(5)
    for note, method, pos, a in ((b"hit: blocks", "hit", 4, (rays,)), (b"radiance: blocks", "radiance", 5, (rays, st)),
                                 (b"bounce: blocks", "bounce", 6, (rays, st)), (b"occluded: blocks", "occluded", 6, (rays,)),
                                 (b"crossings: blocks", "crossings", 9, (rays, 2)), (b"nearest: blocks", "nearest", 9, (pts, 2))):
        _, _, args, _ = glue.run(note, method, {}, *a)
        assert (args[pos], args[pos + 1]) == want, (method, args[pos], args[pos + 1])
        _, _, args, _ = glue.run(note, method, {}, *a, time_range=(np.float32(0.5), 3))
        assert (args[pos], args[pos + 1]) == (0.5, 3.0) and type(args[pos + 1]) is float, method


@pytest.mark.parametrize("n", (0, 1, 5))
def test_radiance(glue, n):
    rays, st = _rays(n), _states(n)
    st_before = st.copy()
    for (mode, m), depth, states in ((MODES[0], 50, st), (MODES[2], 7, st.view(np.int64))):
        peek = {2: ((n, 7), np.float64), 3: ((n, 4), np.uint64)}
        (color, out, ran), name, a, seen = glue.run(b"radiance: blocks", "radiance", peek, rays, states, depth, (0.0, 1.0), mode)
        assert name == "tor_radiance_host" and len(a) == 9
        assert a[1] == n and a[4] == depth and (a[5], a[6]) == (0.0, 1.0) and a[7] == m
        assert color.shape == (n, 3) and color.dtype == np.float64 and not color.any() and ran == "blocks"
        assert out.shape == (n, 4) and out.dtype == np.uint64 and np.array_equal(out, st_before)
        assert not np.shares_memory(out, st) and np.array_equal(st, st_before)     # the states are copied, the caller's left alone
        if n == 0:
            assert a[2] == a[3] == a[8] == 0
        else:
            assert np.array_equal(seen[2], rays) and a[3] == _addr(out) and a[8] == _addr(color)


@pytest.mark.parametrize("n", (0, 1, 5))
@pytest.mark.parametrize("index", INDEXES)
def test_bounce_and_scatter(glue, tor, n, index):
    rays, st = _rays(n), _states(n)
    rays_before, st_before = rays.copy(), st.copy()
    hits = np.arange(n * 8, dtype=np.float64).reshape(n, 8)
    prev = {}
    for step, ((mode, m), out_kind) in enumerate(zip(MODES, ("fresh", "reused", "misfit"))):
        for method in ("bounce", "scatter"):
            out = {"fresh": None, "reused": prev.get(method), "misfit": prev.get(method + " misfit")}[out_kind]
            if method == "bounce":
                peek = {2: ((n, 7), np.float64), 3: ((n, 4), np.uint64), 4: ((3,), np.int32)}
                res, name, a, seen = glue.run(b"bounce: blocks", "bounce", peek, rays, st, index, (0.0, 1.0), mode, out)
                assert name == "tor_bounce_host" and len(a) == 12 and a[1] == n
                assert (a[6], a[7], a[8]) == (0.0, 1.0, m)
                p_list, n_list, outs = a[4], a[5], (a[9], a[10], a[11])
                assert res.mode == _listed_mode(n, index)
            else:
                peek = {2: ((n, 7), np.float64), 3: ((n, 8), np.float64), 4: ((n, 4), np.uint64), 5: ((3,), np.int32)}
                given = hits if step != 1 else tor.HitResult(hits, hits.view(np.int32), "hit: blocks")
                res, name, a, seen = glue.run(b"unused", "scatter", peek, rays, given, st, index, out)
                assert name == "tor_scatter_host" and len(a) == 9 and a[1] == n
                p_list, n_list, outs = a[5], a[6], (None, a[7], a[8])
                assert res.mode == "scatter" and np.array_equal(res.raw, hits)
            _check_list(index, n, p_list, n_list, seen.get(4 if method == "bounce" else 5))
            # the step's own copies of the rays and the states are what the library updates and the result carries
            assert np.array_equal(res.rays, rays_before) and np.array_equal(res.rng, st_before) and res.rng.dtype == np.uint64
            assert not np.shares_memory(res.rays, rays) and not np.shares_memory(res.rng, st)
            assert res.raw.shape == (n, 8) and res.attenuation.shape == (n, 3) and res.attenuation.dtype == np.float64
            assert res.status.shape == (n,) and res.status.dtype == np.int32 and res.object.shape == (n,)
            if n == 0:                                        # an empty numpy call passes NULL for every array
                assert a[2] == a[3] == a[4 if method == "scatter" else 9] == outs[1] == outs[2] == 0
            else:
                assert a[2] == _addr(res.rays) and np.array_equal(seen[2], rays_before)
                assert a[3 if method == "bounce" else 4] == _addr(res.rng)
                assert outs[1] == _addr(res.attenuation) and outs[2] == _addr(res.status)
                assert outs[0] in (None, _addr(res.raw))
                if method == "scatter":
                    assert np.array_equal(seen[3], hits)
            if out_kind == "reused":
                assert res.attenuation is prev[method].attenuation and res.status is prev[method].status
                assert method == "scatter" or res.raw is prev[method].raw
            else:                                             # fresh, or an `out` of another size: new arrays, silently
                assert not res.attenuation.any() and not res.status.any()
                if method == "bounce":
                    assert (res.object == -1).all() and not res.raw[:, :7].any() and not res.front_face.any()
                if out is not None:
                    assert res.status is not out.status and res.attenuation is not out.attenuation
            if out_kind == "fresh":
                prev[method] = res
                res.attenuation[...] = 3.0                    # (so that a reuse shows)
                bigger, _, _, _ = glue.run(b"bounce: blocks", method, {}, _rays(n + 1),
                                           *((_states(n + 1),) if method == "bounce" else (np.zeros((n + 1, 8)), _states(n + 1))))
                prev[method + " misfit"] = bigger
    assert np.array_equal(rays, rays_before) and np.array_equal(st, st_before)     # the caller's arrays, bit for bit


@pytest.mark.parametrize("n", (0, 1, 5))
@pytest.mark.parametrize("index", INDEXES)
@pytest.mark.parametrize("mask", MASKS)
def test_occluded(glue, tor, n, index, mask):
    rays = _rays(n)
    mk, _, _ = _mask(mask, n)
    first = None
    for (mode, m), with_range, out_kind in ((MODES[0], False, "fresh"), (MODES[1], True, "reused"), (MODES[2], True, "raw")):
        t_range = np.tile([0.001, 1.0], (n, 1)) if with_range else None
        out = {"fresh": None, "reused": first, "raw": first.raw if first else None}[out_kind]
        peek = {2: ((n, 7), np.float64), 3: ((n, 2), np.float64), 4: ((3,), np.int32), 10: ((n,), np.uint32)}
        res, name, a, seen = glue.run(b"occluded: blocks", "occluded", peek, rays, t_range, index, (0.0, 1.0), mode, out, mk)
        assert name == ("tor_occluded_host" if mask is None else "tor_occluded_masked_host") and len(a) == (10 if mask is None else 12)
        assert a[1] == n and (a[6], a[7], a[8]) == (0.0, 1.0, m)
        _check_list(index, n, a[4], a[5], seen.get(4))
        if mask is not None:
            _check_mask(mask, n, a[10], a[11], seen.get(10))
        if n == 0:
            assert a[2] == a[3] == a[9] == 0
        else:
            assert np.array_equal(seen[2], rays) and a[9] == _addr(res.raw)
            assert (a[3] == 0) if t_range is None else np.array_equal(seen[3], t_range)
        assert res.raw.shape == (n,) and res.raw.dtype == np.int32 and res.occluded.shape == (n,) and res.occluded.dtype == np.bool_
        assert (n == 0 or np.shares_memory(res.occluded, res.raw)) and res.mode == _listed_mode(n, index)
        if out_kind == "fresh":
            assert not res.raw.any()
            first = res
            first.raw[...] = 1
        else:
            assert res.raw is first.raw and res.occluded.all()
    for misfit in (np.zeros(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int64), tor.OccludedResult(np.zeros(n + 1, dtype=np.int32), None, "")):
        glue.refused(ValueError, "occluded", rays, out=misfit, mask=mk)


@pytest.mark.parametrize("n", (0, 1, 5))
@pytest.mark.parametrize("index", INDEXES)
@pytest.mark.parametrize("mask", MASKS)
def test_crossings(glue, n, index, mask):
    rays = _rays(n)
    mk, _, _ = _mask(mask, n)
    for k in (1, 3):
        for records in (False, True):
            first = None
            for (mode, m), with_range, out_kind in ((MODES[0], False, "fresh"), (MODES[2], True, "reused")):
                t_range = np.tile([0.5, INF], (n, 1)) if with_range else None
                peek = {2: ((n, 7), np.float64), 3: ((n, 2), np.float64), 4: ((3,), np.int32), 7: ((n,), np.uint32)}
                res, name, a, seen = glue.run(b"crossings: blocks", "crossings", peek, rays, k, t_range, index, (0.0, 1.0), mode, mk,
                                              records, first)
                assert name == "tor_crossings_host" and len(a) == 15
                assert a[1] == n and a[6] == k and (a[9], a[10], a[11]) == (0.0, 1.0, m)
                _check_list(index, n, a[4], a[5], seen.get(4))
                _check_mask(mask, n, a[7], a[8], seen.get(7))   # (mask None: NULL and 0xFFFFFFFF, the one entry serves both)
                if n == 0:
                    assert a[2] == a[3] == a[12] == a[13] == a[14] == 0
                else:
                    assert np.array_equal(seen[2], rays) and a[12] == _addr(res.raw) and a[13] == _addr(res.count)
                    assert a[14] == (_addr(res.hits) if records else 0)
                    assert (a[3] == 0) if t_range is None else np.array_equal(seen[3], t_range)
                assert res.raw.shape == (n, k, 2) and res.raw.dtype == np.float64 and res.t.shape == (n, k)
                assert res.object.shape == (n, k) and res.object.dtype == np.int32 and res.which.shape == (n, k)
                assert res.count.shape == (n,) and res.count.dtype == np.int32 and res.mode == _listed_mode(n, index)
                assert (res.hits is None) if not records else (res.hits.shape == (n, k, 8) and res.hits.dtype == np.float64)
                if out_kind == "fresh":                       # every entry unused
                    assert not res.t.any() and (res.object == -1).all() and not res.which.any() and not res.count.any()
                    if records:
                        w = res.hits.view(np.int32)
                        assert not res.hits[:, :, :7].any() and (w[:, :, 14] == -1).all() and not w[:, :, 15].any()
                    first = res
                    first.count[...] = 1
                else:
                    assert res.raw is first.raw and res.count is first.count and res.hits is first.hits and res.count.all()
            for kw in ({"k": k + 1}, {"records": not records}, {"rays": _rays(n + 1), "mask": None if mk is None or isinstance(mk, int) else 1}):
                call = {"rays": rays, "k": k, "records": records, "mask": mk, **kw}
                glue.refused(ValueError, "crossings", call["rays"], call["k"], mask=call["mask"], records=call["records"], out=first)


@pytest.mark.parametrize("n", (0, 1, 5))
@pytest.mark.parametrize("index", INDEXES)
@pytest.mark.parametrize("mask", MASKS)
def test_nearest(glue, n, index, mask):
    pts = _rays(n, 4)
    mk, _, _ = _mask(mask, n)
    per_point = np.arange(n, dtype=np.float64) + 0.5
    first = None
    for (mode, m), k, d_max, out_kind in ((MODES[0], 3, None, "fresh"), (MODES[1], 3, 2.5, "reused"), (MODES[2], 3, per_point, "reused"),
                                          (MODES[0], 1, 7, "other k")):
        peek = {2: ((n, 4), np.float64), 3: ((n,), np.float64), 4: ((3,), np.int32), 7: ((n,), np.uint32)}
        out = first if out_kind == "reused" else None
        res, name, a, seen = glue.run(b"nearest: blocks", "nearest", peek, pts, k, d_max, index, (0.0, 1.0), mode, mk, out)
        assert name == "tor_nearest_host" and len(a) == 14
        assert a[1] == n and a[6] == k and (a[9], a[10], a[11]) == (0.0, 1.0, m)
        _check_list(index, n, a[4], a[5], seen.get(4))
        _check_mask(mask, n, a[7], a[8], seen.get(7))
        if n == 0:
            assert a[2] == a[3] == a[12] == a[13] == 0
        else:
            assert np.array_equal(seen[2], pts) and a[12] == _addr(res.raw) and a[13] == _addr(res.count)
            if d_max is None:
                assert a[3] == 0
            else:                                             # a number is one limit per point
                assert seen[3].tolist() == (per_point.tolist() if d_max is per_point else [float(d_max)] * n)
        assert res.raw.shape == (n, k, 2) and res.raw.dtype == np.float64 and res.distance.shape == (n, k)
        assert res.object.shape == (n, k) and res.object.dtype == np.int32 and res.inside.shape == (n, k)
        assert res.count.shape == (n,) and res.count.dtype == np.int32 and res.mode == _listed_mode(n, index)
        if out_kind == "reused":
            assert res.raw is first.raw and res.count is first.count and res.count.all()
        else:
            assert not res.distance.any() and (res.object == -1).all() and not res.inside.any() and not res.count.any()
            if first is None:
                first = res
                first.count[...] = 1
    glue.refused(ValueError, "nearest", pts, 2, out=first, mask=mk)
    glue.refused(ValueError, "nearest", _rays(n + 1, 4), 3, out=first)


def test_refused_calls_raise_before_any_entry(glue, tor):
    """The refusal lists of tests/test_{hit,occluded,crossings,nearest}_query.py, and the steps' own."""
    r, st = np.zeros((4, 7)), np.zeros((4, 4), dtype=np.uint64)
    for rays, tr in ((np.zeros((4, 6)), None), (np.zeros(7), None), (r, np.zeros((4, 3)))):
        glue.refused(ValueError, "hit", rays, t_range=tr)
        glue.refused(ValueError, "occluded", rays, t_range=tr)
        glue.refused(ValueError, "crossings", rays, 2, t_range=tr)
    for method, a in (("hit", (r,)), ("occluded", (r,)), ("crossings", (r, 2)), ("nearest", (np.zeros((4, 4)), 2)),
                      ("radiance", (r, st)), ("bounce", (r, st))):
        glue.refused(KeyError, method, *a, mode="fastest")
    glue.refused(ValueError, "occluded", r, out=np.zeros(4, dtype=np.int64))
    glue.refused(ValueError, "occluded", r, out=np.zeros(5, dtype=np.int32))
    for k in (0, tor.CROSSINGS_MAX + 1):
        glue.refused(ValueError, "crossings", r, k)
    glue.refused(ValueError, "crossings", r, 2, out=np.zeros((4, 2, 2)))
    for pts, k, dm in ((np.zeros((4, 3)), 2, None), (np.zeros((4, 7)), 2, None), (np.zeros(4), 2, None), (np.zeros((4, 4)), 0, None),
                       (np.zeros((4, 4)), tor.NEAREST_MAX + 1, None), (np.zeros((4, 4)), 2, np.zeros(3)), (np.zeros((4, 4)), 2, np.zeros((4, 2)))):
        glue.refused(ValueError, "nearest", pts, k, max_distance=dm)
    glue.refused(ValueError, "nearest", np.zeros((4, 4)), 2, out=np.zeros((4, 2, 2)))
    for method in ("hit", "occluded"):                                             # a per-ray mask of another length, words that are no integers
        glue.refused(ValueError, method, r, mask=np.zeros(3, dtype=np.uint32))
        glue.refused(ValueError, method, r, mask=np.zeros(4), worded=False)
    glue.refused(ValueError, "crossings", r, 2, mask=np.zeros(5, dtype=np.int32))
    glue.refused(ValueError, "nearest", np.zeros((4, 4)), 2, mask=np.zeros(5, dtype=np.int32))
    for method, extra in (("radiance", ()), ("bounce", ())):
        glue.refused(ValueError, method, np.zeros((4, 6)), st, *extra)
        glue.refused(ValueError, method, r, np.zeros((4, 3), dtype=np.uint64))
        glue.refused(ValueError, method, r, np.zeros((4, 4)))                      # states must be 64-bit integers
        glue.refused(ValueError, method, r, np.zeros((4, 4), dtype=np.uint32))
    glue.refused(ValueError, "scatter", np.zeros((4, 6)), np.zeros((4, 8)), st)
    glue.refused(ValueError, "scatter", r, np.zeros((3, 8)), st)
    glue.refused(ValueError, "scatter", r, np.zeros((4, 8)), np.zeros((5, 4), dtype=np.uint64))


# the ctypes signature of every exported symbol, of tor_render.h and of the six later headers: "argtypes" ("-": none set) and
# restype; *x is POINTER(x)
SIGNATURES = {
    "tor_render": ("*CanvasStruct *Camera HittableList i64", "i32"),
    "tor_render_opt": ("*CanvasStruct *Camera HittableList i64 *Options", "i32"),
    "tor_last_error": ("-", "s"),
    "tor_context_create": ("i32 *v", "i32"),
    "tor_context_destroy": ("v", "i32"),
    "tor_scene_upload": ("v HittableList", "i32"),
    "tor_shard_rows": ("i32 i32 i32 i32 *i32", "i32"),
    "tor_render_device": ("v *Camera i32 i32 i32 f i64 *Options v v", "i32"),
    "tor_quantize_rgb8_device": ("v v i64 v v", "i32"),
    "tor_last_kernel_ms": ("v *f *i64", "i32"),
    "tor_kernel_ms_mean": ("v i32 *f *i32", "i32"),
    "tor_context_set_stats": ("v i32", "i32"),
    "tor_last_stats": ("v *Stats", "i32"),
    "tor_last_wave_log": ("v *u64 i64", "i32"),
    "tor_camera_init": ("*Camera *Vec3 *Vec3 *Vec3 d d d d d d", "i32"),
    "tor_random_scene": ("u64 *HittableVariant i64", "i64"),
    "tor_canvas_to_rgb8": ("*CanvasStruct *u8", "i32"),
    "tor_animation_create": ("u64 i32 i32 f f f *v", "i32"),
    "tor_animation_destroy": ("v", "none"),
    "tor_animation_object_count": ("v", "i64"),
    "tor_animation_next": ("v i32 *Camera *HittableVariant i64 *i64 *f", "i32"),
    "tor_h264_stream_header": ("i32 i32 *u8 i32", "i32"),
    "tor_h264_frame_bytes": ("i32 i32", "i64"),
    "tor_encode_frame_device": ("v v i32 i32 v v v v v", "i32"),
    "tor_render_frame_h264": ("v *Camera i32 i32 i32 f i64 *Options *u8 i64", "i32"),
    "tor_mp4_mux_file": ("s s i32 i32 i32", "i32"),
    "tor_debug_accel_layout": ("HittableList d d *i64 i64 *d *d i64 *i32", "i32"),
    "tor_selftest_filter32_host": ("i64 *d *d *d *d *i32 *d *d *d *i32 *i32", "i32"),
    "tor_selftest_screen_host": ("i64 *d *d *d *d *i32 *d *d *i32 *i32", "i32"),
    "tor_selftest_slab32_host": ("i64 *d *d *d *d *d *i32 *i32", "i32"),
    "tor_debug_filter32_scene": ("HittableList i64 *d *d *d *i8", "i32"),
    "tor_selftest_math_device": ("i32 *d *d *d *d i64 i32", "i32"),
    "tor_selftest_math_host": ("i32 *d *d *d *d i64", "i32"),
    "tor_selftest_rng_host": ("i32 u64 u64 u64 *u64 *u64 i64", "i32"),
    "tor_version": ("-", "s"),
    "tor_last_render_timing": ("*d", "i32"),
    "tor_comm_unique_id": ("*u8", "i32"),
    "tor_comm_init_rank": ("v *u8 i32 i32", "i32"),
    "tor_comm_destroy": ("v", "i32"),
    "tor_render_gather_device": ("v *Camera i32 i32 i32 f i64 *Options i32 v v", "i32"),
    "tor_context_scene_counters": ("v *i64", "i32"),
    "tor_render_ptr": ("*CanvasStruct *Camera *HittableList i64", "i32"),
    "tor_last_pixel_cost": ("v *u32 i64", "i64"),
    "tor_last_note": ("-", "s"),
    "tor_last_handoff_counters": ("v *u64", "i32"),
    "tor_selftest_screen2_host": ("i64 *d *d *d *d *i32 *d *d i32 *i32 *i32", "i32"),
    "tor_debug_screen2_scene": ("HittableList i64 *d *d *d *i8 *i32 *i8 i64", "i32"),
    "tor_debug_layout_segments": ("HittableList *i32 i64 *i64", "i32"),
    "tor_debug_plane32_scene": ("HittableList i64 *d *d *d *i8 *i32 *i64", "i32"),
    "tor_knob_count": ("-", "i32"),
    "tor_knob_info": ("i32 *s *s *s *s *s", "i32"),
    "tor_last_gather_info": ("*i32", "i32"),
    "tor_last_device_kernel_ms": ("*f i32", "i32"),
    "tor_comm_abort": ("v", "i32"),
    "tor_comm_count": ("v *i32", "i32"),
    "tor_context_handoff_stalled": ("v *i32 *i64", "i32"),
    "tor_render_accumulate_device": ("v *Camera i32 i32 i32 i32 i64 *Options v v v", "i32"),
    "tor_resolve_device": ("v v i64 i64 f v v", "i32"),
    "tor_accum_noise_device": ("v v v i64 i64 v *d v", "i32"),
    "tor_render_accumulate_list_device": ("v *Camera i32 i32 v i32 i32 i32 i64 *Options v v v", "i32"),
    "tor_adaptive_select_device": ("v v v v i32 i64 d d v v *i32 v", "i32"),
    "tor_resolve_counts_device": ("v v v i64 f v v", "i32"),
    "tor_debug_last_variant": ("v *i32", "i32"),
    "tor_hit_device": ("v i64 v v d d i32 v v", "i32"),
    "tor_hit_host": ("v i64 v v d d i32 v", "i32"),
    "tor_radiance_device": ("v i64 v v i32 d d i32 v v", "i32"),
    "tor_radiance_host": ("v i64 v v i32 d d i32 v", "i32"),
    "tor_camera_rays_device": ("v *Camera i32 i32 v i64 i32 i32 i32 v v v", "i32"),
    "tor_bounce_device": ("v i64 v v v i64 d d i32 v v v v", "i32"),
    "tor_bounce_host": ("v i64 v v v i64 d d i32 v v v", "i32"),
    "tor_scatter_device": ("v i64 v v v v i64 v v v", "i32"),
    "tor_scatter_host": ("v i64 v v v v i64 v v", "i32"),
    "tor_sky_device": ("v i64 v v i64 v v", "i32"),
    "tor_bounce_select_device": ("v i64 v v i64 v *i64 v", "i32"),
    "tor_render_resume_device": ("v *Camera i32 i32 i32 i32 i64 *Options v v v v", "i32"),
    "tor_debug_last_split_tiles": ("v *i64", "i32"),
    "tor_render_resume_list_device": ("v *Camera i32 i32 v i32 i32 i32 i64 *Options v v v v", "i32"),
    "tor_occluded_device": ("v i64 v v v i64 d d i32 v v", "i32"),
    "tor_occluded_host": ("v i64 v v v i64 d d i32 v", "i32"),
    "tor_scene_groups": ("v i64 v", "i32"),
    "tor_hit_masked_device": ("v i64 v v d d i32 v v v u32", "i32"),
    "tor_hit_masked_host": ("v i64 v v d d i32 v v u32", "i32"),
    "tor_occluded_masked_device": ("v i64 v v v i64 d d i32 v v v u32", "i32"),
    "tor_occluded_masked_host": ("v i64 v v v i64 d d i32 v v u32", "i32"),
    "tor_bounce_masked_device": ("v i64 v v v i64 d d i32 v v v v v u32", "i32"),
    "tor_crossings_device": ("v i64 v v v i64 i32 v u32 d d i32 v v v v", "i32"),
    "tor_crossings_host": ("v i64 v v v i64 i32 v u32 d d i32 v v v", "i32"),
    "tor_nearest_device": ("v i64 v v v i64 i32 v u32 d d i32 v v v", "i32"),
    "tor_nearest_host": ("v i64 v v v i64 i32 v u32 d d i32 v v", "i32"),
    "tor_deposit_device": ("v i64 v v v i64 d i64 v v v v v", "i32"),
    # the later headers' entries, from their declarations (every pointer but the camera's is passed as an address)
    # include/tor_lights.h
    "tor_scene_lights": ("v i64 v v", "i32"),
    "tor_light_sample_device": ("v i64 v v v i64 i32 v v v v v", "i32"),
    "tor_light_sample_host": ("v i64 v v v i64 i32 v v v v", "i32"),
    "tor_light_pdf_device": ("v i64 v v v i64 i32 v v", "i32"),
    "tor_light_pdf_host": ("v i64 v v v i64 i32 v", "i32"),
    # include/tor_env.h
    "tor_scene_environment": ("v i64 v v", "i32"),
    "tor_env_sample_device": ("v i64 v v v i64 v v v v v", "i32"),
    "tor_env_sample_host": ("v i64 v v v i64 v v v v", "i32"),
    "tor_env_eval_device": ("v i64 v v i64 v v v v", "i32"),
    "tor_env_eval_host": ("v i64 v v i64 v v v", "i32"),
    # include/tor_camera.h
    "tor_camera_connect_device": ("v *Camera i32 i32 i64 v v v i64 v v v v v", "i32"),
    "tor_camera_connect_host": ("v *Camera i32 i32 i64 v v v i64 v v v v", "i32"),
    "tor_light_emit_device": ("v i64 v v i64 d d v v v v v", "i32"),
    "tor_light_emit_host": ("v i64 v v i64 d d v v v v", "i32"),
    # include/tor_bsdf.h
    "tor_bsdf_eval_device": ("v i64 v v v v i64 v v v v", "i32"),
    "tor_bsdf_eval_host": ("v i64 v v v v i64 v v v", "i32"),
    # include/tor_photons.h
    "tor_photons_build_device": ("v i64 v v v v i64 d v", "i32"),
    "tor_photons_build_host": ("v i64 v v v v i64 d", "i32"),
    "tor_photons_gather_device": ("v i64 v v v v i64 i32 d v v v", "i32"),
    "tor_photons_gather_host": ("v i64 v v v v i64 i32 d v v", "i32"),
    "tor_photons_info": ("v v", "i32"),
    # include/tor_media.h
    "tor_scene_media": ("v i64 v v v", "i32"),
    "tor_media_march_device": ("v i64 v v v v i64 v v v v v v", "i32"),
    "tor_media_march_host": ("v i64 v v v v i64 v v v v v", "i32"),
    "tor_media_scatter_device": ("v i64 v v v v v i64 v v v", "i32"),
    "tor_media_scatter_host": ("v i64 v v v v v i64 v v", "i32"),
    "tor_rng_uniform_device": ("v i64 v v i64 i32 v v", "i32"),
    "tor_rng_uniform_host": ("v i64 v v i64 i32 v", "i32"),
}


def test_every_exported_symbol_keeps_its_signature(tor):
    simple = {"v": C.c_void_p, "i32": C.c_int32, "i64": C.c_int64, "u32": C.c_uint32, "u64": C.c_uint64, "d": C.c_double,
              "f": C.c_float, "s": C.c_char_p, "u8": C.c_uint8, "i8": C.c_int8, "none": None}

    def of(token):
        if token.startswith("*"):
            return C.POINTER(of(token[1:]))
        return simple[token] if token in simple else getattr(tor, token)

    every = (tor.EXPORTED_SYMBOLS + tor.LIGHT_SYMBOLS + tor.ENV_SYMBOLS + tor.CAMERA_SYMBOLS + tor.BSDF_SYMBOLS + tor.PHOTON_SYMBOLS
             + tor.MEDIA_SYMBOLS)
    assert len(set(every)) == len(set(tor.EXPORTED_SYMBOLS)) + 28          # (the six later lists share no name with any other)
    assert sorted(SIGNATURES) == sorted(set(every))
    L = types.SimpleNamespace(**{name: types.SimpleNamespace(argtypes=None, restype=C.c_int) for name in every})
    tor._bind(L)
    for name, (argtypes, restype) in SIGNATURES.items():
        fn = getattr(L, name)
        want = None if argtypes == "-" else [of(t) for t in argtypes.split()]
        assert (None if fn.argtypes is None else list(fn.argtypes)) == want, name
        assert fn.restype is of(restype), name
    # ... and on other builds of the library: the named symbols only, one that is missing skipped only where asked to
    other = types.SimpleNamespace(tor_hit_device=types.SimpleNamespace(argtypes=None, restype=C.c_int))
    tor._bind(other, ("tor_hit_device", "tor_hit_host"), skip_missing=True)
    assert list(other.tor_hit_device.argtypes) == [of(t) for t in SIGNATURES["tor_hit_device"][0].split()]
    with pytest.raises(AttributeError):
        tor._bind(other, ("tor_hit_device", "tor_hit_host"))
