"""Nearest-surface point queries on the MI355X (tor_nearest_device / tor_nearest_host): in every mode and for K in {1, 2, 4, max}
(both capacity variants of the kernel) the distance bits, object, inside, count and the unused entries of every point are those of
the numpy restatement (tests/nearest_restatement.py, held to hand-worked cases by tests/test_nearest_query.py, which also shows
that these inputs mean something), bit for bit.  What the kernel may break: a neighbour lost to the shrinking bound (a box skipped
although the point lies inside it, a tie decided the wrong way), to d_max, to a wave's other lanes, to a mask, or to the reach."""
import numpy as np
import pytest
import torch

import nearest_inputs as I
import nearest_restatement as N
import query_regimes as Q

pytestmark = pytest.mark.gpu
MODES = ("auto", "brute", "blocks")
KMAX = 16
KS = (1, 2, 4, KMAX)
NO_RAY_REACH = "brute force (the block boxes' margin holds for no ray origin (radii too small))"
AUTO_BRUTE = "brute force (auto: k > 4 without a limit on a one-level layout)"
TWO_LEVEL = ("anim", "dense2")


def _ctx(tor, recs):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    return ctx


def _cuda(a, dtype=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np(res):
    """A NearestResult (tensors or arrays) as numpy fields."""
    f = (lambda v: v.cpu().numpy()) if isinstance(res.raw, torch.Tensor) else np.asarray
    return {"distance": f(res.distance), "object": f(res.object), "inside": f(res.inside), "count": f(res.count)}


def _query(ctx, pts, k, d_max=None, mode="auto", index=None, mask=None, out=None, time_range=I.TIME_RANGE):
    if mask is not None and np.ndim(mask) > 0:
        mask = torch.from_numpy((np.asarray(mask).astype(np.int64) & N.ALL).astype(np.uint32).view(np.int32)).cuda()
    if d_max is not None and np.ndim(d_max) > 0:
        d_max = _cuda(d_max)
    res = ctx.nearest(_cuda(pts), k, d_max, index, time_range, mode, mask, out)
    torch.cuda.synchronize()
    got = _np(res)
    assert got["distance"].shape == (len(pts), k) and got["object"].dtype == np.int32 and got["count"].shape == (len(pts),)
    return got, res.mode


def _cut(want, k):
    """The restatement's first KMAX neighbours cut to the first k."""
    return {"distance": want["distance"][:, :k], "object": want["object"][:, :k], "inside": want["inside"][:, :k],
            "count": np.minimum(want["total"], k).astype(np.int32)}


def _check(ctx, pts, want, d_max=None, modes=MODES, ks=KS, mask=None, time_range=I.TIME_RANGE):
    """Every mode and K against the restatement at KMAX, bit for bit; returns {(mode, K): what ran}."""
    ran = {}
    for m in modes:
        for k in ks:
            got, ran[m, k] = _query(ctx, pts, k, d_max, m, mask=mask, time_range=time_range)
            bad = N.mismatches(got, _cut(want, k))
            assert not bad, f"mode {m} (ran: {ran[m, k]}), K = {k}: {bad}"
            unused = np.arange(k)[None, :] >= got["count"][:, None]
            assert (got["object"][unused] == -1).all() and (got["distance"][unused] == 0).all() and (got["inside"][unused] == 0).all()
    return ran


def _assert_ran(name, ran, limited):
    """What ran, per mode and K.  odd_objects has a radius 0 among the blocks' objects: no ray origin may use the boxes, and the
    library says so.  Elsewhere `blocks` runs the blocks, and so does `auto` but for the large list without a limit on a one-level
    layout, where the brute force measured faster (profiles/nearest_rate.txt)."""
    for (m, k), what in ran.items():
        if m == "brute":
            want = "brute force"
        elif name == "odd_objects":
            want = NO_RAY_REACH
        elif m == "auto" and k > 4 and not limited and name not in TWO_LEVEL:
            want = AUTO_BRUTE
        else:
            want = "blocks"
        assert what == want, (name, m, k, what)


_cases = {}


def _case(tor, name):
    """Scene, points, the restatement without a limit and the two limits: computed once per scene, never changed."""
    if name not in _cases:
        recs = I.scene(tor, name)
        pts = I.points(recs, I.layout(tor, recs))
        open16 = N.nearest(recs, pts, KMAX)
        d_scene = I.scene_d_max(open16)
        _cases[name] = dict(recs=recs, pts=pts, open16=open16, d_scene=d_scene, d_point=I.point_d_max(len(pts), d_scene))
    return _cases[name]


@pytest.mark.parametrize("name", I.SCENES)
def test_every_mode_k_and_limit_against_the_restatement(tor, name):
    g = _case(tor, name)
    recs, pts = g["recs"], g["pts"]
    ctx = _ctx(tor, recs)
    _assert_ran(name, _check(ctx, pts, g["open16"]), False)
    under = N.nearest(recs, pts, KMAX, g["d_scene"])
    assert 0.3 <= (under["total"] == 0).mean() <= 0.7                     # short lists for about half of the points
    _assert_ran(name, _check(ctx, pts, under, g["d_scene"]), True)
    per_point = N.nearest(recs, pts, KMAX, g["d_point"])
    assert (per_point["total"][np.isnan(g["d_point"])] == 0).all() and (per_point["total"] >= KMAX).any()
    _assert_ran(name, _check(ctx, pts, per_point, g["d_point"]), True)


@pytest.mark.parametrize("name", ["groups", "random"])
def test_the_time_range_is_a_hint(tor, name):
    """Over (0.5, 0.75) most points' times lie outside the boxes' range: they walk; over the points' own times (None) the range is
    (-3, 2.5).  The answer is the same."""
    g = _case(tor, name)
    ctx = _ctx(tor, g["recs"])
    t = g["pts"][:, 3]
    assert ((t < 0.5) | (t > 0.75) | np.isnan(t)).mean() > 0.7
    for tr in ((0.5, 0.75), None, (0.25, 0.25)):
        _assert_ran(name, _check(ctx, g["pts"], g["open16"], ks=(1, 4, KMAX), time_range=tr), False)


@pytest.mark.parametrize("name", ["groups", "dense2", "dense"])
def test_masks_that_differ_inside_every_wave(tor, name):
    g = _case(tor, name)
    recs, pts = g["recs"], g["pts"]
    groups, masks = Q.group_words(len(recs)), Q.ray_masks(len(pts), 7)
    for w0 in range(0, len(pts), 64):
        assert np.unique(masks[w0:w0 + 64]).size > 1
    ctx = _ctx(tor, recs)
    before, _ = _query(ctx, pts, 4, mode="blocks")
    ctx.set_groups(groups)
    for d_max in (None, g["d_point"]):
        want = N.masked_nearest(recs, groups, pts, masks, KMAX, d_max)
        assert (want["count"][masks == 0] == 0).all()
        _assert_ran(name, _check(ctx, pts, want, d_max, mask=masks), d_max is not None)
    assert (want["total"] != N.nearest(recs, pts, KMAX, g["d_point"])["total"]).mean() > 0.2
    # one word for every point: the restatement on the sub-list, `object` in the full numbering
    seen = np.nonzero((groups & 6) != 0)[0]
    sub = N.nearest(recs[seen], pts, 4)
    got, _ = _query(ctx, pts, 4, mask=6)
    sub["object"] = np.where(sub["object"] >= 0, seen[np.maximum(sub["object"], 0)], -1).astype(np.int32)
    assert not N.mismatches(got, sub) and (sub["count"] > 0).sum() > 50
    # the unmasked call reads no group state: the same result before and after set_groups, whatever the words
    ctx.set_groups(np.zeros(len(recs), dtype=np.uint32))
    after, mode = _query(ctx, pts, 4, mode="blocks")
    assert mode == "blocks" and not N.mismatches(after, before) and not N.mismatches(before, _cut(g["open16"], 4))
    nothing, _ = _query(ctx, pts, 4, mask=N.ALL - 1)                      # a masked call does read them
    assert (nothing["count"] == 0).all()


def test_lists_keep_what_is_not_listed(tor):
    g = _case(tor, "random")
    recs, pts = g["recs"], g["pts"]
    ctx = _ctx(tor, recs)
    n, k = len(pts), 4
    want = _cut(g["open16"], k)
    dp = _cuda(pts)
    for m in MODES:
        for idx, listed_ids in ((np.arange(1, n, 3, dtype=np.int32), np.arange(1, n, 3)),
                                (np.array([n, 5, -1, 2047, 64, n + 100, 0, -(1 << 31), n - 1, (1 << 31) - 1], dtype=np.int32),
                                 [5, 2047, 64, 0, n - 1])):
            out = ctx.nearest(dp, k, index=np.zeros(0, dtype=np.int32), mode=m, time_range=I.TIME_RANGE)   # an empty list: a no-op
            torch.cuda.synchronize()
            assert out.mode == "nothing to do" and int(out.count.sum()) == 0 and bool((out.object == -1).all())
            out.raw.fill_(7.0)
            out.count.fill_(7)
            res = ctx.nearest(dp, k, index=idx, mode=m, out=out, time_range=I.TIME_RANGE)
            torch.cuda.synchronize()
            assert res.raw is out.raw
            got = _np(res)
            listed = np.zeros(n, dtype=bool)
            listed[listed_ids] = True
            bad = N.mismatches({name: got[name][listed] for name in want}, {name: want[name][listed] for name in want})
            assert not bad, (m, bad)
            assert (got["count"][~listed] == 7).all() and (res.raw.cpu().numpy()[~listed] == 7.0).all(), m


@pytest.mark.parametrize("n", [0, 1, 63, 65, 257])
def test_batch_sizes(tor, n):
    g = _case(tor, "random")
    ctx = _ctx(tor, g["recs"])
    pts = g["pts"][:n]
    want = {name: v[:n] for name, v in g["open16"].items()}
    _check(ctx, pts, want, ks=(1, 4, KMAX))
    if n == 0:   # numpy in, too
        res = ctx.nearest(np.zeros((0, 4)), 3)
        assert res.distance.shape == (0, 3) and res.count.shape == (0,) and res.mode == "nothing to do"


def test_host_entry_and_numpy_input_equal_the_device_entry(tor):
    g = _case(tor, "random")
    recs, pts = g["recs"], g["pts"]
    ctx = _ctx(tor, recs)
    groups, masks = Q.group_words(len(recs)), Q.ray_masks(len(pts), 8)
    ctx.set_groups(groups)
    for m in MODES:
        for k, mask, d_max in ((3, None, None), (KMAX, masks, g["d_point"]), (1, 6, g["d_scene"])):
            host = ctx.nearest(pts, k, d_max, mode=m, mask=mask, time_range=I.TIME_RANGE)   # numpy in: tor_nearest_host
            assert isinstance(host.raw, np.ndarray) and host.object.dtype == np.int32 and host.distance.shape == (len(pts), k)
            dev, ran = _query(ctx, pts, k, d_max, m, mask=mask)
            assert host.mode == ran and not N.mismatches(_np(host), dev), (m, k)
            idx = np.arange(0, len(pts), 2, dtype=np.int32)
            host.count[:] = 7
            again = ctx.nearest(pts, k, d_max, index=idx, mode=m, mask=mask, out=host, time_range=I.TIME_RANGE)   # keeps what is not listed
            assert np.array_equal(again.count[0::2], dev["count"][0::2]) and (again.count[1::2] == 7).all()
    assert (host.count > 0).mean() > 0.05
    with pytest.raises(tor.TorError) as e:
        tor.Context(0).nearest(pts, 2)
    assert "no scene" in str(e.value)


def test_device_only_brute_equals_blocks_on_2_to_the_16_points(tor):
    """2^16 points on dense2 (two levels), all on the device: brute force and blocks agree in every bit, and K = 1 is entry 0 of
    K = 16."""
    recs = I.scene(tor, "dense2")
    pts = _cuda(I.points(recs, I.layout(tor, recs), seed=23, n=1 << 16))
    ctx = _ctx(tor, recs)
    res = {}
    for m in ("brute", "blocks"):
        for k in (1, KMAX):
            res[m, k] = ctx.nearest(pts, k, None, None, I.TIME_RANGE, m)
    torch.cuda.synchronize()
    assert res["brute", 1].mode == "brute force" and res["blocks", KMAX].mode == "blocks"
    for k in (1, KMAX):
        assert torch.equal(res["brute", k].raw.view(torch.int64), res["blocks", k].raw.view(torch.int64)), k
        assert torch.equal(res["brute", k].count, res["blocks", k].count), k
    for m in ("brute", "blocks"):
        assert torch.equal(res[m, 1].raw[:, 0].contiguous().view(torch.int64), res[m, KMAX].raw[:, 0].contiguous().view(torch.int64)), m
    assert int((res["blocks", KMAX].count == KMAX).sum()) > 30000 and int(res["blocks", KMAX].inside.sum()) > 10000


def test_torch_cross_check_of_the_definition(tor):
    """A third statement, independent of library and restatement: the definition as plain torch float64 arithmetic on the device
    (unfused elementwise kernels), min over the objects, at K = 1 without a limit."""
    g = _case(tor, "random")
    recs = torch.from_numpy(np.array(g["recs"])).cuda()
    pts = torch.from_numpy(np.array(g["pts"][:512])).cuda()
    ctx = _ctx(tor, g["recs"])
    res = ctx.nearest(pts, 1, time_range=I.TIME_RANGE)
    p, time = pts[:, None, 0:3], pts[:, None, 3]
    c0, c1, t0, t1, r = recs[None, :, 1:4], recs[None, :, 4:7], recs[None, :, 7], recs[None, :, 8], recs[None, :, 9]
    f = (time - t0) / (t1 - t0)
    c = torch.where((recs[None, :, 0] != 0)[:, :, None], c0 + (c1 - c0) * f[:, :, None], c0.expand(len(pts), -1, -1))
    oc = p - c
    x, y, z = oc[:, :, 0], oc[:, :, 1], oc[:, :, 2]
    d = torch.sqrt(x * x + y * y + z * z) - r.abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    best, arg = d.min(dim=1)
    torch.cuda.synchronize()
    has = torch.isfinite(best)
    assert int(has.sum()) > 400 and torch.equal(res.count, has.int())
    assert torch.equal(res.distance[:, 0][has].contiguous().view(torch.int64), best[has].contiguous().view(torch.int64))
    assert torch.equal(torch.gather(d, 1, res.object[:, :1].long().clamp(min=0))[:, 0][has].view(torch.int64), best[has].view(torch.int64))
