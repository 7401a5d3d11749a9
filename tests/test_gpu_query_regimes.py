"""The query kernels across scene regimes on the MI355X: closest hit, any-hit, ordered crossings (both capacity variants), their
masked forms, one path step and radiance -- every includer of the shared descent and both copies of it -- against the numpy
restatements, bit for bit, in every mode, on the scenes of tests/query_regimes.py: tiny, far from the world origin, huge, dense
clusters with exact duplicates, a two-level layout, every time group, no ground, radii for which the boxes' margin holds for no
origin (the block path must fall back, and say why), a reach that cuts through the ray origins (boxed and walking lanes in every
wave, origins a few ulps either side of the reach), and non-finite and overflowing objects.  tests/test_query_regimes.py shows on
the CPU that these inputs hit, cross, tie and graze enough to mean something.

What the existing query tests could not see: their three scenes give hit_reach, the boxes' inflation and the layout the same
three sets of values, and neither fallback of query_setup ran."""
import numpy as np
import pytest
import torch

import bounce_restatement as B
import crossings_restatement as X
import hit_restatement as H
import masked_restatement as M
import query_regimes as Q
import radiance_restatement as RR

pytestmark = pytest.mark.gpu
MODES = ("auto", "brute", "blocks")
KS = (1, 4, 16)                                           # crossings_kernel<.., CAP = 4> (K <= 4) and <.., CAP = 16>
TIME_RANGE = (0.0, 1.0)
N_RAYS, SCENE_SEED, RAY_SEED, REACH_SEED = 2048, 0, 7, 3  # as tests/test_query_regimes.py measured them
N_STEP, N_RADIANCE = 512, 128                             # (those two restatements loop in Python)
WHY_RADII = "the block boxes' margin holds for no ray origin (radii too small)"
WHY_BOUNDS = "no finite block bounds for the time range"


def _ctx(tor, recs):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    return ctx


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _np(t):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def _cut(want, k):
    """The restatement's first 16 crossings cut to the first k."""
    return {"t": want["t"][:, :k], "object": want["object"][:, :k], "which": want["which"][:, :k],
            "count": np.minimum(want["total"], k).astype(np.int32)}


def _inputs(tor, name):
    """Scene, rays (the regime's own, and the rays on the reach where there is one) and what the block modes must run."""
    recs = Q.scene(name, SCENE_SEED)
    layout = tor.debug_accel_layout(tor.Scene.from_records(recs).list(), *TIME_RANGE)
    assert layout is not None
    rays, tr = Q.rays(recs, N_RAYS, RAY_SEED)
    _, reach, _ = Q.reach_of(recs, layout)
    if reach > 0:
        rr, rtr, _ = Q.reach_rays(recs, layout, REACH_SEED)
        rays, tr = np.concatenate([rays, rr]), np.concatenate([tr, rtr])
    return recs, rays, tr, ("blocks" if reach > 0 else f"brute force ({WHY_RADII})")


def _check_queries(tor, ctx, recs, rays, tr, expect, groups=None, masks=None, time_range=TIME_RANGE, modes=MODES, ks=KS):
    """hit, occluded and crossings (K in ks, records at K = 4) in every mode against the restatements, masked when `masks` is given;
    `expect`: what the modes auto and blocks must run."""
    masked = masks is not None
    want = M.world_hit(recs, groups, rays, masks, tr) if masked else H.world_hit(recs, rays, tr)
    want_bit = (H.fields(want)["object"] >= 0).astype(np.int32)
    want_x = X.masked_crossings(recs, groups, rays, masks, 16, tr) if masked else X.crossings(recs, rays, 16, tr)
    d_rays, d_tr = _dev(rays), _dev(tr)
    d_mask = _dev(M.ray_masks(masks, len(rays))) if masked else None
    tag = " (masked): " if masked else ": "
    for m in modes:
        ran = "brute force" if m == "brute" else expect
        res = ctx.hit(d_rays, d_tr, time_range, m, mask=d_mask)
        assert res.mode == ran and tor.last_note() == "hit" + tag + ran, (m, tor.last_note())
        bad = H.mismatches(_np(res.raw), want)
        assert not bad, f"hit{tag}mode {m} (ran: {res.mode}): {bad}"
        occ = ctx.occluded(d_rays, d_tr, None, time_range, m, mask=d_mask)
        assert occ.mode == ran and tor.last_note() == "occluded" + tag + ran, (m, tor.last_note())
        wrong = np.flatnonzero(_np(occ.raw) != want_bit)
        assert wrong.size == 0, f"occluded{tag}mode {m} (ran: {occ.mode}): {wrong.size} rays differ, first {wrong[:8]}"
        for k in ks:
            records = k == 4
            cr = ctx.crossings(d_rays, k, d_tr, None, time_range, m, d_mask, records)
            assert cr.mode == ran and tor.last_note() == "crossings" + tag + ran, (m, k, tor.last_note())
            got = {"t": _np(cr.t), "object": _np(cr.object), "which": _np(cr.which), "count": _np(cr.count)}
            w = _cut(want_x, k)
            bad = X.mismatches(got, w, _np(cr.hits) if records else None, X.records(recs, rays, w) if records else None)
            assert not bad, f"crossings{tag}mode {m} (ran: {cr.mode}), K = {k}: {bad}"
            unused = np.arange(k)[None, :] >= got["count"][:, None]
            assert (got["object"][unused] == -1).all() and (got["t"][unused] == 0).all() and (got["which"][unused] == 0).all()
    return want


@pytest.mark.parametrize("name", Q.REGIMES)
def test_regime_against_the_restatements(tor, oracle, name):
    """One upload per regime; every query family in every mode.  The upload takes every record of odd_objects (it refuses unknown
    kinds only), so all six odd objects stay in."""
    recs, rays, tr, expect = _inputs(tor, name)
    n = len(rays)
    if name in Q.BASE or name == "reach_split":
        assert expect == "blocks" and n > N_RAYS
    else:
        assert expect.startswith("brute force (") and n == N_RAYS
    ctx = _ctx(tor, recs)
    plain = _check_queries(tor, ctx, recs, rays, tr, expect)

    # one path step and radiance: the other two includers of the shared descent (their range is render.nim's (0.001, +inf))
    step_ids = np.concatenate([np.arange(N_STEP * 3 // 4), np.arange(N_RAYS, N_RAYS + N_STEP // 4)]) if n > N_RAYS else np.arange(N_STEP)
    st = np.asarray(np.random.default_rng(77).integers(0, 2**63, (len(step_ids), 4), dtype=np.uint64))
    want_step = B.step(oracle, recs, rays[step_ids], st)
    assert (want_step["status"] == B.SCATTERED).mean() > 0.2
    rad_ids = step_ids[:: N_STEP // N_RADIANCE]
    want_color, want_st = RR.radiance(oracle, recs, rays[rad_ids], st[:: N_STEP // N_RADIANCE], 50)
    for m in MODES:
        ran = "brute force" if m == "brute" else expect
        b = ctx.bounce(_dev(rays[step_ids]), _dev(st), None, TIME_RANGE, m)
        assert b.mode == ran and tor.last_note() == "bounce: " + ran, (m, tor.last_note())
        assert not H.mismatches(_np(b.raw), want_step["raw"]), ("step", m)
        assert np.array_equal(_np(b.status), want_step["status"]), ("step", m)
        assert _eq(_np(b.attenuation), want_step["attenuation"]) and _eq(_np(b.rays), want_step["rays"]), ("step", m)
        assert np.array_equal(_np(b.rng), want_step["states"]), ("step", m)
        color, st_out, rad_ran = ctx.radiance(_dev(rays[rad_ids]), _dev(st[:: N_STEP // N_RADIANCE]), 50, TIME_RANGE, m)
        assert rad_ran == ran, (m, rad_ran)
        assert _eq(_np(color), want_color) and np.array_equal(_np(st_out), want_st), ("radiance", m)

    # the masked forms: object words 1 << (j % 5), every 11th 0, every 13th 0xFFFFFFFF; masks that differ inside every wave
    groups, masks = Q.group_words(len(recs)), Q.ray_masks(n, RAY_SEED)
    assert all(np.unique(masks[w0:w0 + 64]).size > 1 for w0 in range(0, n - 63, 64))
    changed, keeps, mixed = M.meaningful(recs, groups, rays, masks, tr)
    assert changed >= 0.2 and mixed, f"the masks change only {changed:.3f} of the answers"
    ctx.set_groups(groups)
    masked = _check_queries(tor, ctx, recs, rays, tr, expect, groups, masks)
    assert (H.fields(masked)["object"][masks == 0] == -1).all()
    # ... and the unmasked query reads no group state
    again = ctx.hit(_dev(rays), _dev(tr), TIME_RANGE, "blocks")
    assert again.mode == expect and not H.mismatches(_np(again.raw), plain)


def test_no_finite_block_bounds_for_the_time_range(tor):
    """query_setup's other reason to fall back: over the time range (0, 1e200) -- finite, so every entry accepts it -- the centre of
    odd_objects' mover displaced by 1e200 overflows and compute_block_bounds has no finite box for its block.  The answers are the
    restatement's all the same, and the cached bounds follow the range: (0, 1) afterwards falls back for its own reason."""
    recs = Q.scene("odd_objects", SCENE_SEED)
    rays, tr = Q.rays(recs, N_RAYS, RAY_SEED)
    ctx = _ctx(tor, recs)
    for time_range, why in (((0.0, 1e200), WHY_BOUNDS), (TIME_RANGE, WHY_RADII), ((0.0, 1e200), WHY_BOUNDS)):
        _check_queries(tor, ctx, recs, rays, tr, f"brute force ({why})", time_range=time_range, ks=(4,))
    ctx.set_groups(Q.group_words(len(recs)))
    _check_queries(tor, ctx, recs, rays, tr, f"brute force ({WHY_BOUNDS})", Q.group_words(len(recs)), Q.ray_masks(N_RAYS, RAY_SEED),
                   time_range=(0.0, 1e200), modes=("blocks",), ks=(4,))
    b = ctx.bounce(_dev(rays[:64]), _dev(np.ones((64, 4), dtype=np.uint64)), None, (0.0, 1e200), "blocks")
    assert b.mode == f"brute force ({WHY_BOUNDS})"
    _, _, ran = ctx.radiance(_dev(rays[:64]), _dev(np.ones((64, 4), dtype=np.uint64)), 2, (0.0, 1e200), "auto")
    assert ran == f"brute force ({WHY_BOUNDS})"


def test_dense2_device_side_consistency_over_65536_rays(tor):
    """2^16 rays on the two-level dense scene, all on the device (the pattern of test_gpu_crossings_query's
    test_device_side_consistency_with_hit_and_occluded, without the chained hits): crossing 0 and its record are ctx.hit's answer,
    count > 0 is ctx.occluded's bit, and the brute force equals the blocks for all three queries."""
    recs = Q.scene("dense2", SCENE_SEED)
    n = 1 << 16
    rays, tr = Q.rays(recs, n, RAY_SEED + 1)
    ctx = _ctx(tor, recs)
    d_rays, d_tr = _dev(rays), _dev(tr)
    out = {}
    for m in ("brute", "blocks"):
        cr = ctx.crossings(d_rays, 4, d_tr, None, TIME_RANGE, m, records=True)
        cr16 = ctx.crossings(d_rays, 16, d_tr, None, TIME_RANGE, m)
        hit = ctx.hit(d_rays, d_tr, TIME_RANGE, m)
        occ = ctx.occluded(d_rays, d_tr, None, TIME_RANGE, m)
        torch.cuda.synchronize()
        assert cr.mode == cr16.mode == hit.mode == occ.mode == {"brute": "brute force", "blocks": "blocks"}[m]
        assert torch.equal(cr.hits[:, 0].contiguous().view(torch.int64), hit.raw.view(torch.int64)), f"{m}: record 0 is not hit()'s"
        assert torch.equal(cr.object[:, 0], hit.object)
        assert torch.equal(cr.t[:, 0].contiguous().view(torch.int64), hit.t.contiguous().view(torch.int64))
        assert torch.equal(cr.count == 0, hit.object < 0) and torch.equal(cr.count > 0, occ.occluded)
        assert torch.equal(cr.raw.view(torch.int64), cr16.raw[:, :4].contiguous().view(torch.int64))
        assert torch.equal(cr.count, torch.clamp(cr16.count, max=4))
        out[m] = (cr, cr16, hit, occ)
    for a, b in zip(out["brute"], out["blocks"]):
        assert torch.equal(a.raw.view(torch.int64) if a.raw.dtype == torch.float64 else a.raw,
                           b.raw.view(torch.int64) if b.raw.dtype == torch.float64 else b.raw)
        if hasattr(a, "count"):
            assert torch.equal(a.count, b.count)
    assert torch.equal(out["brute"][0].hits.view(torch.int64), out["blocks"][0].hits.view(torch.int64))
    cr16 = out["blocks"][1]
    assert int((cr16.count == 16).sum()) > n // 8 and int((cr16.count == 0).sum()) > n // 64
    sub = slice(0, n, 64)                                  # and a sample of it against the restatement
    w = _cut(X.crossings(recs, rays[sub], 16, tr[sub]), 16)
    got = {"t": _np(cr16.t)[sub], "object": _np(cr16.object)[sub], "which": _np(cr16.which)[sub], "count": _np(cr16.count)[sub]}
    assert not X.mismatches(got, w)


def _strided(a):
    """`a` as every other row of a device tensor of twice its rows (the rows in between hold other values): not contiguous."""
    a = np.ascontiguousarray(a)
    big = np.full((2 * len(a),) + a.shape[1:], 3, dtype=a.dtype)
    big[::2] = a
    big = _dev(big)
    return big, big[::2]


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def test_non_contiguous_tensors_answer_as_their_contiguous_copies(tor):
    """Every operand a strided view -- rays, t_range, the per-ray mask, max_distance and the states every other row of a tensor of
    514 rows, the points the first four columns of (257, 7) rays: each query works on contiguous copies that its result keeps
    alive, and answers what it answers on .contiguous() copies, bit for bit; a step leaves the caller's strided rays and states
    alone and its result carries the updated copies.  Nine objects (one block of 8 and one more), 257 rays (a workgroup and one)."""
    recs = Q.scene("groups", SCENE_SEED)[:9]
    n = 257
    rays, tr = Q.rays(recs, n, RAY_SEED)
    rng = np.random.default_rng(78)
    (_, s_rays), (_, s_tr), (_, s_mask) = _strided(rays), _strided(tr), _strided(Q.ray_masks(n, RAY_SEED))
    _, s_dmax = _strided(rng.choice([np.inf, 0.5, 4.0], n))
    pts = s_rays.contiguous()[:, :4]
    for t in (s_rays, s_tr, s_mask, s_dmax, pts):
        assert not t.is_contiguous() and t.shape[0] == n
    ctx = _ctx(tor, recs)
    ctx.set_groups(Q.group_words(len(recs)))
    for m in ("brute", "blocks"):
        got = ctx.hit(s_rays, s_tr, None, m, mask=s_mask)
        want = ctx.hit(s_rays.contiguous(), s_tr.contiguous(), None, m, mask=s_mask.contiguous())
        assert got.mode == want.mode and torch.equal(_bits(got.raw), _bits(want.raw)), ("hit", m)
        assert 0 < int((want.object >= 0).sum()) < n
        got = ctx.occluded(s_rays, s_tr, None, TIME_RANGE, m, mask=s_mask)
        want = ctx.occluded(s_rays.contiguous(), s_tr.contiguous(), None, TIME_RANGE, m, mask=s_mask.contiguous())
        assert got.mode == want.mode and torch.equal(got.raw, want.raw) and 0 < int(want.raw.sum()) < n, ("occluded", m)
        got = ctx.crossings(s_rays, 3, s_tr, None, TIME_RANGE, m, s_mask, records=True)
        want = ctx.crossings(s_rays.contiguous(), 3, s_tr.contiguous(), None, TIME_RANGE, m, s_mask.contiguous(), records=True)
        assert got.mode == want.mode and torch.equal(got.count, want.count) and int(want.count.max()) > 1, ("crossings", m)
        assert torch.equal(_bits(got.raw), _bits(want.raw)) and torch.equal(_bits(got.hits), _bits(want.hits)), ("crossings", m)
        got = ctx.nearest(pts, 2, s_dmax, None, TIME_RANGE, m, s_mask)
        want = ctx.nearest(pts.contiguous(), 2, s_dmax.contiguous(), None, TIME_RANGE, m, s_mask.contiguous())
        assert got.mode == want.mode and torch.equal(got.count, want.count) and 0 < int(want.count.sum()) < 2 * n, ("nearest", m)
        assert torch.equal(_bits(got.raw), _bits(want.raw)), ("nearest", m)
        # one step: the strided rays and states are copied, the copies updated and returned
        (big_rays, b_rays), (big_st, b_st) = _strided(rays), _strided(rng.integers(0, 2**63, (n, 4), dtype=np.uint64))
        before_rays, before_st = big_rays.clone(), big_st.clone()
        want = ctx.bounce(b_rays.contiguous(), b_st.contiguous(), None, TIME_RANGE, m, mask=s_mask.contiguous())
        got = ctx.bounce(b_rays, b_st, None, TIME_RANGE, m, mask=s_mask)
        torch.cuda.synchronize()
        assert torch.equal(_bits(big_rays), _bits(before_rays)) and torch.equal(big_st, before_st), ("bounce: the caller's tensors", m)
        assert got.mode == want.mode and torch.equal(_bits(got.raw), _bits(want.raw)) and torch.equal(got.status, want.status), ("bounce", m)
        assert torch.equal(_bits(got.attenuation), _bits(want.attenuation)), ("bounce", m)
        assert torch.equal(_bits(got.rays), _bits(want.rays)) and torch.equal(got.rng, want.rng), ("bounce", m)
        assert got.rays.is_contiguous() and got.rng.is_contiguous() and int((want.status == tor.BOUNCE_SCATTERED).sum()) > 0
        assert not torch.equal(got.rng, b_st)                 # (the step did draw)
