"""Ordered multi-hit queries on the MI355X (tor_crossings_device / tor_crossings_host): in every mode and for K in {1, 2, 4, max}
(both capacity variants of the kernel) the t bits, object, which, count and the unused entries of every ray -- and the records
where requested -- are those of the numpy restatement (tests/crossings_restatement.py, held to hand-worked cases and to
hit_restatement by tests/test_crossings_query.py), bit for bit.  What the kernel may break: a crossing lost to the shrinking bound
(a box skipped, a root dropped, a tie decided the wrong way), to a wave's other lanes, or to a mask."""
import numpy as np
import pytest
import torch

import crossings_restatement as X
import hit_restatement as R

pytestmark = pytest.mark.gpu
MODES = ("auto", "brute", "blocks")
KMAX = 16
KS = (1, 2, 4, KMAX)


def _ctx(tor, recs):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    return ctx


def _cuda(a, dtype=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np(res):
    """A CrossingsResult (tensors or arrays) as numpy fields."""
    f = (lambda v: v.cpu().numpy()) if isinstance(res.raw, torch.Tensor) else np.asarray
    return {"t": f(res.t), "object": f(res.object), "which": f(res.which), "count": f(res.count),
            "hits": None if res.hits is None else f(res.hits)}


def _query(ctx, rays, k, t_range=None, time_range=None, mode="auto", index=None, mask=None, records=False, out=None):
    if mask is not None and np.ndim(mask) > 0:
        mask = torch.from_numpy((np.asarray(mask).astype(np.int64) & X.ALL).astype(np.uint32).view(np.int32)).cuda()
    res = ctx.crossings(_cuda(rays), k, _cuda(t_range), index, time_range, mode, mask, records, out)
    torch.cuda.synchronize()
    got = _np(res)
    assert got["t"].shape == (len(rays), k) and got["object"].dtype == np.int32 and got["count"].shape == (len(rays),)
    return got, res.mode


def _cut(want, k):
    """The restatement's first KMAX crossings cut to the first k."""
    return {"t": want["t"][:, :k], "object": want["object"][:, :k], "which": want["which"][:, :k],
            "count": np.minimum(want["total"], k).astype(np.int32)}


def _check(ctx, recs, rays, t_range=None, time_range=None, modes=MODES, ks=KS, want=None, groups=None, mask=None, records=False):
    """Every mode and K against the restatement, bit for bit; returns ({mode: what ran}, the restatement at KMAX)."""
    if want is None:
        want = X.crossings(recs, rays, KMAX, t_range) if mask is None else X.masked_crossings(recs, groups, rays, mask, KMAX, t_range)
    ran = {}
    for m in modes:
        for k in ks:
            got, ran[m] = _query(ctx, rays, k, t_range, time_range, m, mask=mask, records=records)
            w = _cut(want, k)
            bad = X.mismatches(got, w, got["hits"], X.records(recs, rays, w) if records else None)
            assert not bad, f"mode {m} (ran: {ran[m]}), K = {k}: {bad}"
            unused = np.arange(k)[None, :] >= got["count"][:, None]
            assert (got["object"][unused] == -1).all() and (got["t"][unused] == 0).all() and (got["which"][unused] == 0).all()
    return ran, want


@pytest.fixture(scope="module")
def rscene(tor):
    return tor.random_scene(0xFACADE).to_records()


@pytest.fixture(scope="module")
def anim_frame(tor):
    cam, scene, _ = next(iter(tor.Animation(108, 192).scenes(skip=6)))
    return np.frombuffer(bytes(cam), dtype=np.float64).copy(), scene.to_records()


def test_random_scene_camera_and_incoherent_rays(tor, oracle, rscene):
    ctx = _ctx(tor, rscene)
    cam_rays = R.camera_rays(oracle, oracle.camera(), 108, 192)[::105][:197]
    assert len(cam_rays) == 197
    rays = R.incoherent_rays(rscene, 4096, 1)
    # every other ray starts among the small spheres and runs nearly level: those cross many of them (uniform directions leave
    # the layer of spheres after one or two)
    low = np.arange(1, 4096, 2)
    rays[low, 1] = np.random.default_rng(101).uniform(0.05, 0.45, low.size)
    rays[low, 4] *= 0.05
    want = X.crossings(rscene, rays, KMAX)
    # truncation and the shrinking bound are exercised at K = 4, and so are short lists and misses
    assert (want["total"] > 4).mean() >= 0.10, (want["total"] > 4).mean()
    assert ((want["total"] >= 1) & (want["total"] <= 3)).mean() >= 0.10
    assert (want["total"] == 0).any()
    ran, _ = _check(ctx, rscene, rays, want=want)
    assert ran["auto"] == "blocks" and ran["blocks"] == "blocks" and ran["brute"] == "brute force"
    _check(ctx, rscene, cam_rays)


def test_animation_frame_two_level_layout(tor, anim_frame):
    cam, recs = anim_frame
    assert len(recs) == 1601
    lay = tor.debug_accel_layout(tor.Scene.from_records(recs).list(), min(0.0, cam[22]), max(0.0, cam[23]))
    assert lay is not None and lay[3], "the animation frame should have a two-level culling layout"
    ran, want = _check(_ctx(tor, recs), recs, R.incoherent_rays(recs, 4096, 2))
    assert ran["auto"] == "blocks" and (want["total"] > 4).any()


def test_time_groups_most_rays_outside_the_time_range(tor):
    recs = R.group_scene(5, 699)
    assert len(recs) % 8 != 0
    rays = R.incoherent_rays(recs, 4096, 3, (-1.0, 2.5))
    ran, want = _check(_ctx(tor, recs), recs, rays, time_range=(0.5, 0.75), ks=(1, 4, KMAX))   # most rays walk
    assert ran["blocks"] == "blocks" and ((rays[:, 6] < 0.5) | (rays[:, 6] > 0.75)).mean() > 0.8
    assert (want["total"] > 4).any()


@pytest.mark.parametrize("which", ["anim", "random"])
def test_range_ends_on_a_surface(tor, rscene, anim_frame, which):
    """Origin outside sphere j, direction towards its centre.  t_max is stepped -2 .. +2 ulps across the root of the ray's K-th
    crossing (K = 2: the far side of the sphere, unless something else comes first) and t_min across the first root: both compares
    are strict, so the crossing is there exactly from step +1 (t_max) and up to step -1 (t_min).  The first 200 small static
    spheres of the animation frame; random_scene has 86 of them, all taken."""
    rng = np.random.default_rng(41)
    recs = anim_frame[1] if which == "anim" else rscene
    small = [j for j, rec in enumerate(recs) if rec[0] == 0 and abs(rec[9]) <= 0.5][:200]
    assert len(small) == (200 if which == "anim" else 86)
    base = []
    for j in small:
        c, r = recs[j, 1:4], abs(recs[j, 9])
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        o = c + (r + rng.uniform(0.02, 0.3)) * u
        base.append([*o, *(c - o), 0.0])
    base = np.asarray(base)
    first = X.crossings(recs, base, 2)
    assert (first["count"] == 2).all()
    rays, tr = [], []
    for e, ray in enumerate(base):
        for steps in (-2, -1, 0, 1, 2):
            for lo, hi in ((0.001, first["t"][e, 1]), (first["t"][e, 0], np.inf)):
                edge = hi if lo == 0.001 else lo
                for _ in range(abs(steps)):
                    edge = np.nextafter(edge, np.inf if steps > 0 else -np.inf)
                rays.append(ray)
                tr.append([0.001, edge] if lo == 0.001 else [edge, np.inf])
    rays, tr = np.asarray(rays), np.asarray(tr)
    want = X.crossings(recs, rays, KMAX, tr)
    by = want["total"].reshape(len(base), 5, 2)
    assert (by[:, 3, 0] == by[:, 2, 0] + 1).all() and (by[:, 2, 1] == by[:, 1, 1] - 1).all()   # the crossing appears / disappears
    _check(_ctx(tor, recs), recs, rays, tr, want=want, ks=(1, 2, 4))


def test_coincident_duplicates_entries_k_and_k_plus_1_share_one_t(tor, rscene):
    """Duplicates of the first 60 objects appended: a ray towards object j crosses j and its duplicate at one t.  With K odd the
    K-th and (K + 1)-th crossings tie: the lower index must be the one kept, whichever is visited first."""
    recs = np.concatenate([rscene, rscene[:60]])
    o = np.tile([13.0, 2.0, 3.0], (60, 1))
    rays = np.concatenate([o, rscene[:60, 1:4] - o, np.zeros((60, 1))], axis=1)
    want = X.crossings(recs, rays, KMAX)
    assert want["tied"].all()
    for k in (1, 3):
        w = _cut(want, k)
        tie = [e for e in range(60) if want["total"][e] > k and want["t"][e, k - 1] == want["t"][e, k]]
        assert len(tie) > 20 and all(w["object"][e, k - 1] < want["object"][e, k] for e in tie)
    _check(_ctx(tor, recs), recs, rays, want=want, ks=(1, 2, 3, 4, 5, KMAX))


def test_rays_from_inside_spheres_and_the_hollow_glass_ball(tor, rscene):
    rng = np.random.default_rng(6)
    j = rng.integers(0, len(rscene), 4096)
    o = rscene[j, 1:4] + rng.uniform(-0.05, 0.05, (4096, 3)) * np.abs(rscene[j, 9:10])
    rays = np.concatenate([o, rng.normal(size=(4096, 3)), rng.uniform(0, 1, (4096, 1))], axis=1)
    _, want = _check(_ctx(tor, rscene), rscene, rays, ks=(1, 4))
    assert (want["which"][:, 0][want["count"] > 0] == 1).mean() > 0.5     # the way out comes first
    # hollow glass balls: radii r and -0.9 r, concentric, among enough other spheres for a culling layout
    balls = rscene[[j for j, rec in enumerate(rscene) if rec[0] == 0 and abs(rec[9]) <= 0.5][:40]].copy()
    inner = balls.copy()
    inner[:, 9] *= -0.9
    recs = np.concatenate([rscene, inner])
    o = balls[:, 1:4] + np.array([0.0, 3.0, 0.1])
    rays = np.concatenate([o, balls[:, 1:4] - o, np.zeros((40, 1))], axis=1)
    want = X.crossings(recs, rays, KMAX)
    through = [e for e in range(40) if want["total"][e] >= 4 and want["object"][e, 1] >= len(rscene)]
    assert len(through) > 20
    for e in through[:5]:
        assert want["which"][e, :4].tolist() == [0, 0, 1, 1] and want["object"][e, 2] == want["object"][e, 1]
    _check(_ctx(tor, recs), recs, rays, want=want, records=True)


def test_degenerate_rays_and_small_scenes(tor, rscene):
    rng = np.random.default_rng(9)
    recs = np.concatenate([rscene, R.group_scene(10, 200)])
    rays = R.incoherent_rays(recs, 2048, 10, (0.0, 1.0))
    rays[0::7, 3:6] = 0.0                                   # zero directions
    rays[1::7, 6] = np.nan                                  # NaN times
    rays[2::7, 0:3] += rng.choice([-1.0, 1.0], (len(rays[2::7]), 3)) * 1e5   # far origins, beyond `reach`: they walk
    rays[3::7, 3:6] *= 1e-150                               # tiny directions
    tr = np.tile([0.001, np.inf], (len(rays), 1))           # t_max = +inf
    tr[4::7, 0] = rng.choice([-2.0, -np.inf, np.nan, 0.0], len(tr[4::7]))
    tr[5::7, 1] = rng.choice([np.nan, 5.0, 0.0], len(tr[5::7]))
    ctx = _ctx(tor, recs)
    _check(ctx, recs, rays, tr, time_range=(0.0, 1.0), ks=(1, 4, KMAX))
    far = R.far_grazing_rays(rscene, 20)[::5]
    _check(_ctx(tor, rscene), rscene, far, time_range=(0.0, 1.0), ks=(2, KMAX))
    probe = R.incoherent_rays(R.group_scene(11, 40), 500, 12)
    for n_obj in (0, 1, 9):
        small = R.group_scene(11, 40)[:n_obj]
        ran, want = _check(_ctx(tor, small), small, probe, ks=(1, 4, KMAX))
        assert all(ran[m].startswith("brute force") for m in MODES)
        assert n_obj == 0 or want["total"].any()


@pytest.mark.parametrize("n", [0, 1, 63, 65, 257])
def test_batch_sizes(tor, rscene, n):
    ctx = _ctx(tor, rscene)
    rays = R.incoherent_rays(rscene, max(n, 1), 13)[:n]
    _check(ctx, rscene, rays, ks=(1, 4, KMAX))
    if n == 0:   # numpy in, too
        res = ctx.crossings(np.zeros((0, 7)), 3, records=True)
        assert res.t.shape == (0, 3) and res.count.shape == (0,) and res.hits.shape == (0, 3, 8) and res.mode == "nothing to do"


def test_lists_keep_what_is_not_listed(tor, rscene):
    ctx = _ctx(tor, rscene)
    n, k = 3001, 4
    rays = R.incoherent_rays(rscene, n, 43)
    want = _cut(X.crossings(rscene, rays, KMAX), k)
    dr = _cuda(rays)
    for m in MODES:
        for idx, listed_ids in ((np.arange(1, n, 3, dtype=np.int32), np.arange(1, n, 3)),
                                (np.array([n, 5, -1, 2999, 64, n + 100, 0, -(1 << 31), 3000, (1 << 31) - 1], dtype=np.int32),
                                 [5, 2999, 64, 0, 3000])):
            out = ctx.crossings(dr, k, index=np.zeros(0, dtype=np.int32), mode=m, records=True)   # an empty list: a no-op
            torch.cuda.synchronize()
            assert out.mode == "nothing to do" and int(out.count.sum()) == 0 and bool((out.object == -1).all())
            out.raw.fill_(7.0)
            out.count.fill_(7)
            out.hits.fill_(7.0)
            res = ctx.crossings(dr, k, index=idx, mode=m, records=True, out=out)
            torch.cuda.synchronize()
            assert res.raw is out.raw
            got = _np(res)
            listed = np.zeros(n, dtype=bool)
            listed[listed_ids] = True
            sub = {name: want[name][listed] for name in want}
            bad = X.mismatches({name: got[name][listed] for name in sub}, sub, got["hits"][listed], X.records(rscene, rays[listed], sub))
            assert not bad, (m, bad)
            assert (got["count"][~listed] == 7).all() and (res.raw.cpu().numpy()[~listed] == 7.0).all() \
                and (got["hits"][~listed] == 7.0).all(), m


def test_masks_that_differ_inside_every_wave(tor, rscene):
    groups = tor.groups_by_material(rscene)
    rays = R.incoherent_rays(rscene, 4096, 44)
    masks = np.random.default_rng(45).choice(np.array([0, 1, 2, 5, X.ALL], dtype=np.uint32), len(rays))
    for w0 in range(0, len(rays), 64):
        assert np.unique(masks[w0:w0 + 64]).size > 1
    ctx = _ctx(tor, rscene)
    before, _ = _query(ctx, rays, 4, mode="blocks")
    ctx.set_groups(groups)
    ran, want = _check(ctx, rscene, rays, groups=groups, mask=masks, records=True)
    assert (want["count"][masks == 0] == 0).all() and ran["blocks"] == "blocks"
    plain = X.crossings(rscene, rays, KMAX)
    assert (want["total"] != plain["total"]).mean() > 0.2
    # glass only: the restatement on the sub-list, `object` in the full numbering
    glass = np.nonzero(groups == (1 << tor.MAT_DIELECTRIC))[0]
    sub = X.crossings(rscene[glass], rays, 4)
    got, _ = _query(ctx, rays, 4, mask=1 << tor.MAT_DIELECTRIC)
    sub["object"] = np.where(sub["object"] >= 0, glass[np.maximum(sub["object"], 0)], -1).astype(np.int32)
    assert not X.mismatches(got, sub) and (sub["count"] > 0).sum() > 50
    # the unmasked call reads no group state: the same result before and after set_groups, whatever the words
    ctx.set_groups(np.zeros(len(rscene), dtype=np.uint32))
    after, mode = _query(ctx, rays, 4, mode="blocks")
    assert mode == "blocks" and not X.mismatches(after, before) and not X.mismatches(before, _cut(plain, 4))
    nothing, _ = _query(ctx, rays, 4, mask=X.ALL - 1)                     # a masked call does read them
    assert (nothing["count"] == 0).all()


@pytest.mark.parametrize("which", ["random", "anim", "groups"])
def test_device_side_consistency_with_hit_and_occluded(tor, rscene, anim_frame, which):
    """2^18 rays, brute and blocks, all on the device: (1) crossing 0 and its record are ctx.hit's answer and count == 0 exactly on a
    miss; (2) count > 0 is ctx.occluded's bit; (3) K = 4 chained ctx.hit calls with t_min := the last t give crossings 1 .. 3 on the
    rays the RESTATEMENT reports free of equal-t crossings (crossings_restatement.tied_rays over all 2^18 rays, before anything runs
    on the device): at most 1 % may be excluded, and none on random_scene, which has no duplicates.  The device's own K = 5 answer
    must show equal t values on exactly those rays."""
    recs = {"random": rscene, "anim": anim_frame[1], "groups": R.group_scene(15)}[which]
    n = 1 << 18
    rays = R.incoherent_rays(recs, n, 16, (0.0, 1.0))
    tied_want = X.tied_rays(recs, rays, 4)
    assert tied_want.mean() <= 0.01 and (which != "random" or not tied_want.any())
    clear = torch.from_numpy(~tied_want).cuda()
    ctx = _ctx(tor, recs)
    rt = torch.from_numpy(rays).cuda()
    for m in ("brute", "blocks"):
        cr5 = ctx.crossings(rt, 5, None, None, (0.0, 1.0), m)
        cr = ctx.crossings(rt, 4, None, None, (0.0, 1.0), m, records=True)
        hit = ctx.hit(rt, None, (0.0, 1.0), m)
        occ = ctx.occluded(rt, None, None, (0.0, 1.0), m)
        torch.cuda.synchronize()
        assert cr.mode == hit.mode == {"brute": "brute force", "blocks": "blocks"}[m]
        assert torch.equal(cr.hits[:, 0].view(torch.int64), hit.raw.view(torch.int64)), f"{which}, {m}: record 0 is not hit()'s"
        assert torch.equal(cr.object[:, 0], hit.object) and torch.equal(cr.t[:, 0].view(torch.int64), hit.t.view(torch.int64))
        assert torch.equal(cr.count == 0, hit.object < 0)
        assert torch.equal(cr.count > 0, occ.occluded)
        assert torch.equal(cr.raw.view(torch.int64), cr5.raw[:, :4].contiguous().view(torch.int64))
        k_idx = torch.arange(1, 5, device="cuda")[None, :]
        tied = ((cr5.t[:, 1:] == cr5.t[:, :-1]) & (k_idx < cr5.count[:, None])).any(dim=1)
        assert torch.equal(tied, ~clear), f"{which}, {m}: the device's equal-t rays are not the restatement's"
        tr = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        tr[:, 0], tr[:, 1] = 0.001, float("inf")
        for k in range(4):
            h = ctx.hit(rt, tr, (0.0, 1.0), m)
            torch.cuda.synchronize()
            assert torch.equal(h.object[clear], cr.object[clear, k]), f"{which}, {m}: chained hit {k}"
            assert torch.equal(h.t[clear].view(torch.int64), cr.t[clear, k].contiguous().view(torch.int64)), f"{which}, {m}: chained hit {k}"
            found = h.object >= 0
            tr[:, 0] = torch.where(found, h.t, tr[:, 0])
            tr[:, 1] = torch.where(found, tr[:, 1], torch.full_like(tr[:, 1], -1.0))   # a ray that has missed stays a miss
        assert int((cr.count == 4).sum()) > 10000 and int((cr.count == 0).sum()) > 1000


def test_host_entry_equals_device_entry(tor, rscene):
    ctx = _ctx(tor, rscene)
    rng = np.random.default_rng(17)
    rays = R.incoherent_rays(rscene, 5000, 17)
    tr = np.stack([rng.choice([0.001, 1.0], len(rays)), rng.choice([np.inf, 6.0, 1.5], len(rays))], axis=1)
    masks = rng.choice(np.array([1, 5, X.ALL], dtype=np.uint32), len(rays))
    ctx.set_groups(tor.groups_by_material(rscene))
    for m in MODES:
        for k, mask in ((3, None), (KMAX, masks)):
            host = ctx.crossings(rays, k, tr, mode=m, mask=mask, records=True)   # numpy in: tor_crossings_host
            assert isinstance(host.raw, np.ndarray) and host.object.dtype == np.int32 and host.hits.shape == (5000, k, 8)
            dev, ran = _query(ctx, rays, k, tr, mode=m, mask=mask, records=True)
            assert host.mode == ran and not X.mismatches(_np(host), dev, host.hits, dev["hits"]), (m, k)
            idx = np.arange(0, 5000, 2, dtype=np.int32)
            host.count[:] = 7
            again = ctx.crossings(rays, k, tr, index=idx, mode=m, mask=mask, records=True, out=host)   # keeps what is not listed
            assert np.array_equal(again.count[0::2], dev["count"][0::2]) and (again.count[1::2] == 7).all()
    assert (host.count > 0).mean() > 0.05
    with pytest.raises(tor.TorError) as e:
        tor.Context(0).crossings(rays, 2)
    assert "no scene" in str(e.value)


def test_host_entry_waits_and_a_query_between_renders_changes_no_canvas(tor, rscene):
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    side = torch.cuda.Stream()
    buf = torch.zeros((270, 480, 3), dtype=torch.float64, device="cuda")
    rays = R.incoherent_rays(rscene, 4096, 21)
    want = _cut(X.crossings(rscene, rays, KMAX), 4)
    with torch.cuda.stream(side):
        ctx.render_device(cam, 270, 480, 64, 2.2, 50, tor.make_options(seeding=tor.SEED_SAMPLE), buf.data_ptr(), side.cuda_stream)
    res = ctx.crossings(rays, 4)   # blocking host entry: waits for the render on the other stream instead of refusing it
    assert not X.mismatches(_np(res), want)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=tor.ACCEL_BLOCKS | tor.ACCEL_F32)
    a = torch.zeros((54, 96, 3), dtype=torch.float64, device="cuda")
    b = torch.zeros_like(a)
    ctx.render_device(cam, 54, 96, 8, 2.2, 50, opt, a.data_ptr(), stream)
    torch.cuda.synchronize()
    for m in MODES:
        got, _ = _query(ctx, rays, KMAX, time_range=(-3.0, 0.5), mode=m, records=True)
    ctx.render_device(cam, 54, 96, 8, 2.2, 50, opt, b.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "a query between two renders changed the canvas"
    assert not X.mismatches(got, _cut(X.crossings(rscene, rays, KMAX), KMAX))
