"""Path steps on the MI355X (tor_bounce_device / tor_scatter_device / tor_sky_device / tor_bounce_select_device and the _host twins):
one step equals the numpy restatement (tests/bounce_restatement.py, anchored by tests/test_bounce_query.py) bit for bit, brute force
and blocks; bounce == hit then scatter; the chain -- Context.trace with its defaults and a bare C-ABI loop -- equals
tor_radiance_device, colours and states, and the oracle's sample sums; lists, emission / sky / hook, the empty scene, the host
entries; steps leave renders alone and bad arguments touch nothing.  Every comparison is on the bits (NaN against NaN counts as
equal: a NaN's sign and payload are not part of IEEE results)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bounce_restatement as BR
import hit_restatement as H
import radiance_restatement as RR

pytestmark = pytest.mark.gpu
MODES = ("auto", "brute", "blocks")


def _ctx(tor, recs):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    return ctx


def _cam(tor, cam24):
    return tor.Camera.from_buffer_copy(np.ascontiguousarray(cam24, dtype=np.float64).tobytes())


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _np(t):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def _check_step(res, want, tag):
    """A BounceResult (torch or numpy) against bounce_restatement's dict."""
    get = _np if isinstance(res.raw, torch.Tensor) else np.asarray
    assert not H.mismatches(get(res.raw), want["raw"]), tag
    assert np.array_equal(get(res.status), want["status"]), tag
    assert _eq(get(res.attenuation), want["attenuation"]), tag
    assert _eq(get(res.rays), want["rays"]), tag
    assert np.array_equal(np.asarray(get(res.rng)).view(np.uint64), want["states"]), tag


def _mixed_rays(recs, n, seed):
    """Incoherent rays with times in and around [0, 1], plus rays with a zero direction, a NaN, an infinite and far-off times."""
    odd = np.array([[0, 1, 0, 0, 0, 0, 0.5], [0, 1, 0, 1, 0.2, 0, np.nan], [0, 1, 0, -1, 0.1, 0.3, 7.0], [0, 1, 0, 0.3, -1, 0.1, -3.0],
                    [0, 0.5, 0, 1, 0, 0, np.inf]], dtype=np.float64)
    rays = np.concatenate([H.incoherent_rays(recs, n, seed, (-0.5, 1.5)), odd])
    st = np.asarray(np.random.default_rng(seed + 1).integers(0, 2**63, (rays.shape[0], 4), dtype=np.uint64))
    return rays, st


@pytest.fixture(scope="module")
def rscene(tor):
    return tor.random_scene(0xFACADE).to_records()


@pytest.fixture(scope="module")
def anim120(tor):
    it = iter(tor.Animation(108, 192, 0.005, 0.0, 7.2).scenes(skip=6))
    for _ in range(121):
        cam, scene, _t = next(it)
    return np.frombuffer(bytes(cam), dtype=np.float64).copy(), scene.to_records()


def test_one_step_equals_the_restatement(tor, oracle, rscene, anim120):
    cam24 = oracle.camera()
    cam_rays, cam_st = RR.camera_rays(oracle, cam24, 18, 32, None, 0, 1)
    acam, arecs = anim120
    assert len(arecs) == 1601
    a_rays, a_st = RR.camera_rays(oracle, acam, 12, 20, None, 0, 1)
    group = H.group_scene(5, 300)
    cases = [("camera", rscene, cam_rays, cam_st, None), ("mixed times", rscene, *_mixed_rays(rscene, 1200, 31), (0.0, 1.0)),
             ("time groups", group, *_mixed_rays(group, 800, 33), None), ("anim120 camera", arecs, a_rays, a_st, None),
             ("anim120 mixed", arecs, *_mixed_rays(arecs, 500, 35), (0.25, 0.75))]
    for name, recs, rays, st, tr in cases:
        want = BR.step(oracle, recs, rays, st)
        assert (want["status"] == BR.SCATTERED).any() and (name != "camera" or (want["status"] == BR.MISS).any()), name
        ctx = _ctx(tor, recs)
        for m in MODES:
            res = ctx.bounce(_dev(rays), _dev(st), None, tr, m)
            _check_step(res, want, (name, m, res.mode))
            if m == "brute" or name != "time groups":
                assert res.mode == ("brute force" if m == "brute" else "blocks"), (name, m, res.mode)
            assert tor.last_note() == "bounce: " + res.mode


def test_bounce_equals_hit_then_scatter_and_sky(tor, oracle, rscene):
    rays, st = _mixed_rays(rscene, 3000, 41)
    ctx = _ctx(tor, rscene)
    for m in ("brute", "blocks"):
        r1, s1 = _dev(rays), _dev(st)
        both = ctx.bounce(r1, s1, None, (0.0, 1.0), m)
        assert both.rays is r1 and both.rng is s1                       # contiguous tensors are updated in place
        r2, s2 = _dev(rays), _dev(st)
        hit = ctx.hit(r2, None, (0.0, 1.0), m)
        two = ctx.scatter(r2, hit, s2)
        assert two.mode == "scatter" and tor.last_note() == "scatter"
        torch.cuda.synchronize()
        assert not H.mismatches(_np(both.raw), _np(hit.raw))
        assert torch.equal(both.status, two.status) and _eq(_np(both.attenuation), _np(two.attenuation))
        assert _eq(_np(r1), _np(r2)) and torch.equal(s1, s2)
    # a record the caller changed: perturbed normals, another object's material, objects outside the scene
    raw = H.world_hit(rscene, rays)
    rng = np.random.default_rng(5)
    hitrows = np.nonzero(H.fields(raw)["object"] >= 0)[0]
    nrm = raw[hitrows, 3:6] + rng.normal(scale=0.2, size=(hitrows.size, 3))
    raw[hitrows, 3:6] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    words = raw.view(np.int32)
    words[hitrows[::3], 14] = rng.integers(0, len(rscene), hitrows[::3].size)
    words[hitrows[1::50], 14] = len(rscene)
    words[hitrows[2::50], 14] = 2**31 - 1
    words[hitrows[3::7], 15] ^= 1
    want = BR.scatter(oracle, rscene, rays, raw, st)
    want["raw"] = raw
    _check_step(ctx.scatter(_dev(rays), _dev(raw), _dev(st)), want, "caller's records")
    # the sky of the rays that miss is radiance() at depth 1
    finite = np.isfinite(rays).all(axis=1)
    miss = np.nonzero((H.fields(H.world_hit(rscene, rays))["object"] < 0) & finite)[0]
    assert miss.size > 100
    color, _, _ = ctx.radiance(_dev(rays), _dev(st), 1)
    sky = ctx.sky(_dev(rays), miss.astype(np.int32))
    assert _eq(_np(sky)[miss], _np(color)[miss]) and _eq(_np(sky), BR.sky(rays, miss))
    assert _eq(ctx.sky(rays, miss), BR.sky(rays, miss))                  # numpy in, numpy out


def _c_chain(tor, ctx, rays, st, depth, mode, tr):
    """The bare C-ABI loop: tor_bounce_device + tor_sky_device + tor_bounce_select_device, a full-size array per quantity and a
    shrinking list."""
    L = tor.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = rays.shape[0]
    work, st = rays.clone(), st.clone()
    hits = torch.empty((n, 8), dtype=torch.float64, device="cuda")
    step_att = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    status = torch.empty((n,), dtype=torch.int32, device="cuda")
    sky = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    color = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    att = torch.ones((n, 3), dtype=torch.float64, device="cuda")
    lists = [torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2)]
    cur, n_live = None, n
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    for k in range(depth):
        if n_live == 0:
            break
        assert L.tor_bounce_device(ctx._h, n, p(work), p(st), p(cur), n_live, tr[0], tr[1], tor.HIT_MODES[mode], p(hits), p(step_att),
                                   p(status), s) == 0
        idx = torch.arange(n, device="cuda") if cur is None else cur[:n_live].long()
        miss = idx[status[idx] == tor.BOUNCE_MISS].int()
        if miss.numel():
            assert L.tor_sky_device(ctx._h, n, p(work), p(miss), miss.numel(), p(sky), s) == 0
            color[miss.long()] = sky[miss.long()] * att[miss.long()]
        nxt, n_out = lists[k % 2], C.c_int64(-1)
        assert L.tor_bounce_select_device(ctx._h, n, p(status), p(cur), n_live, p(nxt), C.byref(n_out), s) == 0
        cur, n_live = nxt, int(n_out.value)
        scat = cur[:n_live].long()
        att[scat] = att[scat] * step_att[scat]
    return color, st


@pytest.mark.parametrize("mode", ["brute", "blocks"])
@pytest.mark.parametrize("depth", [0, 1, 2, 50])
def test_the_chain_equals_the_radiance_query_and_the_oracle(tor, oracle, rscene, depth, mode):
    cam24 = oracle.camera()
    nrows, ncols, first, ns = 36, 64, 2, 4
    ctx = _ctx(tor, rscene)
    rays, st = ctx.camera_rays(_cam(tor, cam24), nrows, ncols, first, ns, tor.SEED_SAMPLE)
    rays0 = rays.clone()
    want_c, want_s, _ = ctx.radiance(rays, st.clone(), depth, None, mode)
    st1 = st.clone()
    color, st_out, ran = ctx.trace(rays, st1, depth, mode=mode)
    assert st_out is st1 and torch.equal(rays, rays0)                    # the states in place, the rays untouched
    torch.cuda.synchronize()
    assert torch.equal(color.view(torch.int64), want_c.view(torch.int64)) and torch.equal(st_out, want_s), (depth, mode, ran)
    if depth:
        assert ran == ("brute force" if mode == "brute" else "blocks")
    times = rays[:, 6]
    c2, s2 = _c_chain(tor, ctx, rays, st, depth, mode, (float(times.min()), float(times.max())))
    torch.cuda.synchronize()
    assert torch.equal(c2.view(torch.int64), want_c.view(torch.int64)) and torch.equal(s2, want_s), (depth, mode)
    s, mo = RR.sums_and_moments(color.cpu().numpy(), nrows * ncols, ns)
    want_sum, want_mom = oracle.accumulate(nrows, ncols, first, ns, cam24, rscene, max_depth=depth)
    assert _eq(s, want_sum.reshape(-1, 3)) and _eq(mo, want_mom.reshape(-1, 3))


def test_chain_on_arbitrary_rays_time_groups_and_two_levels(tor, oracle, rscene, anim120):
    for recs, seed in ((rscene, 51), (H.group_scene(5, 300), 52), (RR.three_material_scene(), 53), (anim120[1], 54)):
        rays, st = _mixed_rays(recs, 1500, seed)
        ctx = _ctx(tor, recs)
        for m in ("brute", "blocks"):
            want_c, want_s, _ = ctx.radiance(_dev(rays), _dev(st), 50, None, m)
            color, st_out, _ = ctx.trace(_dev(rays), _dev(st), 50, mode=m)
            assert _eq(_np(color), _np(want_c)) and torch.equal(st_out, want_s), (len(recs), m)


def test_lists(tor, oracle, rscene):
    rays, st = _mixed_rays(rscene, 2000, 61)
    n = rays.shape[0]
    ctx = _ctx(tor, rscene)
    subset = np.sort(np.random.default_rng(7).permutation(n)[:700]).astype(np.int32)      # shuffled, then sorted
    with_junk = np.concatenate([[-1, n, 2**31 - 1, -2**31], subset, [n + 5]]).astype(np.int32)  # entries outside [0, n): skipped
    want = BR.step(oracle, rscene, rays, st, subset)
    L = tor.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    for lst in (subset, with_junk, subset[::-1].copy()):
        r, g = _dev(rays), _dev(st)
        hits = torch.full((n, 8), 7.0, dtype=torch.float64, device="cuda")
        att = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
        status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        dl = _dev(lst)
        for m in (tor.HIT_BRUTE, tor.HIT_BLOCKS):
            r.copy_(_dev(rays)), g.copy_(_dev(st))
            assert L.tor_bounce_device(ctx._h, n, p(r), p(g), p(dl), lst.size, 0.0, 1.0, m, p(hits), p(att), p(status), s) == 0
            listed = np.zeros(n, dtype=bool)
            listed[subset] = True
            assert not H.mismatches(_np(hits)[listed], want["raw"][listed])
            assert np.array_equal(_np(status)[listed], want["status"][listed]) and _eq(_np(att)[listed], want["attenuation"][listed])
            assert _eq(_np(r), want["rays"]) and np.array_equal(_np(g), want["states"])   # (rays not listed: as they were)
            assert (_np(hits)[~listed] == 7.0).all() and (_np(att)[~listed] == 7.0).all() and (_np(status)[~listed] == 7).all()
        # the next list: the listed rays that scattered, in input order
        order = lst[(lst >= 0) & (lst < n)]
        nxt = ctx.bounce_select(status, dl)
        assert np.array_equal(_np(nxt), order[want["status"][order] == BR.SCATTERED])
        # the sky of a list leaves the other rows alone
        sky = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
        ctx.sky(_dev(rays), dl, out=sky)
        assert _eq(_np(sky)[listed], BR.sky(rays, subset)[listed]) and (_np(sky)[~listed] == 7.0).all()
    # every ray: a NULL list
    status = ctx.bounce(_dev(rays), _dev(st)).status
    assert np.array_equal(_np(ctx.bounce_select(status)), np.nonzero(_np(status) == BR.SCATTERED)[0])
    # n_list = 0 and n_rays = 0 are no-ops
    r, g = _dev(rays), _dev(st)
    res = ctx.bounce(r, g, np.zeros(0, dtype=np.int32))
    assert _eq(_np(r), rays) and np.array_equal(_np(g), st) and (res.object == -1).all() and (res.status == 0).all()
    assert ctx.bounce_select(res.status, np.zeros(0, dtype=np.int32)).numel() == 0
    empty = ctx.bounce(torch.empty((0, 7), dtype=torch.float64, device="cuda"), torch.empty((0, 4), dtype=torch.int64, device="cuda"))
    assert empty.status.numel() == 0
    # a compaction across many blocks of the scan: 3 M entries, every third one scattered
    big = (torch.arange(3_000_000, device="cuda") % 3 == 1).to(torch.int32)
    assert torch.equal(ctx.bounce_select(big).long(), torch.nonzero(big == 1).reshape(-1))


def test_emission_sky_and_hook_equal_the_restatement(tor, oracle):
    recs = RR.three_material_scene()
    cam = oracle.camera(look_from=(0, 2, 9), look_at=(0, 0.8, 0), vfov=40.0)
    rays, st = RR.camera_rays(oracle, cam, 18, 32, None, 0, 2)
    n = rays.shape[0]
    emission = np.zeros((len(recs), 3))
    emission[3] = [4.0, 3.0, 2.0]                                          # one lit sphere
    depth = 6
    first_obj, lens = np.full(n, -2, dtype=np.int64), []

    def np_hook(k, index, res):
        lens.append(len(index))
        if k == 0:
            first_obj[index] = H.fields(res["raw"])["object"][index]
    want_c, want_s = BR.trace(oracle, recs, rays, st, depth, sky_fn=lambda r, index: r[index, 3:6] * 0.5 + 0.25, emission=emission,
                              on_bounce=np_hook)
    ctx = _ctx(tor, recs)
    got_obj, got_lens = torch.full((n,), -2, dtype=torch.int64, device="cuda"), []

    def hook(k, index, res):
        got_lens.append(int(index.numel()))
        if k == 0:
            got_obj[index.long()] = res.object[index.long()].long()
    for m in ("brute", "auto"):
        got_lens.clear()
        color, st_out, _ = ctx.trace(_dev(rays), _dev(st), depth, sky=lambda r, index: r[index.long(), 3:6] * 0.5 + 0.25,
                                     emission=torch.from_numpy(emission).cuda(), mode=m, on_bounce=hook)
        assert _eq(_np(color), want_c) and np.array_equal(_np(st_out), want_s), m
        assert got_lens == lens and np.array_equal(_np(got_obj).view(np.int64), first_obj)
    assert (first_obj == 3).sum() > 10                                       # the lit sphere is in view
    # numpy operands: through the device and back
    color, st_out, _ = ctx.trace(rays, st, depth, emission=emission)
    want_c, want_s = BR.trace(oracle, recs, rays, st, depth, emission=emission)
    assert _eq(color, want_c) and st_out.dtype == np.uint64 and np.array_equal(st_out, want_s)


def test_empty_scene_and_host_entries(tor, oracle, rscene):
    rays, st = _mixed_rays(rscene, 600, 71)
    ctx = _ctx(tor, np.zeros((0, 16)))
    for m in MODES:
        r, g = _dev(rays), _dev(st)
        res = ctx.bounce(r, g, None, None, m)
        assert (_np(res.status) == BR.MISS).all() and (_np(res.object) == -1).all() and (_np(res.attenuation) == 0).all()
        assert _eq(_np(r), rays) and np.array_equal(_np(g), st)                           # nothing drawn
        raw = H.world_hit(rscene, rays)
        res = ctx.scatter(_dev(rays), _dev(raw), _dev(st))                                # every object is outside an empty scene
        assert (_np(res.status) == BR.MISS).all() and np.array_equal(_np(res.rng), st)
    ctx = _ctx(tor, rscene)
    idx = np.arange(0, rays.shape[0], 2, dtype=np.int32)
    for index in (None, idx):
        want = BR.step(oracle, rscene, rays, st, index)
        res = ctx.bounce(rays, st, index)                                                 # numpy: tor_bounce_host
        assert isinstance(res.raw, np.ndarray) and res.rng.dtype == np.uint64 and res.mode == "blocks"
        _check_step(res, want, ("host", index is None))
        hit = ctx.hit(rays)
        two = ctx.scatter(rays, hit, st, index)                                           # tor_scatter_host
        want["raw"] = hit.raw
        _check_step(two, want, ("host scatter", index is None))
    assert tor.last_note() == "scatter"


def test_steps_leave_renders_alone_and_bad_arguments_touch_nothing(tor, oracle, rscene):
    ctx = _ctx(tor, rscene)
    cam = _cam(tor, oracle.camera())
    nrows, ncols = 36, 64
    opts = tor.make_options(seeding=tor.SEED_SAMPLE)
    s = torch.cuda.current_stream().cuda_stream
    a = torch.empty((nrows * ncols, 3), dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    ctx.render_device(cam, nrows, ncols, 4, 2.2, 50, opts, a.data_ptr(), s)
    rays, st = ctx.camera_rays(cam, nrows, ncols, 0, 2, tor.SEED_SAMPLE)
    ctx.trace(rays, st.clone(), 50, time_range=(0.3, 0.6))
    ctx.scatter(rays.clone(), ctx.hit(rays), st.clone())
    ctx.render_device(cam, nrows, ncols, 4, 2.2, 50, opts, b.data_ptr(), s)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    L = tor.lib()
    n = rays.shape[0]
    rays0, st0 = rays.clone(), st.clone()
    hits = torch.full((n, 8), 7.0, dtype=torch.float64, device="cuda")
    att = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    lst = torch.arange(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    ok = dict(n=n, rays=rays, rng=st, lst=None, n_list=n, lo=0.0, hi=1.0, mode=0, hits=hits, att=att, status=status)
    for kw in (dict(n=-1), dict(n_list=n - 1), dict(lst=lst, n_list=-1), dict(lo=1.0, hi=0.0), dict(lo=float("nan")), dict(mode=3),
               dict(rays=None), dict(rng=None), dict(hits=None), dict(att=None), dict(status=None)):
        k = dict(ok, **kw)
        rc = L.tor_bounce_device(ctx._h, k["n"], p(k["rays"]), p(k["rng"]), p(k["lst"]), k["n_list"], k["lo"], k["hi"], k["mode"],
                                 p(k["hits"]), p(k["att"]), p(k["status"]), C.c_void_p(s))
        assert rc == tor.ERR_INVALID_ARGUMENT, kw
        if set(kw) <= {"lo", "hi", "mode"}:   # (scatter takes no range and no mode)
            continue
        rc = L.tor_scatter_device(ctx._h, k["n"], p(k["rays"]), p(k["hits"]), p(k["rng"]), p(k["lst"]), k["n_list"], p(k["att"]),
                                  p(k["status"]), C.c_void_p(s))
        assert rc == tor.ERR_INVALID_ARGUMENT, kw
    n_out = C.c_int64(5)
    for args in ((n, p(status), p(None), n - 1, p(lst)), (n, p(status), p(lst), n, p(lst)), (-1, p(status), p(None), -1, p(lst)),
                 (n, p(None), p(None), n, p(lst))):
        assert L.tor_bounce_select_device(ctx._h, *args, C.byref(n_out), C.c_void_p(s)) == tor.ERR_INVALID_ARGUMENT
    assert L.tor_sky_device(ctx._h, n, p(rays), p(None), n - 1, p(att), C.c_void_p(s)) == tor.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert n_out.value == 5 and (hits == 7.0).all() and (att == 7.0).all() and (status == 7).all()
    assert torch.equal(rays, rays0) and torch.equal(st, st0) and torch.equal(lst, torch.arange(n, dtype=torch.int32, device="cuda"))
