"""Participating-media queries on the MI355X (tor_scene_media, tor_media_march_device / _host, tor_media_scatter_device / _host,
tor_rng_uniform_device / _host): for every case of tests/media_inputs.py every bit of status, t, depth, active, rho, the scattered
rays, the attenuation, the advanced states and the uniforms is the numpy restatement's (tests/media_restatement.py, which
tests/test_media_query.py anchors), through device and host entries, tensors and numpy, lists and out=; consequences by
composition (the depth from crossings(), trace_media against the restated loop); the table's lifecycle; and two physics checks
whose tolerances are derived in tests/media_inputs.py and below."""
import numpy as np
import pytest
import torch

import media_inputs as I
import media_restatement as R

pytestmark = pytest.mark.gpu
_want = {}


def _answer(name):
    """The restatement's march of a case: computed once, never changed."""
    if name not in _want:
        _want[name] = I.answer(I.BY_NAME[name])
    return _want[name]


def _ctx(tor, c):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(c["recs"], dtype=np.float64).reshape(-1, 16)).list())
    ctx.set_media(c["objects"], c["sigma"], c["albedo"])
    return ctx


def _cuda(a, dtype=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np(m):
    f = (lambda v: v.cpu().numpy()) if isinstance(m.t, torch.Tensor) else np.asarray
    return dict(status=f(m.status), t=f(m.t), depth=f(m.depth), active=f(m.active), rho=f(m.rho))


@pytest.mark.parametrize("name", I.NAMES)
def test_every_bit_of_the_march(tor, name):
    c, want = I.BY_NAME[name], _answer(name)
    ctx = _ctx(tor, c)
    n = len(c["rays"])
    rays, tau, tr = _cuda(c["rays"]), _cuda(c["tau"]), _cuda(c["t_range"])
    m = ctx.march_media(rays, tau, tr)
    torch.cuda.synchronize()
    assert m.mode == f"{len(c['objects'])} media" and tor.last_note() == f"media march: {len(c['objects'])} media"
    bad = R.march_mismatches(_np(m), want)
    assert not bad, bad
    host = ctx.march_media(c["rays"], c["tau"], c["t_range"])                     # the blocking entry on numpy operands
    assert isinstance(host.t, np.ndarray) and not R.march_mismatches(_np(host), want)
    # two halves through lists, the second into the first's result
    first = np.arange(0, n, 2, dtype=np.int32)
    rest = np.arange(1, n, 2, dtype=np.int32)
    half = ctx.march_media(rays, tau, tr, index=_cuda(first, np.int32))
    both = ctx.march_media(rays, tau, tr, index=_cuda(rest, np.int32), out=half)
    torch.cuda.synchronize()
    assert both.t.data_ptr() == half.t.data_ptr() and not R.march_mismatches(_np(both), want)
    hh = ctx.march_media(c["rays"], c["tau"], c["t_range"], index=first)
    hb = ctx.march_media(c["rays"], c["tau"], c["t_range"], index=rest, out=hh)
    assert hb.t is hh.t and not R.march_mismatches(_np(hb), want)


@pytest.mark.parametrize("name", I.NAMES)
def test_every_bit_of_the_scatter_and_the_uniforms(tor, oracle, name):
    c, want = I.BY_NAME[name], _answer(name)
    ctx = _ctx(tor, c)
    n, M = len(c["rays"]), len(c["objects"])
    st = I.states(n)
    active = want["active"].copy()                                                # every ray is listed: an escaped one has active 0
    if n > 4:
        active[1] = np.uint64(1) << np.uint64(M % 64) if M < 64 else np.uint64(0)  # a bit at n_media: no sample
        active[2] = np.uint64((1 << M) - 1)                                        # every medium at once
    t = want["t"]
    ws = R.scatter(oracle, c["sigma"], c["albedo"], c["rays"], t, active, st)
    rays, states = _cuda(c["rays"]), _cuda(st.view(np.int64), np.int64)
    got = ctx.scatter_media(rays, (_cuda(t), _cuda(active.view(np.int64), np.int64)), states)
    torch.cuda.synchronize()
    new, att = got
    assert got.mode == f"{M} media" and got.rng.data_ptr() == states.data_ptr()   # the states are advanced in place
    assert R.same_bits(new.cpu().numpy(), ws["rays"]).all() and R.same_bits(att.cpu().numpy(), ws["attenuation"]).all()
    assert np.array_equal(states.cpu().numpy().view(np.uint64), ws["states"]) and (ws["states"] != st).any(axis=1).all()
    zero = (ws["attenuation"] == 0).all(axis=1) & (ws["rays"] == 0).all(axis=1)
    assert zero[active == 0].all() and (not M < 64 or n <= 4 or zero[1])
    h = ctx.scatter_media(c["rays"], (t, active.view(np.int64)), st)              # the blocking entry; the caller's states stay
    assert R.same_bits(h.rays, ws["rays"]).all() and R.same_bits(h.attenuation, ws["attenuation"]).all()
    assert np.array_equal(h.rng, ws["states"]) and h.rng is not st
    # a list, into the result of the first call: unlisted rays keep rays, attenuation and state
    listed = np.arange(0, n, 3, dtype=np.int32)
    got.rays[:], got.attenuation[:] = 7.0, 7.0
    states2 = _cuda(st.view(np.int64), np.int64)
    again = ctx.scatter_media(rays, (_cuda(t), _cuda(active.view(np.int64), np.int64)), states2, index=_cuda(listed, np.int32), out=got)
    torch.cuda.synchronize()
    rest = np.ones(n, dtype=bool)
    rest[listed] = False
    a_rays, a_st = again.rays.cpu().numpy(), states2.cpu().numpy().view(np.uint64)
    assert again.rays.data_ptr() == got.rays.data_ptr() and R.same_bits(a_rays[listed], ws["rays"][listed]).all()
    assert (a_rays[rest] == 7.0).all() and np.array_equal(a_st[rest], st[rest]) and np.array_equal(a_st[listed], ws["states"][listed])
    # the uniforms: 3 draws per state, then 1 more from where they left off
    wu, wst = R.uniforms(oracle, st, 3)
    states3 = _cuda(st.view(np.int64), np.int64)
    u, s3 = ctx.uniform(states3, 3)
    torch.cuda.synchronize()
    assert tor.last_note() == "rng uniform: 3 draws" and s3.data_ptr() == states3.data_ptr()
    assert np.array_equal(R.bits(u.cpu().numpy()), R.bits(wu)) and np.array_equal(s3.cpu().numpy().view(np.uint64), wst)
    hu, hs = ctx.uniform(st, 3)
    assert np.array_equal(R.bits(hu), R.bits(wu)) and np.array_equal(hs, wst) and (wu >= 0).all() and (wu < 1).all()
    wu1, wst1 = R.uniforms(oracle, wst, 1, listed)
    buf = torch.full((n, 1), 7.0, dtype=torch.float64, device="cuda")
    u1, _ = ctx.uniform(states3, 1, index=_cuda(listed, np.int32), out=buf)
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(u1.cpu().numpy()[listed]), R.bits(wu1[listed])) and (u1.cpu().numpy()[rest] == 7.0).all()
    assert np.array_equal(states3.cpu().numpy().view(np.uint64), wst1)


@pytest.mark.parametrize("length", [1, 63, 64, 65, 257])
def test_lists_leave_the_other_rays_alone(tor, length):
    c, want = I.BY_NAME["row64"], _answer("row64")
    ctx = _ctx(tor, c)
    n = len(c["rays"])
    index = I.lists()[length]
    listed = index[(index >= 0) & (index < n)]
    rays, tau = _cuda(c["rays"]), _cuda(c["tau"])
    first = ctx.march_media(rays, tau)
    first.status[:], first.t[:], first.depth[:], first.active[:], first.rho[:] = 77, 7.0, 7.0, 77, 7.0       # sentinels
    m = ctx.march_media(rays, tau, index=_cuda(index, np.int32), out=first)
    torch.cuda.synchronize()
    got = _np(m)
    assert not R.march_mismatches(got, want, listed)
    rest = np.ones(n, dtype=bool)
    rest[listed] = False
    assert (got["status"][rest] == 77).all() and (got["t"][rest] == 7.0).all() and (got["depth"][rest] == 7.0).all()
    assert (got["active"][rest] == 77).all() and (got["rho"][rest] == 7.0).all()
    hm = ctx.march_media(c["rays"], c["tau"], index=index)
    assert not R.march_mismatches(_np(hm), want, listed) and (hm.t[rest] == 0).all() and (hm.status[rest] == 0).all()


def test_the_depth_is_the_chord_that_crossings_reports(tor):
    """One medium of sigma 1 and tau = inf: depth == (t1 - t0) * sqrt(a), in numpy, from crossings(k=2) of that object alone."""
    c = I.BY_NAME["one"]
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(c["recs"]).list())
    ctx.set_media([0], [1.0])
    rays, _ = I.physics_rays(1024, 5, b_max=0.999)
    tr = np.zeros((len(rays), 2))
    tr[:, 0], tr[:, 1] = -np.inf, np.inf
    x = ctx.crossings(rays, 2, t_range=tr, mask=0xFFFFFFFF)
    m = ctx.march_media(rays, np.inf, tr)
    both = x.count == 2
    d = rays[:, 3:6]
    ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    want = 1.0 * ((x.t[:, 1] - x.t[:, 0]) * ln)
    assert both.sum() >= 1000 and np.array_equal(R.bits(m.depth[both]), R.bits(want[both])) and (m.depth[~both] == 0).all()


def _fog_scene():
    recs = np.asarray([I._sphere((0, -100.5, -1), 100.0), I._sphere((1.2, 0, -1), 0.5, 1), I._sphere((-1.2, 0, -1), 0.5, 2),
                       I._sphere((0, 0, -1), 0.9), I._sphere((0.6, 0.3, -1.2), 0.7)], dtype=np.float64)
    recs[1, 11:15] = [0.8, 0.6, 0.2, 0.3]
    g = np.random.default_rng(77)
    n = 256
    rays = np.zeros((n, 7))
    rays[:, 2] = 1.5
    rays[:, 3:6] = np.stack([g.uniform(-1.6, 1.6, n), g.uniform(-0.6, 0.9, n), np.full(n, -2.5)], axis=1)
    rays[:, 6] = g.random(n)
    return recs, [3, 4], [0.8, 1.7], [[0.9, 0.8, 0.7], [0.3, 0.5, 0.95]], rays


def test_trace_media_is_the_restated_loop(tor, oracle):
    recs, objects, sigma, albedo, rays = _fog_scene()
    flight = lambda u: u / (1.0 - u)                                               # defined bits (no log)
    st = I.states(len(rays), 9)
    want_c, want_s = R.trace(oracle, recs, objects, sigma, albedo, rays, st, 6, flight)
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(recs).list())
    ctx.set_groups([1, 1, 1, 2, 2])
    ctx.set_media(objects, sigma, albedo)
    states = _cuda(st.view(np.int64), np.int64)
    color, rng = ctx.trace_media(_cuda(rays), states, max_depth=6, mask=1, free_flight=flight)
    torch.cuda.synchronize()
    assert rng.data_ptr() == states.data_ptr()
    assert R.same_bits(color.cpu().numpy(), want_c).all() and np.array_equal(rng.cpu().numpy().view(np.uint64), want_s)
    hc, hs = ctx.trace_media(rays, st, max_depth=6, mask=1, free_flight=flight)
    assert R.same_bits(hc, want_c).all() and np.array_equal(hs, want_s)
    assert (want_c > 0).any() and (want_s != st).any(axis=1).all()
    # the first iteration chained by hand on numpy operands: uniform, march up to the hit, the medium's scatter
    hit = ctx.hit(rays, mask=1)
    u, s1 = ctx.uniform(st, 1)
    tr = np.zeros((len(rays), 2))
    tr[:, 1] = np.where(hit.object >= 0, hit.t, np.inf)
    m = ctx.march_media(rays, flight(u[:, 0]), tr)
    col = np.nonzero(m.status == 1)[0].astype(np.int32)
    sc = ctx.scatter_media(rays, m, s1, index=col)
    wm = R.march(recs, objects, sigma, rays, flight(R.uniforms(oracle, st, 1)[0][:, 0]), tr)
    ws = R.scatter(oracle, sigma, albedo, rays, wm["t"], wm["active"], R.uniforms(oracle, st, 1)[1], col)
    assert col.size >= 20 and not R.march_mismatches(_np(m), wm) and R.same_bits(sc.rays, ws["rays"]).all()
    assert np.array_equal(sc.rng, ws["states"])
    # ... and the same chain, finished by hand (the material's scatter at the surfaces, the sky for the rest), is trace_media at
    # max_depth = 1: colours (only a ray that reached nothing has one after one iteration) and states
    surf = np.nonzero((m.status == 0) & (hit.object >= 0))[0].astype(np.int32)
    gone = np.nonzero((m.status == 0) & (hit.object < 0))[0].astype(np.int32)
    s2 = ctx.scatter(rays, hit, sc.rng, index=surf).rng
    by_hand = np.zeros((len(rays), 3))
    by_hand[gone] = ctx.sky(rays, gone)[gone]
    c1, r1 = ctx.trace_media(rays, st, max_depth=1, mask=1, free_flight=flight)
    assert surf.size >= 20 and gone.size >= 5 and R.same_bits(c1, by_hand).all() and np.array_equal(r1, np.asarray(s2).view(np.uint64))
    # transmittance: numpy's exp of the depth, times visible under a mask
    p, q = rays[:, 0:3], rays[:, 0:3] + rays[:, 3:6]
    seg, str_ = ctx.shadow_segments(p, q, rays[:, 6], 0.0)
    depth = R.march(recs, objects, sigma, seg, np.inf, str_)["depth"]
    assert np.array_equal(R.bits(ctx.transmittance(p, q, rays[:, 6])), R.bits(np.exp(-depth)))
    vis = ctx.visible(p, q, rays[:, 6], mask=1)
    assert np.array_equal(R.bits(ctx.transmittance(p, q, rays[:, 6], mask=1)), R.bits(np.exp(-depth) * vis))
    tt = ctx.transmittance(_cuda(p), _cuda(q), _cuda(rays[:, 6]))
    assert np.allclose(tt.cpu().numpy(), np.exp(-depth), rtol=1e-14) and (depth > 0).sum() >= 50


def test_the_table_follows_the_light_tables_lifecycle(tor):
    c, want = I.BY_NAME["two_overlap"], _answer("two_overlap")
    ctx = _ctx(tor, c)
    scene = tor.Scene.from_records(c["recs"])
    march = lambda: _np(ctx.march_media(c["rays"], c["tau"], c["t_range"]))
    ctx.set_lights([1], [2.0])
    ctx.set_environment(np.ones((4, 4, 3)))
    assert not R.march_mismatches(march(), want)                                   # survives set_lights and set_environment
    ctx.upload(scene.list())                                                       # a byte-identical upload keeps it
    assert not R.march_mismatches(march(), want)
    for bad in (lambda: ctx.set_media([0, 0], [1.0, 1.0]), lambda: ctx.set_media([0, 7], [1.0, 1.0]),
                lambda: ctx.set_media([0], [-1.0]), lambda: ctx.set_media([0], [np.nan]), lambda: ctx.set_media([0], [np.inf]),
                lambda: ctx.set_media([0], [1.0], [[1.0, -0.5, 1.0]]), lambda: ctx.set_media([0, 1, 2, 0], [1.0] * 4)):
        with pytest.raises(tor.TorError):
            bad()
        assert not R.march_mismatches(march(), want)                               # nothing changes on a refusal
    # a render before and after a query gives the same canvas
    cam = tor.camera()
    big, _ = tor.random_scene(), None
    ctx2 = tor.Context(0)
    ctx2.upload(big.list())
    ctx2.set_media([1, 2], [0.5, 0.25])
    stream = torch.cuda.current_stream().cuda_stream
    a = torch.zeros((54, 96, 3), dtype=torch.float64, device="cuda")
    b = torch.zeros_like(a)
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    ctx2.render_device(cam, 54, 96, 4, 2.2, 50, opt, a.data_ptr(), stream)
    torch.cuda.synchronize()
    r = _cuda(I.physics_rays(512, 3, b_max=3.0)[0])
    m = ctx2.march_media(r, 0.5)
    ctx2.scatter_media(r, m, _cuda(I.states(512).view(np.int64), np.int64))
    ctx2.render_device(cam, 54, 96, 4, 2.2, 50, opt, b.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "a media query between two renders changed the canvas"
    # a replacing upload clears the table: a march is refused until it is set again; so does an empty table
    other = c["recs"].copy()
    other[0, 9] = 1.25
    ctx.upload(tor.Scene.from_records(other).list())
    with pytest.raises(tor.TorError, match="no media table"):
        march()
    with pytest.raises(tor.TorError, match="no media table"):
        ctx.scatter_media(c["rays"], (c["tau"], np.zeros(len(c["tau"]), dtype=np.int64)), I.states(len(c["tau"])))
    u, _ = ctx.uniform(I.states(4), 2)                                             # the uniforms need no table
    assert u.shape == (4, 2)
    ctx.set_media(c["objects"], c["sigma"], c["albedo"])
    assert R.march_mismatches(march(), want)                                       # another radius: another answer
    ctx.set_media([], [])
    with pytest.raises(tor.TorError, match="no media table"):
        march()
    fresh = tor.Context(0)
    with pytest.raises(tor.TorError, match="no scene"):
        fresh.set_media([0], [1.0])
    with pytest.raises(tor.TorError, match="no scene"):
        fresh.march_media(c["rays"], 1.0)
    assert fresh.uniform(I.states(3), 1)[0].shape == (3, 1)                        # ... and no scene
    fresh.upload(scene.list())
    with pytest.raises(tor.TorError, match="TOR_MEDIA_MAX|n_media"):
        fresh.set_media(list(range(65)), [1.0] * 65)


def test_collision_fraction_of_central_rays(tor):
    """4096 central rays through the unit ball of sigma 0.5 (depth 1), tau = -log1p(-u) of uniforms from seeded states: the
    collision fraction against 1 - exp(-1) within 5 binomial standard errors (0.0377: media_inputs.PHYSICS_TOL)."""
    rays, _ = I.physics_rays(4096, 31)
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(I.PHYSICS_RECS).list())
    ctx.set_media([0], [0.5])
    st = _cuda(I.states(4096, 8).view(np.int64), np.int64)
    u, _ = ctx.uniform(st, 1)
    m = ctx.march_media(_cuda(rays), -torch.log1p(-u[:, 0]))
    torch.cuda.synchronize()
    frac = float((m.status == 1).double().mean())
    print(f"collision fraction {frac:.4f}, expected {I.PHYSICS_P:.4f}: {(frac - I.PHYSICS_P) / (I.PHYSICS_TOL / 5):+.2f} standard errors")
    assert abs(frac - I.PHYSICS_P) <= I.PHYSICS_TOL
    inside = m.t[m.status == 1]
    assert (m.active[m.status == 1] == 1).all() and (m.rho[m.status == 1] == 0.5).all() and bool((inside > 0).all())


def test_depth_against_the_chord(tor):
    """tau = inf: depth against sigma * chord, the chord 2 sqrt(1 - b^2) from the impact parameter the rays were built with, within
    1e-9 relative.  The discriminant's absolute error is about 12 eps |d|^2 (|oc|^2 + r^2) (head of tor_query.hip): with |oc| <= 8,
    r = 1 and b <= 0.9 (disc >= 0.19 |d|^2) the chord's relative error is below 12 * 1.1e-16 * 65 / (2 * 0.19) = 2.3e-13, and the
    construction of the rays adds a few eps of its own; the rest is margin."""
    rays, b = I.physics_rays(4096, 32, b_max=0.9)
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(I.PHYSICS_RECS).list())
    ctx.set_media([0], [0.75])
    m = ctx.march_media(_cuda(rays), float("inf"))
    torch.cuda.synchronize()
    want = 0.75 * 2.0 * np.sqrt(1.0 - b * b)
    rel = np.abs(m.depth.cpu().numpy() - want) / want
    print(f"largest relative error of the depth against the chord: {rel.max():.3e}")
    assert (m.status.cpu().numpy() == 0).all() and rel.max() <= 1e-9
