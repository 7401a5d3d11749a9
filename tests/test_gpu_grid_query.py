"""Heterogeneous media on the MI355X (tor_scene_media_grid, tor_media_grid_march_device / _host, tor_media_grid_density_device / _host,
and tor_media_march_device on a table with grid media): for every case of tests/grid_inputs.py every bit of status, t, depth,
active, rho and cell is the numpy restatement's (tests/grid_restatement.py, which tests/test_grid_query.py anchors), through device
and host entries, tensors and numpy, lists and out=; the lookup; the grid-masked homogeneous march; the scatter and phase entries
fed a GridMarch; transmittance; trace_media and trace_media_direct with one and with two grid media against the restated loops,
bit for bit; the lifecycle; the refusals that need a context; and one statistics check whose tolerance is derived in
tests/grid_inputs.py."""
import numpy as np
import pytest
import torch

import grid_inputs as I
import grid_restatement as R
import light_restatement as LR
import masked_restatement as MS
import media_inputs as MI
import media_restatement as MR
import phase_inputs as PI
import phase_restatement as PR

pytestmark = pytest.mark.gpu
_want = {}
INF = float("inf")


def _answer(name):
    """The restatement's march of a case: computed once, never changed."""
    if name not in _want:
        _want[name] = I.answer(I.BY_NAME[name])
    return _want[name]


def _ctx(tor, c):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(c["recs"], dtype=np.float64).reshape(-1, 16)).list())
    ctx.set_media(c["objects"], c["sigma"], c.get("albedo"))
    ctx.set_media_grid(c["grid"]["medium"], c["density"], c["box"])
    return ctx


def _cuda(a, dtype=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _i64(a):
    return _cuda(np.ascontiguousarray(a).view(np.int64), np.int64)


def _np(m):
    f = (lambda v: v.cpu().numpy()) if isinstance(m.t, torch.Tensor) else np.asarray
    out = dict(status=f(m.status), t=f(m.t), depth=f(m.depth), active=f(m.active), rho=f(m.rho))
    if hasattr(m, "cell"):
        out["cell"] = f(m.cell)
    return out


@pytest.mark.parametrize("name", I.NAMES)
def test_every_bit_of_the_march(tor, name):
    c, want = I.BY_NAME[name], _answer(name)
    ctx = _ctx(tor, c)
    n, m_ = len(c["rays"]), c["grid"]["medium"]
    dims = "x".join(str(v) for v in c["grid"]["n"])
    assert ctx.media_grids() == [m_]
    got_dims, got_box, word = ctx.media_grid_info(m_)
    assert got_dims == c["grid"]["n"] and word == 1 << m_ and np.array_equal(got_box, np.asarray(c["grid"]["lo"] + c["grid"]["hi"], dtype=np.float64))
    rays, tau, tr = _cuda(c["rays"]), _cuda(c["tau"]), _cuda(c["t_range"])
    m = ctx.march_media_grid(rays, tau, m_, tr)
    torch.cuda.synchronize()
    assert m.mode == f"medium {m_}, {dims}" and tor.last_note() == f"media grid march: medium {m_}, {dims}" and m.medium == m_
    bad = R.mismatches(_np(m), want)
    assert not bad, bad
    host = ctx.march_media_grid(c["rays"], c["tau"], m_, c["t_range"])             # the blocking entry on numpy operands
    assert isinstance(host.t, np.ndarray) and not R.mismatches(_np(host), want)
    # two halves through lists, the second into the first's result
    first = np.arange(0, n, 2, dtype=np.int32)
    rest = np.arange(1, n, 2, dtype=np.int32)
    half = ctx.march_media_grid(rays, tau, m_, tr, index=_cuda(first, np.int32))
    both = ctx.march_media_grid(rays, tau, m_, tr, index=_cuda(rest, np.int32), out=half)
    torch.cuda.synchronize()
    assert both.t.data_ptr() == half.t.data_ptr() and both.cell.data_ptr() == half.cell.data_ptr() and not R.mismatches(_np(both), want)
    hh = ctx.march_media_grid(c["rays"], c["tau"], m_, c["t_range"], index=first)
    hb = ctx.march_media_grid(c["rays"], c["tau"], m_, c["t_range"], index=rest, out=hh)
    assert hb.t is hh.t and not R.mismatches(_np(hb), want)


@pytest.mark.parametrize("name", ["g357", "box_offset", "moving", "negative_radius", "edges", "g64x3x2"])
def test_every_bit_of_the_lookup(tor, name):
    c = I.BY_NAME[name]
    ctx = _ctx(tor, c)
    pts = I.lookup_points(c)
    wc, wv = R.density(c["recs"], c["objects"], c["grid"], pts)
    assert (wc >= 0).sum() >= 5 and (wc < 0).sum() >= 20
    cell, value = ctx.media_density(_cuda(pts), c["grid"]["medium"])
    torch.cuda.synchronize()
    assert tor.last_note().startswith(f"media grid density: medium {c['grid']['medium']}, ")
    assert np.array_equal(cell.cpu().numpy(), wc) and np.array_equal(MR.bits(value.cpu().numpy()), MR.bits(wv))
    hc, hv = ctx.media_density(pts, c["grid"]["medium"])
    assert np.array_equal(hc, wc) and np.array_equal(MR.bits(hv), MR.bits(wv))
    listed = np.arange(0, len(pts), 3, dtype=np.int32)
    cell[:], value[:] = 77, 7.0
    c2, v2 = ctx.media_density(_cuda(pts), c["grid"]["medium"], index=_cuda(listed, np.int32), out=(cell, value))
    torch.cuda.synchronize()
    rest = np.ones(len(pts), dtype=bool)
    rest[listed] = False
    assert c2.data_ptr() == cell.data_ptr() and np.array_equal(c2.cpu().numpy()[listed], wc[listed]) and (c2.cpu().numpy()[rest] == 77).all()
    assert np.array_equal(MR.bits(v2.cpu().numpy()[listed]), MR.bits(wv[listed])) and (v2.cpu().numpy()[rest] == 7.0).all()
    # the density where a march collides is the cell's: rho == sigma * density[cell]
    want = _answer(name)
    col = want["status"] == 1
    sg = float(c["sigma"][c["grid"]["medium"]])
    assert np.array_equal(MR.bits(want["rho"][col]), MR.bits(sg * c["density"].reshape(-1)[want["cell"][col]]))


@pytest.mark.parametrize("length", [1, 63, 64, 65, 257])
def test_lists_leave_the_other_rays_alone(tor, length):
    c, want = I.BY_NAME["wave16"], _answer("wave16")
    ctx = _ctx(tor, c)
    n = len(c["rays"])
    index = I.lists()[length]
    listed = index[(index >= 0) & (index < n)]
    rays, tau, tr = _cuda(c["rays"]), _cuda(c["tau"]), _cuda(c["t_range"])
    first = ctx.march_media_grid(rays, tau, 0, tr)
    first.status[:], first.t[:], first.depth[:], first.active[:], first.rho[:], first.cell[:] = 77, 7.0, 7.0, 77, 7.0, 77   # sentinels
    m = ctx.march_media_grid(rays, tau, 0, tr, index=_cuda(index, np.int32), out=first)
    torch.cuda.synchronize()
    got = _np(m)
    assert not R.mismatches(got, want, listed)
    rest = np.ones(n, dtype=bool)
    rest[listed] = False
    assert (got["status"][rest] == 77).all() and (got["t"][rest] == 7.0).all() and (got["depth"][rest] == 7.0).all()
    assert (got["active"][rest] == 77).all() and (got["rho"][rest] == 7.0).all() and (got["cell"][rest] == 77).all()
    hm = ctx.march_media_grid(c["rays"], c["tau"], 0, c["t_range"], index=index)
    assert not R.mismatches(_np(hm), want, listed) and (hm.t[rest] == 0).all() and (hm.cell[rest] == -1).all()


@pytest.mark.parametrize("name,grid_media", [("nested3", [1]), ("row64", [0, 5, 63]), ("two_overlap", [0, 1])])
def test_the_homogeneous_march_leaves_grid_media_out(tor, name, grid_media):
    c = MI.BY_NAME[name]
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(c["recs"]).list())
    ctx.set_media(c["objects"], c["sigma"], c["albedo"])
    plain = MI.answer(c)
    assert not MR.march_mismatches(_np(ctx.march_media(c["rays"], c["tau"], c["t_range"])), plain)
    for m in grid_media:
        ctx.set_media_grid(m, np.ones((2, 2, 2)))
    assert ctx.media_grids() == sorted(grid_media)
    want = R.march_with_grids(c["recs"], c["objects"], c["sigma"], grid_media, c["rays"], c["tau"], c["t_range"])
    got = ctx.march_media(_cuda(c["rays"]), _cuda(c["tau"]), _cuda(c["t_range"]))
    torch.cuda.synchronize()
    assert not MR.march_mismatches(_np(got), want) and MR.march_mismatches(want, plain)
    assert not MR.march_mismatches(_np(ctx.march_media(c["rays"], c["tau"], c["t_range"])), want)
    for m in grid_media:                                                           # removing the grids gives the table back
        ctx.set_media_grid(m, None)
    assert ctx.media_grids() == [] and not MR.march_mismatches(_np(ctx.march_media(c["rays"], c["tau"], c["t_range"])), plain)


def test_scatter_and_phase_take_a_grid_march(tor, oracle):
    c, want = I.BY_NAME["g2"], _answer("g2")                                       # two media, the grid on medium 1
    ctx = _ctx(tor, c)
    gs = [0.6, -0.4]
    ctx.set_media_phase(gs)
    assert ctx.media_grids() == [1]                                                # set_media_phase keeps the grid
    n = len(c["rays"])
    col = np.nonzero(want["status"] == 1)[0].astype(np.int32)
    assert col.size >= 29 and (want["active"][col] == 2).all()
    st = MI.states(n)
    rays = _cuda(c["rays"])
    m = ctx.march_media_grid(rays, _cuda(c["tau"]), 1)
    ws = MR.scatter(oracle, c["sigma"], c["albedo"], c["rays"], want["t"], want["active"], st, col)
    s1 = _i64(st)
    sc = ctx.scatter_media(rays, m, s1, index=_cuda(col, np.int32))
    torch.cuda.synchronize()
    assert MR.same_bits(sc.rays.cpu().numpy()[col], ws["rays"][col]).all() and MR.same_bits(sc.attenuation.cpu().numpy()[col], ws["attenuation"][col]).all()
    assert np.array_equal(s1.cpu().numpy().view(np.uint64), ws["states"])
    assert (ws["attenuation"][col] == np.asarray(c["albedo"][1])).all()           # one active medium: its own albedo
    wp = PR.sample(oracle, c["sigma"], c["albedo"], gs, c["rays"], want["t"], want["active"], st, col)
    s2 = _i64(st)
    ps = ctx.sample_phase(rays, m, s2, index=_cuda(col, np.int32))
    torch.cuda.synchronize()
    for k, v in (("rays", ps.rays), ("attenuation", ps.attenuation), ("pdf", ps.pdf)):
        assert MR.same_bits(v.cpu().numpy()[col], wp[k][col]).all(), k
    assert np.array_equal(s2.cpu().numpy().view(np.uint64), wp["states"])
    we = PR.evaluate(c["sigma"], c["albedo"], gs, c["rays"], want["active"], wp["rays"], col)
    ev = ctx.phase(rays, m, ps.rays, index=_cuda(col, np.int32))
    torch.cuda.synchronize()
    assert MR.same_bits(ev.value.cpu().numpy()[col], we["value"][col]).all() and MR.same_bits(ev.pdf.cpu().numpy()[col], we["pdf"][col]).all()
    hm = ctx.march_media_grid(c["rays"], c["tau"], 1)                              # ... and on numpy operands
    hs = ctx.sample_phase(c["rays"], hm, st, index=col)
    assert MR.same_bits(hs.rays[col], wp["rays"][col]).all() and np.array_equal(hs.rng, wp["states"])


# ---- the integrators ------------------------------------------------------------------------------------------------------------------

FLIGHT = lambda u: u / (1.0 - u)                                                    # defined bits (no log)
TRANSMIT = lambda d: 1.0 / (1.0 + d)                                                # ... and no exp
GS = [0.7, -0.3]


def _lit_fog():
    """The lit fog of tests/test_gpu_phase_query.py: a ground, a metal and a glass ball, two overlapping media (objects 3 and 4), a
    lamp above.  Groups: surfaces 1, the media's boundaries 2, the lamp 4."""
    recs = np.asarray([MI._sphere((0, -100.5, -1), 100.0), MI._sphere((1.2, 0, -1), 0.5, 1), MI._sphere((-1.2, 0, -1), 0.5, 2),
                       MI._sphere((0, 0, -1), 0.9), MI._sphere((0.6, 0.3, -1.2), 0.7), MI._sphere((0.2, 2.2, -0.8), 0.4)], dtype=np.float64)
    recs[1, 11:15] = [0.8, 0.6, 0.2, 0.3]
    g = np.random.default_rng(77)
    n = 256
    rays = np.zeros((n, 7))
    rays[:, 2] = 1.5
    rays[:, 3:6] = np.stack([g.uniform(-1.6, 1.6, n), g.uniform(-0.6, 0.9, n), np.full(n, -2.5)], axis=1)
    rays[:, 6] = g.random(n)
    emission = np.zeros((6, 3))
    emission[5] = [4.0, 4.0, 3.0]
    return recs, [3, 4], [0.8, 1.7], [[0.9, 0.8, 0.7], [0.3, 0.5, 0.95]], rays, [1, 1, 1, 2, 2, 4], emission


_DENS = {1: I._distinct((4, 4, 4), 31) * 1.5, 0: I._distinct((3, 5, 2), 32)}
_BOX = {1: None, 0: [-0.8, -0.9, -0.7, 0.9, 0.8, 0.85]}


def _lit_ctx(tor, grid_media):
    recs, objects, sigma, albedo, rays, groups, emission = _lit_fog()
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(recs).list())
    ctx.set_groups(groups)
    ctx.set_media(objects, sigma, albedo)
    ctx.set_media_phase(GS)
    ctx.set_lights([5], [1.0])
    for m in grid_media:
        ctx.set_media_grid(m, _DENS[m], _BOX[m])
    grids = [R.make_grid(recs, objects, m, _DENS[m], _BOX[m]) for m in grid_media]
    return ctx, grids


class _Counting:
    """The loaded library behind a proxy that notes which entries are called (and the n_draws of tor_rng_uniform_device)."""

    def __init__(self, real):
        self._real, self.names, self.draws = real, [], []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("tor_") or name in ("tor_last_error", "tor_last_note"):
            return fn

        def entry(*args):
            self.names.append(name)
            if name == "tor_rng_uniform_device":
                self.draws.append(args[5])
            return fn(*args)
        return entry


@pytest.mark.parametrize("grid_media", [[1], [0, 1]])
def test_trace_media_with_grids_is_the_restated_loop(tor, oracle, grid_media):
    recs, objects, sigma, albedo, rays, groups, emission = _lit_fog()
    st = MI.states(len(rays), 9)
    ctx, grids = _lit_ctx(tor, grid_media)
    assert ctx.media_grids() == grid_media
    plain = MR.trace(oracle, recs, objects, sigma, albedo, rays, st, 4, FLIGHT)
    for phase in (False, True):
        want_c, want_s = R.trace(oracle, recs, objects, sigma, albedo, GS, grids, rays, st, 4, FLIGHT, phase=phase)
        states = _i64(st)
        color, rng = ctx.trace_media(_cuda(rays), states, max_depth=4, mask=5, free_flight=FLIGHT, phase=phase)
        torch.cuda.synchronize()
        assert rng.data_ptr() == states.data_ptr() and np.array_equal(rng.cpu().numpy().view(np.uint64), want_s)
        assert MR.same_bits(color.cpu().numpy(), want_c).all(), int((~MR.same_bits(color.cpu().numpy(), want_c).all(axis=1)).sum())
        assert (want_c > 0).any() and not np.array_equal(want_s, plain[1])            # 1 + K uniforms per iteration: other states
    hc, hs = ctx.trace_media(rays, st, max_depth=4, mask=5, free_flight=FLIGHT, phase=True)
    assert MR.same_bits(hc, want_c).all() and np.array_equal(hs, want_s)
    # the lamp lights the fog through the grids: the shadow segment's depth is the table's plus each grid's
    direct = dict(emission=emission, light_states=PI.derived_states(st), transmit=TRANSMIT,
                  light_sample=lambda points, lst, idx: LR.sample(oracle, recs, [5], [1.0], points, lst, idx, LR.BY_SOLID_ANGLE),
                  occluded=lambda seg, tr, idx: MS.occluded(recs, groups, seg, 1, tr))
    dc, ds = R.trace(oracle, recs, objects, sigma, albedo, GS, grids, rays, st, 4, FLIGHT, phase=True, direct=direct)
    states = _i64(st)
    color, rng = ctx.trace_media_direct(_cuda(rays), states, emission, 1, max_depth=4, mask=5, free_flight=FLIGHT, transmit=TRANSMIT)
    torch.cuda.synchronize()
    got = color.cpu().numpy()
    assert np.array_equal(rng.cpu().numpy().view(np.uint64), ds) and np.array_equal(ds, want_s)
    assert MR.same_bits(got, dc).all(), int((~MR.same_bits(got, dc).all(axis=1)).sum())
    lit = int((dc != want_c).any(axis=1).sum())
    assert lit >= 15, lit
    # the first iteration chained by hand: the earliest collision of the independent sources
    n = len(rays)
    hit = ctx.hit(rays, mask=5)
    u, _ = ctx.uniform(st, 1 + len(grid_media))
    tr = np.zeros((n, 2))
    tr[:, 1] = np.where(hit.object >= 0, hit.t, np.inf)
    best = ctx.march_media(rays, FLIGHT(u[:, 0]), tr)
    t, won_by = np.where(best.status == 1, best.t, tr[:, 1]), np.where(best.status == 1, -1, -2)
    for j, m in enumerate(grid_media):
        g = ctx.march_media_grid(rays, FLIGHT(u[:, 1 + j]), m, np.stack([np.zeros(n), t], axis=1))
        assert (g.t[g.status == 1] <= t[g.status == 1]).all()                      # a collision cannot pass the bound
        t, won_by = np.where(g.status == 1, g.t, t), np.where(g.status == 1, m, won_by)
    assert all((won_by == m).sum() >= 5 for m in grid_media), [(m, int((won_by == m).sum())) for m in grid_media]


def test_without_a_grid_trace_media_issues_the_launches_it_always_did(tor):
    recs, objects, sigma, albedo, rays, groups, emission = _lit_fog()
    st = MI.states(len(rays), 9)
    ctx, _ = _lit_ctx(tor, [])
    real = tor.lib()
    try:
        tor._lib = proxy = _Counting(real)
        ctx.trace_media(_cuda(rays), _i64(st), max_depth=3, mask=5, free_flight=FLIGHT)
        ctx.trace_media_direct(_cuda(rays), _i64(st), emission, 1, max_depth=3, mask=5, free_flight=FLIGHT, transmit=TRANSMIT)
        torch.cuda.synchronize()
    finally:
        tor._lib = real
    assert not [n for n in proxy.names if "grid" in n] and set(proxy.draws) == {1} and len(proxy.draws) >= 4
    assert proxy.names.count("tor_media_march_device") >= len(proxy.draws)          # (and the shadow segments' marches)
    # the sequence, entry by entry: per iteration hit, uniform, march, then the sky of the misses, the surfaces' scatter and the
    # collisions' scatter where there are any -- trace_media (3 iterations) --, then trace_media_direct's with the phase sample
    # and, but for the last iteration, light sample, shadow ray, segment march and phase value.  On these 256 rays every
    # iteration of either integrator has misses, surface hits and collisions, so the sequence is a literal: three iterations
    # each, nothing before, between or after them (an entry that is not of the loop would show as x).
    letter = {"tor_hit_device": "H", "tor_hit_masked_device": "H", "tor_rng_uniform_device": "U", "tor_media_march_device": "M",
              "tor_sky_device": "S", "tor_scatter_device": "B", "tor_media_scatter_device": "C", "tor_phase_sample_device": "P",
              "tor_light_sample_device": "L", "tor_occluded_device": "O", "tor_occluded_masked_device": "O",
              "tor_phase_eval_device": "E"}
    seq = "".join(letter.get(n, "x") for n in proxy.names)
    print("entries without a grid:", seq)
    assert seq == "HUMSBC" * 3 + "HUMSBPLOME" * 2 + "HUMSBP", seq
    assert seq.count("U") == len(proxy.draws)
    ctx.set_media_grid(1, _DENS[1])
    try:
        tor._lib = proxy = _Counting(real)
        ctx.trace_media(_cuda(rays), _i64(st), max_depth=3, mask=5, free_flight=FLIGHT)
        torch.cuda.synchronize()
    finally:
        tor._lib = real
    assert proxy.names.count("tor_media_grid_march_device") == len(proxy.draws) >= 2 and set(proxy.draws) == {2}


def test_transmittance_adds_the_grid_depths(tor):
    recs, objects, sigma, albedo, rays, groups, emission = _lit_fog()
    ctx, grids = _lit_ctx(tor, [0, 1])
    p, q = rays[:, 0:3], rays[:, 0:3] + rays[:, 3:6]
    seg, tr = ctx.shadow_segments(p, q, rays[:, 6], 0.0)
    depth = R.depth_through(recs, objects, sigma, grids, seg, tr)
    assert np.array_equal(MR.bits(ctx.transmittance(p, q, rays[:, 6])), MR.bits(np.exp(-depth))) and (depth > 0).sum() >= 50
    vis = ctx.visible(p, q, rays[:, 6], mask=1)
    assert np.array_equal(MR.bits(ctx.transmittance(p, q, rays[:, 6], mask=1)), MR.bits(np.exp(-depth) * vis))
    tt = ctx.transmittance(_cuda(p), _cuda(q), _cuda(rays[:, 6]))
    assert np.allclose(tt.cpu().numpy(), np.exp(-depth), rtol=1e-14)
    assert (depth != MR.march(recs, objects, sigma, seg, np.inf, tr)["depth"]).sum() >= 50   # not the homogeneous table's


# ---- lifecycle and refusals ------------------------------------------------------------------------------------------------------------

def test_the_grids_follow_the_media_tables_lifecycle(tor):
    c, want = I.BY_NAME["g2"], _answer("g2")
    ctx = _ctx(tor, c)
    scene = tor.Scene.from_records(c["recs"])
    march = lambda: _np(ctx.march_media_grid(c["rays"], c["tau"], 1, c["t_range"]))
    ctx.set_lights([1], [2.0])
    ctx.set_environment(np.ones((4, 4, 3)))
    ctx.set_media_phase([0.5, 0.0])
    assert ctx.media_grids() == [1] and not R.mismatches(march(), want)            # survives lights, environment and phase
    ctx.upload(scene.list())                                                       # a byte-identical upload keeps it
    assert ctx.media_grids() == [1] and not R.mismatches(march(), want)
    # every refusal of tor_scene_media_grid changes nothing
    d = c["density"]
    nan, neg, inf = d.copy(), d.copy(), d.copy()
    nan[0, 0, 0], neg[1, 1, 1], inf[0, 1, 0] = np.nan, -0.5, np.inf
    for bad, word in ((lambda: ctx.set_media_grid(2, d), "outside the media table"), (lambda: ctx.set_media_grid(-1, d), "outside the media table"),
                      (lambda: ctx.set_media_grid(1, np.ones((1025, 1, 1))), "TOR_GRID_MAX_DIM"),
                      (lambda: ctx.set_media_grid(1, d, [0, 0, 0, 1, 1, 0]), "lo < hi"), (lambda: ctx.set_media_grid(1, d, [0, 0, 0, 1, np.inf, 1]), "lo < hi"),
                      (lambda: ctx.set_media_grid(1, d, [0, np.nan, 0, 1, 1, 1]), "lo < hi"),
                      (lambda: ctx.set_media_grid(1, nan), "finite and >= 0"), (lambda: ctx.set_media_grid(1, neg), "finite and >= 0"),
                      (lambda: ctx.set_media_grid(1, inf), "finite and >= 0")):
        with pytest.raises(tor.TorError, match=word):
            bad()
        assert ctx.media_grids() == [1] and not R.mismatches(march(), want)
    L = tor.lib()
    one = np.ones(1)
    assert L.tor_scene_media_grid(ctx._h, 1, 1024, 1024, 17, None, one.ctypes.data) == -1 and "TOR_GRID_MAX_CELLS" in L.tor_last_error().decode()
    assert L.tor_scene_media_grid(ctx._h, 1, 0, 1, 1, None, one.ctypes.data) == -1 and "TOR_GRID_MAX_DIM" in L.tor_last_error().decode()
    assert L.tor_scene_media_grid(ctx._h, 1, 2, 2, 2, None, None) == -1 and "density is NULL" in L.tor_last_error().decode()
    assert not R.mismatches(march(), want)
    # the refusals of the queries that need a context, after tor_media_march_device's: the medium, then its grid
    with pytest.raises(tor.TorError, match="outside the media table"):
        ctx.march_media_grid(c["rays"], 1.0, 2)
    with pytest.raises(tor.TorError, match="has no density grid"):
        ctx.march_media_grid(c["rays"], 1.0, 0)
    with pytest.raises(tor.TorError, match="has no density grid"):
        ctx.media_density(np.zeros((3, 4)), 0)
    with pytest.raises(tor.TorError, match="outside the media table"):
        ctx.media_density(_cuda(np.zeros((3, 4))), 5)
    assert ctx.march_media_grid(np.zeros((0, 7)), 1.0, 1).t.shape == (0,)           # nothing to do is no error
    # replacing a grid: another density, another answer; and back
    ctx.set_media_grid(1, d * 2.0)
    assert R.mismatches(march(), want)
    ctx.set_media_grid(1, d, c["box"])
    assert not R.mismatches(march(), want)
    # a render before and after the queries gives the same canvas
    cam = tor.camera()
    ctx2 = tor.Context(0)
    ctx2.upload(tor.random_scene().list())
    ctx2.set_media([1, 2], [0.5, 0.25])
    ctx2.set_media_grid(0, np.ones((4, 4, 4)))
    stream = torch.cuda.current_stream().cuda_stream
    a = torch.zeros((54, 96, 3), dtype=torch.float64, device="cuda")
    b = torch.zeros_like(a)
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    ctx2.render_device(cam, 54, 96, 4, 2.2, 50, opt, a.data_ptr(), stream)
    torch.cuda.synchronize()
    r = _cuda(MI.physics_rays(512, 3, b_max=3.0)[0])
    ctx2.march_media_grid(r, 0.5, 0)
    ctx2.march_media(r, 0.5)
    ctx2.media_density(r[:, 0:4].contiguous(), 0)
    ctx2.render_device(cam, 54, 96, 4, 2.2, 50, opt, b.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "a grid query between two renders changed the canvas"
    # set_media drops every grid, as it resets g; so does an upload that replaces the scene
    ctx.set_media(c["objects"], c["sigma"], c["albedo"])
    assert ctx.media_grids() == [] and ctx.media_grid_info(1)[0] == (0, 0, 0)
    with pytest.raises(tor.TorError, match="has no density grid"):
        march()
    ctx.set_media_grid(1, d)
    ctx.set_media_grid(0, np.ones((1, 1, 1)))
    assert ctx.media_grids() == [0, 1] and ctx.media_grid_info(0)[2] == 3
    other = c["recs"].copy()
    other[0, 9] = 1.25
    ctx.upload(tor.Scene.from_records(other).list())
    assert ctx.media_grids() == []
    with pytest.raises(tor.TorError, match="no media table"):
        march()
    with pytest.raises(tor.TorError, match="no media table"):
        ctx.set_media_grid(0, d)
    ctx.set_media(c["objects"], c["sigma"], c["albedo"])
    assert ctx.media_grids() == []
    fresh = tor.Context(0)
    with pytest.raises(tor.TorError, match="no scene"):
        fresh.set_media_grid(0, d)
    with pytest.raises(tor.TorError, match="no scene"):
        fresh.march_media_grid(c["rays"], 1.0, 0)


# ---- statistics ----------------------------------------------------------------------------------------------------------------------------

def test_collision_fraction_through_two_slabs(tor):
    """4096 central rays through the unit ball of sigma 1 with the two-slab grid (density 0, then 2), tau = -log1p(-u) of uniforms from
    seeded states: every ray has depth 2, so the collision fraction is 1 - exp(-2) within 5 binomial standard errors (0.0267:
    grid_inputs.PHYSICS_TOL, as tests/test_grid_query.py shows for the restatement), and every collision lies in the dense slab."""
    c = I.physics_case()
    ctx = _ctx(tor, c)
    st = _i64(MI.states(4096, 8))
    u, _ = ctx.uniform(st, 1)
    m = ctx.march_media_grid(_cuda(c["rays"]), -torch.log1p(-u[:, 0]), 0)
    torch.cuda.synchronize()
    frac = float((m.status == 1).double().mean())
    print(f"collision fraction {frac:.4f}, expected {I.PHYSICS_P:.4f}: {(frac - I.PHYSICS_P) / (I.PHYSICS_TOL / 5):+.2f} standard errors")
    assert abs(frac - I.PHYSICS_P) <= I.PHYSICS_TOL
    hit = m.status == 1
    assert (m.cell[hit] == 1).all() and (m.rho[hit] == 2.0).all() and (m.active[hit] == 1).all()
    depth = ctx.march_media_grid(_cuda(c["rays"]), INF, 0).depth
    assert float((depth - 2.0).abs().max()) <= 1e-12
