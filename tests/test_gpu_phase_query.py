"""Phase-function queries on the MI355X (tor_scene_media_phase, tor_phase_sample_device / _host, tor_phase_eval_device / _host): for
every case of tests/phase_inputs.py every bit of the scattered rays, the attenuation, the density, the advanced states, the
evaluation's value and density is the numpy restatement's (tests/phase_restatement.py, which tests/test_phase_query.py anchors),
through device and host entries, tensors and numpy, lists and out=; the table's lifecycle; trace_media with and without phase
functions and trace_media_direct against restated loops; and two statistical checks on the GPU's own draws, whose tolerances
are derived in tests/test_phase_query.py."""
import math

import numpy as np
import pytest
import torch

import light_restatement as LR
import masked_restatement as MS
import media_inputs as MI
import media_restatement as MR
import phase_inputs as I
import phase_restatement as R

pytestmark = pytest.mark.gpu
_want = {}


def _answer(oracle, name):
    """The restatement's answers of a case: computed once, never changed."""
    if name not in _want:
        _want[name] = (I.answer(oracle, I.BY_NAME[name]), I.evaluation(I.BY_NAME[name]))
    return _want[name]


def _ctx(tor, c):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(c["recs"], dtype=np.float64).reshape(-1, 16)).list())
    ctx.set_media(c["objects"], c["sigma"], c["albedo"])
    ctx.set_media_phase(c["g"])
    return ctx


def _cuda(a, dtype=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _i64(a):
    return _cuda(np.ascontiguousarray(a).view(np.int64), np.int64)


def _sample_np(ps):
    f = (lambda v: v.cpu().numpy()) if isinstance(ps.pdf, torch.Tensor) else np.asarray
    return dict(rays=f(ps.rays), attenuation=f(ps.attenuation), pdf=f(ps.pdf), states=f(ps.rng).view(np.uint64))


def _eval_np(ev):
    f = (lambda v: v.cpu().numpy()) if isinstance(ev.pdf, torch.Tensor) else np.asarray
    return dict(value=f(ev.value), pdf=f(ev.pdf))


@pytest.mark.parametrize("name", I.NAMES)
def test_every_bit_of_the_sample_and_the_evaluation(tor, oracle, name):
    c = I.BY_NAME[name]
    want, wev = _answer(oracle, name)
    ctx = _ctx(tor, c)
    n, M = len(c["rays"]), len(c["objects"])
    rays, t, active, out = _cuda(c["rays"]), _cuda(c["t"]), _i64(c["active"]), _cuda(c["out"])
    states = _i64(c["states"])
    got = ctx.sample_phase(rays, (t, active), states)
    torch.cuda.synchronize()
    assert got.mode == f"{M} media" and tor.last_note() == f"phase sample: {M} media" and got.rng.data_ptr() == states.data_ptr()
    bad = R.mismatches(_sample_np(got), want)
    assert not bad, bad
    new, att = got                                                                  # unpacks as a MediaScatter does
    assert new is got.rays and att is got.attenuation
    ev = ctx.phase(rays, active, out)
    torch.cuda.synchronize()
    assert ev.mode == f"{M} media" and tor.last_note() == f"phase eval: {M} media"
    bad = R.mismatches(_eval_np(ev), wev, keys=("value", "pdf"))
    assert not bad, bad
    # the blocking entries on numpy operands; the caller's states stay
    h = ctx.sample_phase(c["rays"], (c["t"], c["active"].view(np.int64)), c["states"])
    assert isinstance(h.pdf, np.ndarray) and not R.mismatches(_sample_np(h), want) and h.rng is not c["states"]
    he = ctx.phase(c["rays"], c["active"].view(np.int64), c["out"])
    assert not R.mismatches(_eval_np(he), wev, keys=("value", "pdf"))
    # two halves through lists into one out; unlisted rows keep sentinels and states
    first, rest = np.arange(0, n, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)
    states2 = _i64(c["states"])
    got.rays[:], got.attenuation[:], got.pdf[:] = 7.0, 7.0, 7.0
    half = ctx.sample_phase(rays, (t, active), states2, index=_cuda(first, np.int32), out=got)
    torch.cuda.synchronize()
    hs = _sample_np(half)
    assert half.rays.data_ptr() == got.rays.data_ptr() and not R.mismatches(hs, want, first)
    assert (hs["rays"][rest] == 7.0).all() and (hs["attenuation"][rest] == 7.0).all() and (hs["pdf"][rest] == 7.0).all()
    assert np.array_equal(hs["states"][rest], c["states"][rest])
    both = ctx.sample_phase(rays, (t, active), states2, index=_cuda(rest, np.int32), out=half)
    torch.cuda.synchronize()
    assert not R.mismatches(_sample_np(both), want)
    ev.value[:], ev.pdf[:] = 7.0, 7.0
    e1 = ctx.phase(rays, active, out, index=_cuda(first, np.int32), out=ev)
    torch.cuda.synchronize()
    assert (e1.pdf.cpu().numpy()[rest] == 7.0).all() and (e1.value.cpu().numpy()[rest] == 7.0).all()
    e2 = ctx.phase(rays, active, out, index=_cuda(rest, np.int32), out=e1)
    torch.cuda.synchronize()
    assert e2.pdf.data_ptr() == ev.pdf.data_ptr() and not R.mismatches(_eval_np(e2), wev, keys=("value", "pdf"))
    hh = ctx.sample_phase(c["rays"], (c["t"], c["active"].view(np.int64)), c["states"], index=first)
    hb = ctx.sample_phase(c["rays"], (c["t"], c["active"].view(np.int64)), hh.rng, index=rest, out=hh)
    assert hb.pdf is hh.pdf and not R.mismatches(_sample_np(hb), want)
    # in place: the out rays may be the rays
    work = rays.clone()
    ps = tor.PhaseSample(work, torch.zeros((n, 3), dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"),
                         None, "")
    inplace = ctx.sample_phase(work, (t, active), _i64(c["states"]), out=ps)
    torch.cuda.synchronize()
    assert inplace.rays.data_ptr() == work.data_ptr() and not R.mismatches(_sample_np(inplace), want)


@pytest.mark.parametrize("length", [1, 63, 64, 65, 257])
def test_lists_leave_the_other_rays_alone(tor, oracle, length):
    c = I.BY_NAME["row64"]
    want, wev = _answer(oracle, "row64")
    ctx = _ctx(tor, c)
    n = len(c["rays"])
    index = I.lists()[length]
    listed = index[(index >= 0) & (index < n)]
    rest = np.ones(n, dtype=bool)
    rest[listed] = False
    rays, t, active = _cuda(c["rays"]), _cuda(c["t"]), _i64(c["active"])
    states = _i64(c["states"])
    sent = tor.PhaseSample(torch.full((n, 7), 7.0, dtype=torch.float64, device="cuda"), torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda"),
                           torch.full((n,), 7.0, dtype=torch.float64, device="cuda"), None, "")
    got = _sample_np(ctx.sample_phase(rays, (t, active), states, index=_cuda(index, np.int32), out=sent))
    assert not R.mismatches(got, want, listed)
    assert (got["rays"][rest] == 7.0).all() and (got["attenuation"][rest] == 7.0).all() and (got["pdf"][rest] == 7.0).all()
    assert np.array_equal(got["states"][rest], c["states"][rest])
    sev = tor.PhaseEval(torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda"), torch.full((n,), 7.0, dtype=torch.float64, device="cuda"), "")
    ev = _eval_np(ctx.phase(rays, active, _cuda(c["out"]), index=_cuda(index, np.int32), out=sev))
    assert not R.mismatches(ev, wev, listed, keys=("value", "pdf")) and (ev["pdf"][rest] == 7.0).all() and (ev["value"][rest] == 7.0).all()
    hs = ctx.sample_phase(c["rays"], (c["t"], c["active"].view(np.int64)), c["states"], index=index)
    assert not R.mismatches(_sample_np(hs), want, listed) and (hs.pdf[rest] == 0).all() and np.array_equal(hs.rng[rest], c["states"][rest])


def test_the_table_lives_in_the_media_table(tor, oracle):
    c = I.BY_NAME["two_overlap"]
    want, wev = _answer(oracle, "two_overlap")
    ctx = _ctx(tor, c)
    args = (c["rays"], (c["t"], c["active"].view(np.int64)), c["states"])
    sample = lambda: _sample_np(ctx.sample_phase(*args))
    evaluate = lambda: _eval_np(ctx.phase(c["rays"], c["active"].view(np.int64), c["out"]))
    same = lambda: not R.mismatches(sample(), want) and not R.mismatches(evaluate(), wev, keys=("value", "pdf"))
    assert same()
    ctx.set_lights([1], [2.0])
    ctx.set_environment(np.ones((4, 4, 3)))
    assert same()                                                                   # survives set_lights and set_environment
    ctx.upload(tor.Scene.from_records(c["recs"]).list())                            # a byte-identical upload keeps it
    assert same()
    # every refusal leaves the answers unchanged, in the header's order
    for bad, word in ((lambda: ctx.set_media_phase([0.3]), "count"), (lambda: ctx.set_media_phase([0.3, 0.3, 0.3]), "count"),
                      (lambda: ctx.set_media_phase([np.nan, 0.3]), "finite"), (lambda: ctx.set_media_phase([0.3, np.inf]), "finite"),
                      (lambda: ctx.set_media_phase([2.0, np.nan]), "finite"),                  # not finite comes before too large
                      (lambda: ctx.set_media_phase([0.3, 0.991]), "G_MAX"), (lambda: ctx.set_media_phase([-1.0, 0.3]), "G_MAX"),
                      (lambda: ctx.set_media_phase([1e-7, 1.5]), "G_MAX"),                      # too large comes before too small
                      (lambda: ctx.set_media_phase([0.3, 1e-7]), "G_MIN"), (lambda: ctx.set_media_phase([-(2.0 ** -21), 0.3]), "G_MIN")):
        with pytest.raises(tor.TorError, match=word):
            bad()
        assert same()
    ctx.set_media_phase([2.0 ** -20, -0.99])                                        # both bounds are allowed
    ctx.set_media_phase(c["g"])
    assert same()
    # g = None, and set_media again, reset the table to isotropic: hg does not depend on mu, the density is 1 / FOUR_PI
    iso = R.evaluate(c["sigma"], c["albedo"], None, c["rays"], c["active"], c["out"])
    ctx.set_media_phase()
    assert not R.mismatches(evaluate(), iso, keys=("value", "pdf")) and R.mismatches(iso, wev, keys=("value", "pdf"))
    ctx.set_media_phase(c["g"])
    ctx.set_media(c["objects"], c["sigma"], c["albedo"])
    e = evaluate()
    assert not R.mismatches(e, iso, keys=("value", "pdf")) and (e["pdf"][e["pdf"] > 0] == 1.0 / R.FOUR_PI).all()
    # a render before and after the queries gives the same canvas
    cam = tor.camera()
    ctx2 = tor.Context(0)
    ctx2.upload(tor.random_scene().list())
    ctx2.set_media([1, 2], [0.5, 0.25])
    ctx2.set_media_phase([0.7, -0.3])
    stream = torch.cuda.current_stream().cuda_stream
    a = torch.zeros((54, 96, 3), dtype=torch.float64, device="cuda")
    b = torch.zeros_like(a)
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    ctx2.render_device(cam, 54, 96, 4, 2.2, 50, opt, a.data_ptr(), stream)
    torch.cuda.synchronize()
    r = _cuda(MI.physics_rays(512, 3, b_max=3.0)[0])
    m = ctx2.march_media(r, 0.5)
    ps = ctx2.sample_phase(r, m, _i64(MI.states(512)))
    ctx2.phase(r, m, ps.rays)
    ctx2.render_device(cam, 54, 96, 4, 2.2, 50, opt, b.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "a phase query between two renders changed the canvas"
    # a replacing upload clears the table; so does an empty media table; a context without a scene has none
    other = c["recs"].copy()
    other[0, 9] = 1.25
    ctx.upload(tor.Scene.from_records(other).list())
    for refused in (sample, evaluate, lambda: ctx.set_media_phase(c["g"])):
        with pytest.raises(tor.TorError, match="no media table"):
            refused()
    ctx.set_media(c["objects"], c["sigma"], c["albedo"])
    assert not R.mismatches(evaluate(), iso, keys=("value", "pdf"))                 # set again: isotropic
    ctx.set_media([], [])
    with pytest.raises(tor.TorError, match="no media table"):
        ctx.set_media_phase([])
    fresh = tor.Context(0)
    for refused in (lambda: fresh.set_media_phase([0.3]), lambda: fresh.sample_phase(*args),
                    lambda: fresh.phase(c["rays"], c["active"].view(np.int64), c["out"])):
        with pytest.raises(tor.TorError, match="no scene"):
            refused()


# ---- the integrators ------------------------------------------------------------------------------------------------------------------

FLIGHT = lambda u: u / (1.0 - u)                                                    # defined bits (no log)
TRANSMIT = lambda d: 1.0 / (1.0 + d)                                                # ... and no exp
GS = [0.7, -0.3]


def _lit_fog():
    """media_inputs-sized fog: the scene of test_gpu_media_query's trace test (a ground, a metal and a glass ball, two overlapping
    media) plus a lamp above it.  Groups: surfaces 1, the media's boundaries 2, the lamp 4."""
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


def _lit_ctx(tor, phase=True):
    recs, objects, sigma, albedo, rays, groups, emission = _lit_fog()
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(recs).list())
    ctx.set_groups(groups)
    ctx.set_media(objects, sigma, albedo)
    if phase:
        ctx.set_media_phase(GS)
    ctx.set_lights([5], [1.0])
    return ctx


def test_trace_media_without_phase_is_what_it_was_and_with_phase_the_restated_loop(tor, oracle):
    recs, objects, sigma, albedo, rays, groups, emission = _lit_fog()
    st = MI.states(len(rays), 9)
    ctx = _lit_ctx(tor)
    # phase=False (the default): media_restatement.trace, the loop trace_media has always been held to -- whatever g the table holds
    want_c, want_s = MR.trace(oracle, recs, objects, sigma, albedo, rays, st, 5, FLIGHT)
    for kw in ({}, {"phase": False}):
        states = _i64(st)
        color, rng = ctx.trace_media(_cuda(rays), states, max_depth=5, mask=5, free_flight=FLIGHT, **kw)
        torch.cuda.synchronize()
        assert rng.data_ptr() == states.data_ptr()
        assert MR.same_bits(color.cpu().numpy(), want_c).all() and np.array_equal(rng.cpu().numpy().view(np.uint64), want_s)
    # phase=True: the restated loop with the phase sampler at the collisions
    pc, ps = R.trace(oracle, recs, objects, sigma, albedo, GS, rays, st, 5, FLIGHT)
    states = _i64(st)
    color, rng = ctx.trace_media(_cuda(rays), states, max_depth=5, mask=5, free_flight=FLIGHT, phase=True)
    torch.cuda.synchronize()
    assert MR.same_bits(color.cpu().numpy(), pc).all() and np.array_equal(rng.cpu().numpy().view(np.uint64), ps)
    assert not np.array_equal(ps, want_s) and not MR.same_bits(pc, want_c).all() and (pc > 0).any()   # three draws, other directions
    hc, hs = ctx.trace_media(rays, st, max_depth=5, mask=5, free_flight=FLIGHT, phase=True)
    assert MR.same_bits(hc, pc).all() and np.array_equal(hs, ps)


def test_trace_media_direct_is_the_restated_loop(tor, oracle):
    recs, objects, sigma, albedo, rays, groups, emission = _lit_fog()
    n = len(rays)
    st = MI.states(n, 9)
    ctx = _lit_ctx(tor)
    # zero emission: trace_media(phase=True) in colours and states
    pc, ps = R.trace(oracle, recs, objects, sigma, albedo, GS, rays, st, 4, FLIGHT)
    color, rng = ctx.trace_media_direct(_cuda(rays), _i64(st), np.zeros((6, 3)), 1, max_depth=4, mask=5, free_flight=FLIGHT, transmit=TRANSMIT)
    torch.cuda.synchronize()
    assert MR.same_bits(color.cpu().numpy(), pc).all() and np.array_equal(rng.cpu().numpy().view(np.uint64), ps)
    with pytest.raises(ValueError, match="lamp_mask"):
        ctx.trace_media_direct(_cuda(rays), _i64(st), emission, None)
    # one lamp: the loop restated from the hit, scatter, light, media and phase restatements, bit for bit
    direct = dict(emission=emission, light_states=I.derived_states(st), transmit=TRANSMIT,
                  light_sample=lambda points, lst, idx: LR.sample(oracle, recs, [5], [1.0], points, lst, idx, LR.BY_SOLID_ANGLE),
                  occluded=lambda seg, tr, idx: MS.occluded(recs, groups, seg, 1, tr))
    want_c, want_s = R.trace(oracle, recs, objects, sigma, albedo, GS, rays, st, 4, FLIGHT, direct=direct)
    states = _i64(st)
    color, rng = ctx.trace_media_direct(_cuda(rays), states, emission, 1, max_depth=4, mask=5, free_flight=FLIGHT, transmit=TRANSMIT)
    torch.cuda.synchronize()
    got = color.cpu().numpy()
    assert rng.data_ptr() == states.data_ptr() and np.array_equal(rng.cpu().numpy().view(np.uint64), want_s) and np.array_equal(want_s, ps)
    assert MR.same_bits(got, want_c).all(), int((~MR.same_bits(got, want_c).all(axis=1)).sum())
    lit = ((want_c != pc).any(axis=1)).sum()
    assert lit >= 19, lit                                                           # the lamp lights the fog
    hc, hs = ctx.trace_media_direct(rays, st, emission, 1, max_depth=4, mask=5, free_flight=FLIGHT, transmit=TRANSMIT)
    assert MR.same_bits(hc, want_c).all() and np.array_equal(hs, want_s)
    # one collision's contribution by hand from the query outputs: the first iteration chained on numpy operands; with a black
    # sky and max_depth = 2 a path that collided at once has nothing else in its colour (what it hits next was counted here, a
    # second collision is on the last step and samples no light)
    hit = ctx.hit(rays, mask=5)
    u, s1 = ctx.uniform(st, 1)
    tr = np.zeros((n, 2))
    tr[:, 1] = np.where(hit.object >= 0, hit.t, np.inf)
    m = ctx.march_media(rays, FLIGHT(u[:, 0]), tr)
    col = np.nonzero(m.status == 1)[0].astype(np.int32)
    sc = ctx.sample_phase(rays, m, s1, index=col)
    points = np.zeros((n, 4))
    points[col, 0:3], points[col, 3] = sc.rays[col, 0:3], sc.rays[col, 6]
    ls = ctx.sample_lights(points, I.derived_states(st), col, "solid_angle")
    sr = np.zeros((n, 2))
    sr[:, 0], sr[:, 1] = 0.001, 1.0
    occ = ctx.occluded(ls.rays, sr, col, mask=1)
    zr = np.zeros((n, 2))
    zr[:, 1] = 1.0
    depth = ctx.march_media(ls.rays, np.inf, zr, index=col).depth[col]
    ev = ctx.phase(rays, m, ls.rays, index=col)
    pdf, lamp = ls.pdf[col], ls.light[col].astype(np.int64)
    ok = (~occ.occluded[col]) & (lamp >= 0) & (pdf > 0) & np.isfinite(pdf)
    by_hand = np.zeros((n, 3))
    by_hand[col] = np.where(ok[:, None], 1.0 * ev.value[col] * emission[np.maximum(lamp, 0)] * (TRANSMIT(depth) / pdf)[:, None], 0.0)
    black = lambda r, idx: torch.zeros((len(idx), 3), dtype=torch.float64, device="cuda")
    c2, _ = ctx.trace_media_direct(_cuda(rays), _i64(st), emission, 1, max_depth=2, sky=black, mask=5, free_flight=FLIGHT, transmit=TRANSMIT)
    torch.cuda.synchronize()
    print(f"by hand: {col.size} collisions at once, {int(ok.sum())} lit")
    assert col.size >= 20 and ok.sum() >= 5 and MR.same_bits(c2.cpu().numpy()[col], by_hand[col]).all()


# ---- statistics on the GPU's own draws ---------------------------------------------------------------------------------------------------

def test_mean_cosine_and_cdf_bins(tor):
    """4096 draws at g = 0.7 on the GPU: the mean cosine within 5 sqrt((1 - g^2) / 3 / 4096) = 0.0322 of g, and the shares of the 8
    equal bins of [-1, 1] within 5 binomial standard errors of the closed-form CDF (derived in tests/test_phase_query.py,
    test_g_physics_on_the_restatement).  The cosine is dot(unit(in), out), numpy's, from the scattered rays."""
    g = 0.7
    c = I.physics_case(g)
    ctx = _ctx(tor, c)
    ps = ctx.sample_phase(_cuda(c["rays"]), (_cuda(c["t"]), _i64(c["active"])), _i64(c["states"]))
    torch.cuda.synchronize()
    res = _sample_np(ps)
    assert (res["pdf"] > 0).all()
    mu = I.cosines(c, res)
    se = math.sqrt((1.0 - g * g) / 3.0 / 4096)
    print(f"mean cosine {mu.mean():.5f}, expected {g}: {(mu.mean() - g) / se:+.2f} standard errors")
    assert abs(mu.mean() - g) <= 5.0 * se
    edges = np.linspace(-1.0, 1.0, 9)
    p = I.hg_cdf(g, edges[1:]) - I.hg_cdf(g, edges[:-1])
    frac = np.histogram(np.clip(mu, -1.0, 1.0), bins=edges)[0] / 4096.0
    print("bins", np.round(frac, 4), "expected", np.round(p, 4))
    assert (np.abs(frac - p) <= 5.0 * np.sqrt(p * (1.0 - p) / 4096)).all()
