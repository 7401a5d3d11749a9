"""The BSDF query on the MI355X (tor_bsdf_eval_device / _host): for every item of tests/bsdf_inputs.py value, pdf and kind are those
of the numpy restatement of include/tor_bsdf.h (tests/bsdf_restatement.py, which tests/test_bsdf_query.py shows to be the density
of the reference's scatter), bit for bit; lists, the blocking twin, numpy operands, the refusals; the round trip through
Context.scatter; and Context.trace_direct(glossy=...) against Context.trace on a small frame with a glossy floor and one small
lamp."""
import numpy as np
import pytest
import torch

import bsdf_inputs as I
import bsdf_restatement as R

pytestmark = pytest.mark.gpu
_state = {}


def _case(oracle):
    """The items and the restatement's answer: computed once, never changed."""
    g = I.all_items(oracle)
    if "res" not in g:
        g["res"] = R.evaluate(g["recs"], *g["items"])
    return g


def _ctx(tor, g):
    if "ctx" not in _state:
        ctx = tor.Context(0)
        ctx.upload(tor.Scene.from_records(g["recs"]).list())
        _state["ctx"] = ctx
    return _state["ctx"]


def _cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np(ev):
    """A BsdfEval (tensors or arrays) as numpy fields."""
    f = (lambda v: v.cpu().numpy()) if isinstance(ev.pdf, torch.Tensor) else np.asarray
    return dict(value=f(ev.value), pdf=f(ev.pdf), kind=f(ev.kind))


def _mismatches(got, want, rows=slice(None)):
    """What differs, bit for bit; a NaN on both sides counts as equal (tor_bsdf.h: a NaN's sign and payload are not defined)."""
    bad = []
    for k in ("value", "pdf"):
        same = R.same_bits(got[k][rows], want[k][rows])
        if not same.all():
            bad.append(f"{k}: {int((~same).reshape(same.shape[0], -1).any(axis=1).sum())} items")
    if not np.array_equal(got["kind"][rows], want["kind"][rows]):
        bad.append(f"kind: {int((got['kind'][rows] != want['kind'][rows]).sum())} items")
    return bad


def test_every_bit_against_the_restatement(tor, oracle):
    """The kernel on tensors, the _host twin on numpy operands: value, pdf and kind of every item, in every bit."""
    g = _case(oracle)
    ctx = _ctx(tor, g)
    rin, raw, rout = (_cuda(a) for a in g["items"])
    ev = ctx.bsdf(rin, raw, rout)
    torch.cuda.synchronize()
    assert ev.note == "bsdf eval" and tor.last_note() == "bsdf eval"
    assert ev.kind.dtype == torch.int32 and tuple(ev.value.shape) == (len(rin), 3)
    got = _np(ev)
    assert not _mismatches(got, g["res"]), _mismatches(got, g["res"])
    assert (got["kind"] == R.DENSITY).sum() > 400 and (got["pdf"] > 0).sum() > 250     # not a comparison of zeros
    host = ctx.bsdf(*g["items"])
    assert isinstance(host.pdf, np.ndarray) and host.kind.dtype == np.int32 and host.note == "bsdf eval"
    assert not _mismatches(_np(host), g["res"]), _mismatches(_np(host), g["res"])
    # a HitResult-like object with .raw is taken as its records; d_kind is nullable in the C entry
    class Rec:
        pass
    rec = Rec()
    rec.raw = raw
    assert not _mismatches(_np(ctx.bsdf(rin, rec, rout)), g["res"])
    L = tor.lib()
    n = len(rin)
    value, pdf = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda"), torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    rc = L.tor_bsdf_eval_device(ctx._h, n, rin.data_ptr(), raw.data_ptr(), rout.data_ptr(), None, n, value.data_ptr(), pdf.data_ptr(),
                                None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and R.same_bits(pdf.cpu().numpy(), g["res"]["pdf"]).all() and R.same_bits(value.cpu().numpy(), g["res"]["value"]).all()


@pytest.mark.parametrize("operands", ("tensors", "arrays"))
def test_lists_leave_the_other_items_alone(tor, oracle, operands):
    g = _case(oracle)
    ctx = _ctx(tor, g)
    n = len(g["items"][0])
    rs = np.random.RandomState(3)
    listed = rs.permutation(n)[:n // 3]                                    # a shuffled sub-list, past one block
    index = np.concatenate([listed[:50], [-1, n, n + 700, -2 ** 31], listed[50:]]).astype(np.int32)   # entries outside [0, n) are skipped
    put = _cuda if operands == "tensors" else (lambda a, dtype=np.float64: np.ascontiguousarray(a, dtype=dtype))
    items = [put(a) for a in g["items"]]
    first = ctx.bsdf(*items)
    first.value[:], first.pdf[:], first.kind[:] = 7.0, 7.0, 77              # sentinels
    ev = ctx.bsdf(*items, index=put(index, np.int32), out=first)
    torch.cuda.synchronize()
    assert ev.value is first.value and ev.pdf is first.pdf and ev.kind is first.kind
    got = _np(ev)
    assert not _mismatches(got, g["res"], listed)
    rest = np.ones(n, dtype=bool)
    rest[listed] = False
    assert (got["value"][rest] == 7.0).all() and (got["pdf"][rest] == 7.0).all() and (got["kind"][rest] == 77).all()
    # an empty list is a no-op: nothing is written
    first.value[:], first.pdf[:], first.kind[:] = 5.0, 5.0, 55
    none = _np(ctx.bsdf(*items, index=np.zeros(0, dtype=np.int32), out=first))
    torch.cuda.synchronize()
    assert (none["value"] == 5.0).all() and (none["pdf"] == 5.0).all() and (none["kind"] == 55).all()
    # no items at all
    empty = ctx.bsdf(items[0][:0], items[1][:0], items[2][:0])
    assert tuple(empty.pdf.shape) == (0,)


def test_refusals_in_their_order_with_nothing_written(tor, oracle):
    g = _case(oracle)
    ctx = _ctx(tor, g)
    L = tor.lib()
    err = lambda: L.tor_last_error().decode()
    rin, raw, rout = (_cuda(a[:64]) for a in g["items"])
    value = torch.full((64, 3), 7.0, dtype=torch.float64, device="cuda")
    pdf = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    kind = torch.full((64,), 77, dtype=torch.int32, device="cuda")
    lst = torch.arange(8, dtype=torch.int32, device="cuda")
    a = [rin.data_ptr(), raw.data_ptr(), rout.data_ptr(), value.data_ptr(), pdf.data_ptr()]
    dev = lambda h, n, p, l, nl: L.tor_bsdf_eval_device(h, n, p[0], p[1], p[2], l, nl, p[3], p[4], kind.data_ptr(), None)
    assert dev(None, -1, [None] * 5, None, -1) == -1 and "ctx" in err()                        # ctx first
    assert dev(ctx._h, -1, [None] * 5, None, -1) == -1 and "n_list" not in err()               # then n
    assert dev(ctx._h, 64, [None] * 5, None, -1) == -1 and "n_list < 0" in err()               # then n_list
    assert dev(ctx._h, 64, [None] * 5, None, 8) == -1 and "without a list" in err()            # then the list
    for hole in range(5):                                                                     # then the NULL arrays
        b = list(a)
        b[hole] = None
        assert dev(ctx._h, 64, b, lst.data_ptr(), 8) == -1 and "NULL" in err()
        assert L.tor_bsdf_eval_host(ctx._h, 64, b[0], b[1], b[2], None, 64, b[3], b[4], None) == -1 and "NULL" in err()
    bare = tor.Context(0)                                                                     # a context without a scene: last
    assert dev(bare._h, 64, [None] * 5, lst.data_ptr(), 8) == -1 and "NULL" in err()
    assert dev(bare._h, 64, a, lst.data_ptr(), 8) == -1 and "no scene" in err()
    with pytest.raises(tor.TorError) as e:
        bare.bsdf(rin, raw, rout)
    assert e.value.code == -1 and "no scene" in str(e.value)
    with pytest.raises(tor.TorError):
        bare.bsdf(*(x[:64] for x in g["items"]))
    assert dev(bare._h, 0, [None] * 5, None, 0) == -1 and "no scene" in err()                  # (nothing to do, but still no scene)
    torch.cuda.synchronize()
    assert (value == 7.0).all() and (pdf == 7.0).all() and (kind == 77).all()                 # nothing was written
    # the wrapper's own refusals
    with pytest.raises(ValueError):
        ctx.bsdf(rin, raw, rout[:10])
    with pytest.raises(ValueError):
        ctx.bsdf(rin, raw[:, :7], rout)
    with pytest.raises(ValueError):
        ctx.bsdf(rin, raw, rout, out=object())
    assert dev(ctx._h, 64, a, lst.data_ptr(), 8) == 0                                          # and the same call with a scene runs
    torch.cuda.synchronize()
    assert (pdf[8:] == 7.0).all() and R.same_bits(pdf[:8].cpu().numpy(), g["res"]["pdf"][:8]).all()


def test_scatter_outputs_fed_back_have_a_density_where_they_were_accepted(tor, oracle):
    """(f) of the CPU suite through the library: Context.scatter's rays go straight in as rays_out; SCATTERED Metal rays have
    pdf > 0, ABSORBED ones pdf == 0 (on the objects whose lobe float64 resolves), and the Lambertian ones cos / pi."""
    g = _case(oracle)
    ctx = _ctx(tor, g)
    import light_inputs as LI
    t0, status = g["trip"]
    rin, raw = _cuda(g["items"][0][t0:]), _cuda(g["items"][1][t0:])
    st = _cuda(LI.states(I.N_TRIP, 0xB5DF).view(np.int64), np.int64)
    res = ctx.scatter(rin.clone(), raw, st)
    ev = ctx.bsdf(rin, raw, res.rays)
    torch.cuda.synchronize()
    stat, pdf = res.status.cpu().numpy(), ev.pdf.cpu().numpy()
    assert np.array_equal(stat, status)                                    # the library's scatter is the restated one
    assert R.same_bits(pdf, g["res"]["pdf"][t0:]).all()
    assert (stat == tor.BOUNCE_SCATTERED).sum() >= 100 and (stat == tor.BOUNCE_ABSORBED).sum() >= 10
    assert (pdf[stat == tor.BOUNCE_SCATTERED] > 0).all() and (pdf[stat == tor.BOUNCE_ABSORBED] == 0).all()
    # Lambertian items: the scatter's own direction has the density cos / pi of the restatement, and it is > 0
    n = 256
    rs = np.random.RandomState(11)
    nrm = I._unit(rs.normal(size=(n, 3)))
    lin, lraw, _ = I.pack([I.FLOOR, I.RED] * (n // 2), nrm, -nrm + 0.3 * rs.normal(size=(n, 3)), nrm)
    res = ctx.scatter(lin.copy(), lraw, LI.states(n, 12))
    ev = ctx.bsdf(lin, lraw, res.rays)
    want = R.evaluate(g["recs"], lin, lraw, res.rays)
    assert (res.status == tor.BOUNCE_SCATTERED).all() and not _mismatches(_np(ev), want)
    assert (ev.pdf > 0).sum() >= n - 2                                     # (n + U may round onto the horizon: not excluded)


# ---- trace_direct(glossy=...) against trace ----------------------------------------------------------------------------------------------
SIDE, SPP, DEPTH, BATCHES = 8, 64, 4, 16
LAMP = I.G_LAMP


def _frame(tor):
    """The 8 x 8 frame of bsdf_inputs.glossy_scene, depth 4: every run of the checks below, from camera rays and states of the same streams;
    per run the per-path luminances (pixels, samples).  Computed once."""
    if "frame" not in _state:
        recs, emission = I.glossy_scene()
        scene = tor.Scene.from_records(recs)
        ctx = tor.Context(0)
        ctx.upload(scene.list())
        ctx.set_lights([LAMP])
        ctx.set_groups(np.where(np.arange(len(recs)) == LAMP, 2, 1).astype(np.uint32))    # the lamp has a group of its own
        cam = I.glossy_camera(tor)
        diffuse, glossy = tor.diffuse_objects(scene), tor.glossy_objects(scene)
        assert list(diffuse) == [False, True, True] and list(glossy) == [True, False, False]
        black = lambda rays, idx: torch.zeros((len(idx), 3), dtype=torch.float64, device=rays.device)    # (never asked: no ray escapes)
        f = {}
        lum = lambda c, spp: c.mean(dim=1).reshape(SIDE * SIDE, spp).cpu().numpy()
        rays, rng = ctx.camera_rays(cam, SIDE, SIDE, 0, SPP)
        kw = dict(max_depth=DEPTH, sky=black, lamp_mask=1)
        f["mis"] = lum(ctx.trace_direct(rays, rng.clone(), emission, diffuse, mis=True, glossy=glossy, **kw)[0], SPP)
        f["nee"] = lum(ctx.trace_direct(rays, rng.clone(), emission, diffuse, mis=False, glossy=glossy, **kw)[0], SPP)
        none = np.zeros(len(recs), dtype=bool)
        f["pairs"] = [(ctx.trace_direct(rays, rng.clone(), emission, diffuse, mis=m, **kw)[0].cpu().numpy(),
                       ctx.trace_direct(rays, rng.clone(), emission, diffuse, mis=m, glossy=none, **kw)[0].cpu().numpy())
                      for m in (False, True)]
        big, brng = ctx.camera_rays(cam, SIDE, SIDE, 0, 16 * SPP)
        f["trace"] = lum(ctx.trace(big, brng, DEPTH, sky=black, emission=emission)[0], 16 * SPP)
        # all-zero emission under the open sky, which colours the paths
        recs, _ = I.glossy_scene(enclosed=False)
        ctx.upload(tor.Scene.from_records(recs).list())
        ctx.set_lights([LAMP])
        ctx.set_groups(np.where(np.arange(len(recs)) == LAMP, 2, 1).astype(np.uint32))
        zero = np.zeros((len(recs), 3))
        a = ctx.trace(rays, rng.clone(), DEPTH, emission=zero)
        b = ctx.trace_direct(rays, rng.clone(), zero, diffuse, DEPTH, glossy=glossy)
        c = ctx.trace_direct(rays, rng.clone(), zero, diffuse, DEPTH, mis=True, glossy=glossy, lamp_mask=1)
        torch.cuda.synchronize()
        f["zero"] = [(x[0].cpu().numpy(), x[1].cpu().numpy()) for x in (a, b, c)]
        _state["frame"] = f
    return _state["frame"]


def _mean_and_error(lum):
    """The frame mean and its standard error from BATCHES batches of samples: the scatter of the batches' frame means."""
    batches = lum.reshape(lum.shape[0], BATCHES, -1).mean(axis=(0, 2))
    return float(lum.mean()), float(batches.std(ddof=1) / np.sqrt(BATCHES))


def test_i_all_zero_emission_gives_trace_colours_bit_for_bit(tor):
    (c0, s0), (c1, s1), (c2, s2) = _frame(tor)["zero"]
    assert (c0 > 0).any() and len(np.unique(c0)) > 16                     # the sky coloured the paths: not a frame of zeros
    assert np.array_equal(c0.view(np.uint64), c1.view(np.uint64)) and np.array_equal(c0.view(np.uint64), c2.view(np.uint64))
    assert np.array_equal(s0, s1) and np.array_equal(s0, s2)              # the light draws come from a second stream


def test_ii_glossy_all_false_is_the_default_path(tor):
    """Only the source of cos / pi differs (bsdf() against torch arithmetic): 1e-12 relative, with and without MIS."""
    for default, through_bsdf in _frame(tor)["pairs"]:
        assert (default > 0).sum() >= 300                                  # (the ball fills a twentieth of the frame: not a comparison of zeros)
        assert np.allclose(through_bsdf, default, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("which", ("mis", "nee"))
def test_iii_iv_glossy_trace_direct_agrees_with_trace(tor, which):
    """The frame mean of trace_direct(glossy=...) -- (iii) with MIS, (iv) without -- agrees with plain trace(emission=...) at 16
    times the samples within 4 combined standard errors, each estimated from 16 batches; trace is the unbiased estimator that
    needs none of the new code.  Measured (8 x 8 pixels, depth 4, 64 against 1024 samples per pixel): trace 0.04677 +- 0.00355;
    trace_direct(glossy) with MIS 0.04296 +- 0.00361, without 0.04135 +- 0.00247."""
    f = _frame(tor)
    m0, e0 = _mean_and_error(f["trace"])
    m1, e1 = _mean_and_error(f[which])
    msg = f"trace: {m0:.5f} +- {e0:.5f}; trace_direct(glossy, {which}): {m1:.5f} +- {e1:.5f}"
    print(msg)
    assert m1 > 0 and e1 > 0 and e0 > 0 and abs(m1 - m0) <= 4.0 * np.sqrt(e0 * e0 + e1 * e1), msg
