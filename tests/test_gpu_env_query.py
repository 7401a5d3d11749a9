"""Environment-light queries on the MI355X (tor_scene_environment, tor_env_sample_device / _host, tor_env_eval_device / _host): for
every map, point set and direction set of tests/env_inputs.py the rays, densities, texels, colours and generator states are those
of the numpy restatement of include/tor_env.h (tests/env_restatement.py, which tests/test_env_query.py shows to be a sound
sampler), bit for bit; lists, the blocking twins, numpy operands and the map's lifecycle; and Context.trace_environment against
Context.trace on a small open frame under a sky with a sun."""
import numpy as np
import pytest
import torch

import env_inputs as I
import env_restatement as ER

pytestmark = pytest.mark.gpu


def _ctx(tor, g):
    ctx = tor.Context(0)
    ctx.set_environment(g["rgb"], g["imp"])
    return ctx


def _cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np(es):
    """An EnvSample (tensors or arrays) as numpy fields."""
    f = (lambda v: v.cpu().numpy()) if isinstance(es.rays, torch.Tensor) else np.asarray
    return dict(rays=f(es.rays), pdf=f(es.pdf), texel=f(es.texel), color=f(es.color), states=f(es.rng).view(np.uint64))


def _np_eval(ev):
    f = (lambda v: v.cpu().numpy()) if isinstance(ev.color, torch.Tensor) else np.asarray
    return dict(color=f(ev.color), pdf=f(ev.pdf), texel=f(ev.texel))


def _mismatches(got, want, rows=slice(None), keys=("rays", "pdf", "color", "texel", "states")):
    """What differs, bit for bit; in the rays a NaN on both sides counts as equal (the NaN coordinate of the last point)."""
    bad = []
    for k in keys:
        a, b = got[k][rows], want[k][rows]
        same = ER.same_bits(a, b) if a.dtype == np.float64 else (a == b)
        if not same.all():
            bad.append(f"{k}: {int((~same).reshape(same.shape[0], -1).any(axis=1).sum())} rows")
    return bad


EVAL = ("color", "pdf", "texel")


@pytest.mark.parametrize("name", I.MAPS)
def test_samples_in_every_bit_against_the_restatement(tor, oracle, name):
    g = I.case(oracle, name)
    ctx = _ctx(tor, g)
    pts, st = _cuda(g["pts"]), _cuda(g["st"].view(np.int64), np.int64)
    es = ctx.sample_environment(pts, st)
    torch.cuda.synchronize()
    assert es.mode == "env sample" and es.rng.data_ptr() == st.data_ptr()              # the states are updated in place
    got = _np(es)
    bad = _mismatches(got, g["res"])
    assert not bad, bad
    assert np.isnan(got["rays"][-1, 0]) and np.isfinite(got["rays"][-1, 1:]).all()     # a NaN point reaches the origin alone


@pytest.mark.parametrize("name", I.MAPS)
def test_evaluation_in_every_bit_against_the_restatement(tor, oracle, name):
    g = I.case(oracle, name)
    ctx = _ctx(tor, g)
    rays = _cuda(g["dirs"])
    ev = ctx.environment(rays, pdf=True)
    torch.cuda.synchronize()
    assert ev.mode == "env eval" and tor.last_note() == "env eval"
    got = _np_eval(ev)
    bad = _mismatches(got, g["ev"], keys=EVAL)
    assert not bad, bad
    u = slice(len(g["dirs"]) - I.N_UNUSABLE, None)                                     # for an unusable direction every word is defined
    assert (got["texel"][u] == -1).all() and (got["color"][u].view(np.uint64) == 0).all() and (got["pdf"][u].view(np.uint64) == 0).all()
    only = ctx.environment(rays).cpu().numpy()                                         # without pdf: the colours alone
    assert np.array_equal(only.view(np.uint64), g["ev"]["color"].view(np.uint64))


def test_lists_leave_the_others_alone_and_out_is_written_again(tor, oracle):
    g = I.case(oracle, "n257")
    ctx = _ctx(tor, g)
    n = len(g["pts"])
    listed = [0, 5, 64, 130, n - 4, n - 1]
    index = np.array(listed[:3] + [-3, n + 7] + listed[3:], dtype=np.int32)            # two entries outside [0, n) are skipped
    pts, st = _cuda(g["pts"]), _cuda(g["st"].view(np.int64), np.int64)
    first = ctx.sample_environment(pts, st.clone())
    first.rays[:], first.pdf[:], first.texel[:], first.color[:] = 7.0, 7.0, 77, 7.0    # sentinels
    es = ctx.sample_environment(pts, st, index=_cuda(index, np.int32), out=first)
    torch.cuda.synchronize()
    assert es.rays.data_ptr() == first.rays.data_ptr()
    got = _np(es)
    assert not _mismatches(got, g["res"], listed)
    rest = np.ones(n, dtype=bool)
    rest[listed] = False
    assert (got["rays"][rest] == 7.0).all() and (got["pdf"][rest] == 7.0).all() and (got["texel"][rest] == 77).all()
    assert (got["color"][rest] == 7.0).all() and np.array_equal(got["states"][rest], g["st"][rest])
    # an empty list is a no-op
    none = ctx.sample_environment(pts, st, index=np.zeros(0, dtype=np.int32))
    torch.cuda.synchronize()
    assert (none.texel.cpu().numpy() == -1).all() and np.array_equal(none.rng.cpu().numpy().view(np.uint64), got["states"])
    # the evaluation
    rays = _cuda(g["dirs"])
    m = len(g["dirs"])
    elisted = [1, 3, 200, m - 2]
    eidx = _cuda(np.array(elisted + [m, -1], dtype=np.int32), np.int32)
    ev = ctx.environment(rays, pdf=True)
    ev.color[:], ev.pdf[:], ev.texel[:] = 7.0, 7.0, 77
    ev2 = ctx.environment(rays, index=eidx, out=ev, pdf=True)
    torch.cuda.synchronize()
    assert ev2.color.data_ptr() == ev.color.data_ptr()
    got = _np_eval(ev2)
    assert not _mismatches(got, g["ev"], elisted, keys=EVAL)
    rest = np.ones(m, dtype=bool)
    rest[elisted] = False
    assert (got["color"][rest] == 7.0).all() and (got["pdf"][rest] == 7.0).all() and (got["texel"][rest] == 77).all()
    buf = torch.full((m, 3), 5.0, dtype=torch.float64, device="cuda")
    col = ctx.environment(rays, index=eidx, out=buf).cpu().numpy()
    assert (col[rest] == 5.0).all() and np.array_equal(col[elisted].view(np.uint64), g["ev"]["color"][elisted].view(np.uint64))


@pytest.mark.parametrize("name", ("n5", "n257"))
def test_host_twins_and_numpy_operands_equal_the_device_entries(tor, oracle, name):
    """numpy operands go through tor_env_sample_host / tor_env_eval_host: the same bits as the device entries on tensors, and the
    caller's arrays are never written."""
    g = I.case(oracle, name)
    ctx = _ctx(tor, g)
    st = g["st"].copy()
    index = np.arange(0, len(g["pts"]), 2, dtype=np.int32)
    for idx in (None, index):
        host = ctx.sample_environment(g["pts"], st, index=idx)
        assert isinstance(host.rays, np.ndarray) and host.texel.dtype == np.int32 and np.array_equal(st, g["st"])
        dev = ctx.sample_environment(_cuda(g["pts"]), _cuda(g["st"].view(np.int64), np.int64), index=idx)
        torch.cuda.synchronize()
        a, b = _np(host), _np(dev)
        assert not _mismatches(a, b)
        assert not _mismatches(a, g["res"], slice(None) if idx is None else idx)
        eidx = None if idx is None else np.arange(0, len(g["dirs"]), 3, dtype=np.int32)
        he = ctx.environment(g["dirs"], index=eidx, pdf=True)
        de = ctx.environment(_cuda(g["dirs"]), index=eidx, pdf=True)
        assert isinstance(he.color, np.ndarray) and he.texel.dtype == np.int32
        a, b = _np_eval(he), _np_eval(de)
        assert not _mismatches(a, b, keys=EVAL)
        assert not _mismatches(a, g["ev"], slice(None) if eidx is None else eidx, keys=EVAL)
        hc = ctx.environment(g["dirs"], index=eidx)
        assert isinstance(hc, np.ndarray) and np.array_equal(hc.view(np.uint64), a["color"].view(np.uint64))


def test_the_maps_lifecycle(tor, oracle):
    g, g2 = I.case(oracle, "n5"), I.case(oracle, "dyadic4")
    ctx = tor.Context(0)
    pts, st = g["pts"], g["st"]
    for query in (lambda: ctx.sample_environment(pts, st), lambda: ctx.environment(g["dirs"])):
        with pytest.raises(tor.TorError) as e:                            # no map yet
            query()
        assert e.value.code == -1 and "environment map" in str(e.value)
    ctx.set_environment(g["rgb"])                                         # no scene is needed
    want = _np(ctx.sample_environment(pts, st))
    assert not _mismatches(want, g["res"])
    bad_rgb = g["rgb"].copy()
    bad_rgb[1, 1, 1] = -1.0
    nan_rgb = g["rgb"].copy()
    nan_rgb[0, 0, 0] = np.nan
    inf_imp = np.ones((5, 5))
    inf_imp[4, 4] = np.inf
    huge = np.full((5, 5), 1e308)                                         # finite values whose total is not
    for rgb, imp in ((bad_rgb, None), (nan_rgb, None), (g["rgb"], inf_imp), (g["rgb"], -np.ones((5, 5))), (g["rgb"], np.zeros((5, 5))),
                     (g["rgb"], huge), (np.zeros((5, 5, 3)), None)):
        with pytest.raises(tor.TorError) as e:
            ctx.set_environment(rgb, imp)
        assert e.value.code == -1
        assert not _mismatches(_np(ctx.sample_environment(pts, st)), want)     # a refusal changes nothing
    with pytest.raises(ValueError):
        ctx.set_environment(np.zeros((5, 4, 3)))
    with pytest.raises(ValueError):
        ctx.set_environment(g["rgb"], np.ones((4, 4)))
    with pytest.raises(tor.TorError):                                     # n above TOR_ENV_MAX_SIDE
        ctx.set_environment(np.ones((tor.ENV_MAX_SIDE + 1, tor.ENV_MAX_SIDE + 1, 3)))
    # the map survives the upload of a scene, and of a different one
    import light_inputs
    recs, _, _ = light_inputs.table("three")
    ctx.upload(tor.Scene.from_records(recs).list())
    assert not _mismatches(_np(ctx.sample_environment(pts, st)), want)
    ctx.upload(tor.Scene.from_records(I.open_scene()).list())
    assert not _mismatches(_np(ctx.sample_environment(pts, st)), want)
    assert not _mismatches(_np_eval(ctx.environment(g["dirs"], pdf=True)), g["ev"], keys=EVAL)
    # a second set_environment replaces it
    ctx.set_environment(g2["rgb"], g2["imp"])
    assert not _mismatches(_np(ctx.sample_environment(pts, st)), g2["res"])
    # None clears it, and the queries are refused again
    ctx.set_environment(None)
    with pytest.raises(tor.TorError):
        ctx.sample_environment(pts, st)
    with pytest.raises(tor.TorError):
        ctx.environment(g["dirs"])
    ctx.set_environment(g["rgb"])
    assert not _mismatches(_np(ctx.sample_environment(pts, st)), want)


# ---- trace_environment against trace --------------------------------------------------------------------------------------------------
SIDE, SPP, DEPTH, MAP_N = 8, 64, 8, 64
_frames = {}


def _frame(tor):
    """The 8 x 8 frame of env_inputs.open_scene under env_inputs.sun_sky baked into a 64 x 64 map, SPP samples per pixel:
    trace(sky=the map), trace_environment without the direct term, with it, and with MIS, from the same camera rays and states;
    per run the colours, the states and the per-sample luminances (pixels, SPP).  Computed once."""
    if not _frames:
        scene = tor.Scene.from_records(I.open_scene())
        ctx = tor.Context(0)
        ctx.upload(scene.list())
        ctx.set_environment(I.sun_sky(tor.environment_directions(MAP_N)))
        cam = tor.camera(look_from=(0.0, 1.0, 3.0), look_at=(0.0, 0.0, -1.0), vertical_field_of_view=40.0, aspect_ratio=1.0,
                         aperture=0.0, focus_distance=1.0, shutter_open=0.0, shutter_close=0.0)
        rays, rng = ctx.camera_rays(cam, SIDE, SIDE, 0, SPP)
        diffuse = tor.diffuse_objects(scene)
        runs = {"trace": ctx.trace(rays, rng.clone(), DEPTH, sky=lambda r, idx: ctx.environment(r, idx)[idx]),
                "indirect": ctx.trace_environment(rays, rng.clone(), diffuse, DEPTH, direct=False),
                "direct": ctx.trace_environment(rays, rng.clone(), diffuse, DEPTH),
                "mis": ctx.trace_environment(rays, rng.clone(), diffuse, DEPTH, mis=True)}
        torch.cuda.synchronize()
        for k, (color, states, _) in runs.items():
            c = color.cpu().numpy()
            _frames[k] = dict(color=c, states=states.cpu().numpy().view(np.uint64), lum=c.mean(axis=1).reshape(SIDE * SIDE, SPP))
    return _frames


def _mean_and_error(lum):
    """The frame mean and its standard error from the per-pixel sample variances."""
    return lum.mean(), np.sqrt((lum.var(axis=1, ddof=1) / lum.shape[1]).sum()) / lum.shape[0]


def test_without_the_direct_term_it_is_trace_with_the_map_as_the_sky(tor):
    f = _frame(tor)
    a, b = f["trace"], f["indirect"]
    assert (a["color"] > 0).any() and len(np.unique(a["color"])) > 16     # not a frame of zeros
    assert np.array_equal(a["color"].view(np.uint64), b["color"].view(np.uint64))
    assert np.array_equal(a["states"], b["states"])
    for k in ("direct", "mis"):                                           # the environment draws come from a third stream
        assert np.array_equal(a["states"], f[k]["states"])


@pytest.mark.parametrize("which", ("direct", "mis"))
def test_the_direct_term_agrees_with_the_scattered_rays(tor, which):
    """The frame means of trace_environment with next-event estimation (and with MIS) and without it, at the same sample count,
    agree within 5 combined standard errors, the errors from the per-pixel sample variances of the two runs; the seeds are fixed.
    The per-pixel sample variances themselves are recorded in profiles/env_sample_rate.txt, not asserted.
    Measured (8 x 8 pixels, 64 samples each, depth 8): direct=False 1.371 +- 0.202; direct=True 1.446 +- 0.016, with MIS
    1.445 +- 0.016."""
    f = _frame(tor)
    m0, e0 = _mean_and_error(f["indirect"]["lum"])
    m1, e1 = _mean_and_error(f[which]["lum"])
    print(f"direct=False: {m0:.5f} +- {e0:.5f}; {which}: {m1:.5f} +- {e1:.5f}; mean per-pixel sample variance "
          f"{f['indirect']['lum'].var(axis=1, ddof=1).mean():.4g} against {f[which]['lum'].var(axis=1, ddof=1).mean():.4g}")
    assert m1 > 0 and e1 > 0 and e0 > 0 and abs(m1 - m0) <= 5 * np.sqrt(e0 * e0 + e1 * e1)
