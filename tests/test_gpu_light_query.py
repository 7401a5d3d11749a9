"""Direct-light sampling queries on the MI355X (tor_scene_lights, tor_light_sample_device / _host, tor_light_pdf_device / _host):
for every light table and point set of tests/light_inputs.py and both strategies the rays, densities, lights, distances and
generator states are those of the numpy restatement of include/tor_lights.h (tests/light_restatement.py, which
tests/test_light_query.py shows to be a sound sampler), bit for bit; lists, the blocking twins, numpy operands and the light
table's lifecycle; and Context.trace_direct against Context.trace on a small enclosed frame with one small lamp."""
import numpy as np
import pytest
import torch

import light_inputs as I
import light_restatement as LR

pytestmark = pytest.mark.gpu
STRATEGIES = {LR.BY_WEIGHT: "weight", LR.BY_SOLID_ANGLE: "solid_angle"}
NOTES = {LR.BY_WEIGHT: "by weight", LR.BY_SOLID_ANGLE: "by solid angle"}
_cases = {}


def _case(oracle, name, strategy):
    """Table, points, states and the restatement's sample and densities: computed once, never changed."""
    key = (name, strategy)
    if key not in _cases:
        recs, lights, weights = I.table(name, oracle)
        pts = I.points(recs, lights)
        st = I.states(len(pts))
        res = LR.sample(oracle, recs, lights, weights, pts, st, None, strategy)
        _cases[key] = dict(recs=recs, lights=lights, weights=weights, pts=pts, st=st, res=res,
                           pdf=LR.pdf(recs, lights, weights, pts, res["light"], None, strategy))
    return _cases[key]


def _ctx(tor, g):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(g["recs"], dtype=np.float64).reshape(-1, 16)).list())
    ctx.set_lights(g["lights"], g["weights"])
    return ctx


def _cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np(ls):
    """A LightSample (tensors or arrays) as numpy fields."""
    f = (lambda v: v.cpu().numpy()) if isinstance(ls.rays, torch.Tensor) else np.asarray
    return dict(rays=f(ls.rays), pdf=f(ls.pdf), light=f(ls.light), dist=f(ls.dist), states=f(ls.rng).view(np.uint64))


def _mismatches(got, want, rows=slice(None)):
    """What differs, bit for bit; in rays and dist a NaN on both sides counts as equal (tor_lights.h: a NaN's sign and payload are
    not defined)."""
    bad = []
    for k in ("rays", "dist"):
        same = LR.same_bits(got[k][rows], want[k][rows])
        if not same.all():
            bad.append(f"{k}: {int((~same).reshape(same.shape[0], -1).any(axis=1).sum())} points")
    if not np.array_equal(got["pdf"][rows].view(np.uint64), want["pdf"][rows].view(np.uint64)):
        bad.append(f"pdf: {int((got['pdf'][rows].view(np.uint64) != want['pdf'][rows].view(np.uint64)).sum())} points")
    if not np.array_equal(got["light"][rows], want["light"][rows]):
        bad.append(f"light: {int((got['light'][rows] != want['light'][rows]).sum())} points")
    if not np.array_equal(got["states"][rows], want["states"][rows]):
        bad.append(f"states: {int((got['states'][rows] != want['states'][rows]).any(axis=1).sum())} points")
    return bad


@pytest.mark.parametrize("name", I.TABLES)
@pytest.mark.parametrize("strategy", list(STRATEGIES))
def test_every_bit_against_the_restatement(tor, oracle, name, strategy):
    g = _case(oracle, name, strategy)
    ctx = _ctx(tor, g)
    pts, st = _cuda(g["pts"]), _cuda(g["st"].view(np.int64), np.int64)
    ls = ctx.sample_lights(pts, st, strategy=STRATEGIES[strategy])
    torch.cuda.synchronize()
    assert ls.mode == NOTES[strategy] and ls.rng.data_ptr() == st.data_ptr()          # the states are updated in place
    got = _np(ls)
    bad = _mismatches(got, g["res"])
    assert not bad, bad
    assert np.array_equal(got["rays"][:, 0:3].view(np.uint64)[got["light"] >= 0], g["pts"][:, 0:3].view(np.uint64)[got["light"] >= 0])
    back = ctx.light_pdf(pts, ls.light, strategy=STRATEGIES[strategy])
    torch.cuda.synchronize()
    assert tor.last_note() == "light pdf: " + NOTES[strategy]
    back = back.cpu().numpy()
    assert np.array_equal(back.view(np.uint64), g["pdf"].view(np.uint64))
    assert np.array_equal(back.view(np.uint64), got["pdf"].view(np.uint64))           # light_pdf(point, sample.light) == sample.pdf
    # an object that is no light has density 0
    other = ctx.light_pdf(pts, _cuda(np.zeros(len(g["pts"])), np.int32), strategy=STRATEGIES[strategy])
    assert (other.cpu().numpy() == 0).all()


@pytest.mark.parametrize("strategy", list(STRATEGIES))
def test_lists_leave_the_other_points_alone(tor, oracle, strategy):
    g = _case(oracle, "three", strategy)
    ctx = _ctx(tor, g)
    n = len(g["pts"])
    listed = [0, 5, 64, 130, n - 4, n - 1]
    index = np.array(listed[:3] + [-3, n + 7] + listed[3:], dtype=np.int32)            # two entries outside [0, n) are skipped
    pts, st = _cuda(g["pts"]), _cuda(g["st"].view(np.int64), np.int64)
    first = ctx.sample_lights(pts, st.clone(), strategy=STRATEGIES[strategy])
    first.rays[:], first.pdf[:], first.light[:], first.dist[:] = 7.0, 7.0, 77, 7.0        # sentinels
    ls = ctx.sample_lights(pts, st, index=_cuda(index, np.int32), strategy=STRATEGIES[strategy], out=first)
    torch.cuda.synchronize()
    assert ls.rays.data_ptr() == first.rays.data_ptr()
    got = _np(ls)
    assert not _mismatches(got, g["res"], listed)
    rest = np.ones(n, dtype=bool)
    rest[listed] = False
    assert (got["rays"][rest] == 7.0).all() and (got["pdf"][rest] == 7.0).all() and (got["light"][rest] == 77).all()
    assert (got["dist"][rest] == 7.0).all() and np.array_equal(got["states"][rest], g["st"][rest])
    back = ctx.light_pdf(pts, _cuda(g["res"]["light"], np.int32), index=index, strategy=STRATEGIES[strategy]).cpu().numpy()
    assert np.array_equal(back[listed].view(np.uint64), g["pdf"][listed].view(np.uint64)) and (back[rest] == 0).all()
    # an empty list is a no-op
    none = ctx.sample_lights(pts, st, index=np.zeros(0, dtype=np.int32), strategy=STRATEGIES[strategy])
    torch.cuda.synchronize()
    assert (none.light.cpu().numpy() == -1).all() and np.array_equal(none.rng.cpu().numpy().view(np.uint64), got["states"])


@pytest.mark.parametrize("name", ("three", "many65"))
@pytest.mark.parametrize("strategy", list(STRATEGIES))
def test_host_twins_and_numpy_operands_equal_the_device_entries(tor, oracle, name, strategy):
    """numpy operands go through tor_light_sample_host / tor_light_pdf_host: the same bits as the device entries on tensors, and
    the caller's arrays are never written."""
    g = _case(oracle, name, strategy)
    ctx = _ctx(tor, g)
    st = g["st"].copy()
    index = np.arange(0, len(g["pts"]), 2, dtype=np.int32)
    for idx in (None, index):
        host = ctx.sample_lights(g["pts"], st, index=idx, strategy=STRATEGIES[strategy])
        assert isinstance(host.rays, np.ndarray) and host.light.dtype == np.int32 and np.array_equal(st, g["st"])
        dev = ctx.sample_lights(_cuda(g["pts"]), _cuda(g["st"].view(np.int64), np.int64), index=idx, strategy=STRATEGIES[strategy])
        torch.cuda.synchronize()
        a, b = _np(host), _np(dev)
        assert not _mismatches(a, b)
        rows = slice(None) if idx is None else idx
        assert not _mismatches(a, g["res"], rows)
        hp = ctx.light_pdf(g["pts"], g["res"]["light"], index=idx, strategy=STRATEGIES[strategy])
        dp = ctx.light_pdf(_cuda(g["pts"]), _cuda(g["res"]["light"], np.int32), index=idx, strategy=STRATEGIES[strategy]).cpu().numpy()
        assert isinstance(hp, np.ndarray) and np.array_equal(hp.view(np.uint64), dp.view(np.uint64))
        assert np.array_equal(hp[rows].view(np.uint64), g["pdf"][rows].view(np.uint64))


def test_the_light_table_lifecycle(tor, oracle):
    g = _case(oracle, "three", LR.BY_SOLID_ANGLE)
    world = tor.Scene.from_records(g["recs"]).list()
    ctx = tor.Context(0)
    with pytest.raises(tor.TorError):                                     # no scene
        ctx.set_lights([0])
    ctx.upload(world)
    pts, st = g["pts"], g["st"]
    with pytest.raises(tor.TorError) as e:                                # no table yet
        ctx.sample_lights(pts, st)
    assert e.value.code == -1 and "light table" in str(e.value)
    ctx.set_lights(g["lights"], g["weights"])
    want = _np(ctx.sample_lights(pts, st))
    assert not _mismatches(want, g["res"])
    for objects, weights in (([5], None), ([-1], None), ([1, 1], None), ([1, 2], [1.0, -1.0]), ([1, 2], [1.0, np.nan]),
                             ([1, 2], [np.inf, 1.0]), ([1, 2], [0.0, 0.0]), ([0, 1, 2, 3, 4, 0], None)):
        with pytest.raises(tor.TorError) as e:
            ctx.set_lights(objects, weights)
        assert e.value.code == -1, (objects, weights)
        assert not _mismatches(_np(ctx.sample_lights(pts, st)), want)     # a refusal changes nothing
    with pytest.raises(ValueError):
        ctx.set_lights([1, 2], [1.0])
    with pytest.raises(tor.TorError):                                     # a strategy that is neither
        ctx.sample_lights(pts, st, strategy=2)
    ctx.upload(world)                                                     # a byte-identical upload keeps the table
    assert not _mismatches(_np(ctx.sample_lights(pts, st)), want)
    recs2 = g["recs"].copy()
    recs2[0, 9] = 99.0
    ctx.upload(tor.Scene.from_records(recs2).list())                      # a replacing upload clears it
    with pytest.raises(tor.TorError):
        ctx.sample_lights(pts, st)
    with pytest.raises(tor.TorError):
        ctx.light_pdf(pts, g["res"]["light"])
    ctx.set_lights(g["lights"], g["weights"])
    assert not _mismatches(_np(ctx.sample_lights(pts, st)), want)         # (object 0 is no light: the same table)
    ctx.set_lights(g["lights"])                                           # weights None: all 1
    ones = _np(ctx.sample_lights(pts, st, strategy="weight"))
    assert not _mismatches(ones, LR.sample(oracle, g["recs"], g["lights"], None, pts, st, None, LR.BY_WEIGHT))
    ctx.set_lights([])                                                    # n_lights == 0 clears the table
    with pytest.raises(tor.TorError):
        ctx.sample_lights(pts, st)


# ---- trace_direct against trace ---------------------------------------------------------------------------------------------------------
SIDE, SPP, DEPTH = 8, 128, 8
_frames = {}


def _frame(tor):
    """The 8 x 8 frame of light_inputs.lamp_scene, SPP samples per pixel: trace(emission=) and trace_direct with and without MIS,
    from the same camera rays and states; per run the per-sample luminances (pixels, SPP).  Computed once."""
    if not _frames:
        recs, emission, lamp = I.lamp_scene()
        scene = tor.Scene.from_records(recs)
        ctx = tor.Context(0)
        ctx.upload(scene.list())
        ctx.set_lights([lamp])
        ctx.set_groups(np.where(np.arange(len(recs)) == lamp, 2, 1).astype(np.uint32))
        cam = tor.camera(look_from=(0.0, 0.0, 4.5), look_at=(0.0, 0.0, 0.0), vertical_field_of_view=70.0, aspect_ratio=1.0,
                         aperture=0.0, focus_distance=1.0, shutter_open=0.0, shutter_close=0.0)
        rays, rng = ctx.camera_rays(cam, SIDE, SIDE, 0, SPP)
        diffuse = tor.diffuse_objects(scene)
        lum = lambda c: c.mean(dim=1).reshape(SIDE * SIDE, SPP).cpu().numpy()
        _frames["trace"] = lum(ctx.trace(rays, rng.clone(), DEPTH, emission=emission)[0])
        _frames["direct"] = lum(ctx.trace_direct(rays, rng.clone(), emission, diffuse, DEPTH)[0])
        _frames["mis"] = lum(ctx.trace_direct(rays, rng.clone(), emission, diffuse, DEPTH, mis=True)[0])
        _frames["masked"] = lum(ctx.trace_direct(rays, rng.clone(), emission, diffuse, DEPTH, lamp_mask=1)[0])
        # all-zero emission, in an OPEN scene (the sky colours the paths): table `three` of the light tests
        recs, lights, weights = I.table("three")
        scene = tor.Scene.from_records(recs)
        ctx.upload(scene.list())
        ctx.set_lights(lights, weights)
        cam = tor.camera(look_from=(0.0, 1.5, 7.0), look_at=(0.0, 0.5, 0.0), vertical_field_of_view=50.0, aspect_ratio=1.0)
        rays, rng = ctx.camera_rays(cam, SIDE, SIDE, 0, 4)
        zero, diffuse = np.zeros((len(recs), 3)), tor.diffuse_objects(scene)
        a = ctx.trace(rays, rng.clone(), DEPTH, emission=zero)
        b = ctx.trace_direct(rays, rng.clone(), zero, diffuse, DEPTH)
        c = ctx.trace_direct(rays, rng.clone(), zero, diffuse, DEPTH, mis=True)
        torch.cuda.synchronize()
        _frames["zero"] = [(x[0].cpu().numpy(), x[1].cpu().numpy()) for x in (a, b, c)]
    return _frames


def _mean_and_error(lum):
    """The frame mean and its standard error from the per-pixel sample variances."""
    return lum.mean(), np.sqrt((lum.var(axis=1, ddof=1) / lum.shape[1]).sum()) / lum.shape[0]


@pytest.mark.parametrize("which", ("direct", "mis", "masked"))
def test_trace_direct_agrees_with_trace_and_is_less_noisy(tor, which):
    """The frame means of trace_direct and trace(emission=) at the same sample count agree within 5 combined standard errors, the
    errors from the per-pixel sample variances of the two runs, and trace_direct's standard error is the smaller one.
    Measured (8 x 8 pixels, 128 samples each, depth 8): trace 0.0852 +- 0.0126; trace_direct 0.0916 +- 0.0017, with MIS
    0.0911 +- 0.0016, with the lamp masked out of the shadow segments 0.0916 +- 0.0017."""
    f = _frame(tor)
    m0, e0 = _mean_and_error(f["trace"])
    m1, e1 = _mean_and_error(f[which])
    print(f"trace: {m0:.5f} +- {e0:.5f}; trace_direct ({which}): {m1:.5f} +- {e1:.5f}")
    assert m1 > 0 and e1 > 0 and abs(m1 - m0) <= 5 * np.sqrt(e0 * e0 + e1 * e1)
    assert e1 < e0


def test_the_trace_direct_variants_agree_with_each_other(tor):
    """With and without MIS, with the lamp masked out of the shadow segments or the segments stopping short of it: the same
    integral, at trace_direct's own (small) standard errors."""
    f = _frame(tor)
    runs = {k: _mean_and_error(f[k]) for k in ("direct", "mis", "masked")}
    for a in runs:
        for b in runs:
            assert abs(runs[a][0] - runs[b][0]) <= 5 * np.sqrt(runs[a][1] ** 2 + runs[b][1] ** 2), (a, b, runs)


def test_all_zero_emission_gives_trace_colours_bit_for_bit(tor):
    (c0, s0), (c1, s1), (c2, s2) = _frame(tor)["zero"]
    assert (c0 > 0).any() and len(np.unique(c0)) > 16                     # the sky coloured the paths: not a frame of zeros
    assert np.array_equal(c0.view(np.uint64), c1.view(np.uint64)) and np.array_equal(c0.view(np.uint64), c2.view(np.uint64))
    assert np.array_equal(s0, s1) and np.array_equal(s0, s2)              # the light draws come from a second stream
