"""Light-tracing queries on the MI355X (tor_camera_connect_device / _host, tor_light_emit_device / _host): for every camera, frame
and point set of tests/camera_inputs.py the rays, pixels, factors, lens points and generator states, and for every light table
and time range the emitted rays, normals, lights, densities and states, are those of the numpy restatement of
include/tor_camera.h (tests/camera_restatement.py, which tests/test_camera_query.py shows to be sound), bit for bit; lists, the
blocking twins, numpy operands, out= and the lifecycle; Context.trace_light against Context.trace_direct on a frame of diffuse
surfaces, Film.add_light_pass, and the second stream of the connection draws."""
import numpy as np
import pytest
import torch

import camera_inputs as I
import camera_restatement as CR
import light_inputs as LI

pytestmark = pytest.mark.gpu
_cases = {}


def _connect_case(oracle, name, frame):
    """Camera, points, states and the restatement's connection: computed once, never changed."""
    key = ("connect", name, frame)
    if key not in _cases:
        cam = I.camera(oracle, name)
        pts = I.points(cam, *frame)
        st = I.states(len(pts))
        _cases[key] = dict(cam=cam, pts=pts, st=st, res=CR.connect(oracle, cam, frame[0], frame[1], pts, st))
    return _cases[key]


def _emit_case(oracle, name, tr):
    key = ("emit", name, tr)
    if key not in _cases:
        recs, lights, weights = I.table(name, oracle)
        st = I.states(I.N_POINTS)
        _cases[key] = dict(recs=recs, lights=lights, weights=weights, st=st, res=CR.emit(oracle, recs, lights, weights, st, tr[0], tr[1]))
    return _cases[key]


def _ctx(tor, g):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(g["recs"], dtype=np.float64).reshape(-1, 16)).list())
    ctx.set_lights(g["lights"], g["weights"])
    return ctx


def _cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _states(st):
    return _cuda(st.view(np.int64), np.int64)


def _np(r, fields):
    f = (lambda v: v.cpu().numpy()) if isinstance(r.rays, torch.Tensor) else np.asarray
    out = {k: f(getattr(r, k)) for k in fields}
    out["states"] = f(r.rng).view(np.uint64)
    return out


CONNECT, EMIT = ("rays", "pixel", "factor", "lens"), ("rays", "normal", "light", "pdf")


def _mismatches(got, want, fields, rows=slice(None)):
    """What differs, bit for bit; in float fields a NaN on both sides counts as equal (a NaN's sign and payload are not defined)."""
    bad = []
    for k in fields + ("states",):
        a, b = got[k][rows], want[k][rows]
        same = CR.same_bits(a, b) if a.dtype == np.float64 else (a == b)
        if not same.all():
            bad.append(f"{k}: {int((~same).reshape(same.shape[0], -1).any(axis=1).sum())} entries")
    return bad


@pytest.mark.parametrize("name", list(I.CAMERAS))
@pytest.mark.parametrize("frame", I.FRAMES)
def test_connect_every_bit_against_the_restatement(tor, oracle, name, frame):
    g = _connect_case(oracle, name, frame)
    ctx = tor.Context(0)                                                   # no scene: the query reads none
    cam = I.camera_struct(tor, g["cam"])
    pts, st = _cuda(g["pts"]), _states(g["st"])
    con = ctx.connect_camera(cam, frame[0], frame[1], pts, st)
    torch.cuda.synchronize()
    assert con.mode == ("pinhole" if g["cam"][21] == 0 else "thin lens") and con.rng.data_ptr() == st.data_ptr()
    bad = _mismatches(_np(con, CONNECT), g["res"], CONNECT)
    assert not bad, bad
    assert (g["res"]["pixel"] >= 0).sum() > 30 and (g["res"]["pixel"] < 0).sum() > 30


@pytest.mark.parametrize("name", I.TABLES)
@pytest.mark.parametrize("tr", I.TIME_RANGES)
def test_emit_every_bit_against_the_restatement(tor, oracle, name, tr):
    g = _emit_case(oracle, name, tr)
    ctx = _ctx(tor, g)
    st = _states(g["st"])
    em = ctx.emit_lights(st, tr)
    torch.cuda.synchronize()
    assert em.mode == "by weight" and em.rng.data_ptr() == st.data_ptr()
    got = _np(em, EMIT)
    bad = _mismatches(got, g["res"], EMIT)
    assert not bad, bad
    assert np.array_equal(em.pdf_area.cpu().numpy(), got["pdf"][:, 0]) and np.array_equal(em.pdf_dir.cpu().numpy(), got["pdf"][:, 1])


def test_lists_leave_the_other_entries_alone(tor, oracle):
    frame = (5, 7)
    g = _connect_case(oracle, "lens", frame)
    e = _emit_case(oracle, "three", I.TIME_RANGES[1])
    ctx = _ctx(tor, e)
    cam = I.camera_struct(tor, g["cam"])
    n = len(g["pts"])
    listed = [0, 5, 64, 130, n - 4, n - 1]
    index = _cuda(np.array(listed[:3] + [-3, n + 7] + listed[3:]), np.int32)           # two entries outside [0, n) are skipped
    rest = np.ones(n, dtype=bool)
    rest[listed] = False
    pts = _cuda(g["pts"])
    first = ctx.connect_camera(cam, 5, 7, pts, _states(g["st"]))
    first.rays[:], first.pixel[:], first.factor[:], first.lens[:] = 7.0, 77, 7.0, 7.0    # sentinels
    st = _states(g["st"])
    con = ctx.connect_camera(cam, 5, 7, pts, st, index=index, out=first)
    torch.cuda.synchronize()
    assert con.rays.data_ptr() == first.rays.data_ptr() and con.pixel.data_ptr() == first.pixel.data_ptr()     # out= reuses its buffers
    got = _np(con, CONNECT)
    assert not _mismatches(got, g["res"], CONNECT, listed)
    assert (got["rays"][rest] == 7.0).all() and (got["pixel"][rest] == 77).all() and (got["factor"][rest] == 7.0).all()
    assert (got["lens"][rest] == 7.0).all() and np.array_equal(got["states"][rest], g["st"][rest])
    efirst = ctx.emit_lights(_states(e["st"]), I.TIME_RANGES[1])
    efirst.rays[:], efirst.normal[:], efirst.light[:], efirst.pdf[:] = 7.0, 7.0, 77, 7.0
    st = _states(e["st"])
    em = ctx.emit_lights(st, I.TIME_RANGES[1], index=index, out=efirst)
    torch.cuda.synchronize()
    assert em.rays.data_ptr() == efirst.rays.data_ptr() and em.pdf.data_ptr() == efirst.pdf.data_ptr()
    got = _np(em, EMIT)
    assert not _mismatches(got, e["res"], EMIT, listed)
    assert (got["rays"][rest] == 7.0).all() and (got["normal"][rest] == 7.0).all() and (got["light"][rest] == 77).all()
    assert (got["pdf"][rest] == 7.0).all() and np.array_equal(got["states"][rest], e["st"][rest])
    none = ctx.emit_lights(st, I.TIME_RANGES[1], index=np.zeros(0, dtype=np.int32))     # an empty list is a no-op
    torch.cuda.synchronize()
    assert (none.light.cpu().numpy() == -1).all() and np.array_equal(none.rng.cpu().numpy().view(np.uint64), got["states"])


def test_host_twins_and_numpy_operands_equal_the_device_entries(tor, oracle):
    """numpy operands go through the _host entries: the same bits as the device entries on tensors, and the caller's arrays are
    never written."""
    frame = (48, 64)
    g = _connect_case(oracle, "tilted", frame)
    e = _emit_case(oracle, "many65", I.TIME_RANGES[1])
    ctx = _ctx(tor, e)
    cam = I.camera_struct(tor, g["cam"])
    index = np.arange(0, len(g["pts"]), 2, dtype=np.int32)
    for idx in (None, index):
        rows = slice(None) if idx is None else idx
        st = g["st"].copy()
        host = ctx.connect_camera(cam, frame[0], frame[1], g["pts"], st, index=idx)
        assert isinstance(host.rays, np.ndarray) and host.pixel.dtype == np.int32 and np.array_equal(st, g["st"])
        dev = ctx.connect_camera(cam, frame[0], frame[1], _cuda(g["pts"]), _states(g["st"]), index=idx)
        torch.cuda.synchronize()
        a, b = _np(host, CONNECT), _np(dev, CONNECT)
        assert not _mismatches(a, b, CONNECT) and not _mismatches(a, g["res"], CONNECT, rows)
        st = e["st"].copy()
        host = ctx.emit_lights(st, I.TIME_RANGES[1], index=idx)
        assert isinstance(host.rays, np.ndarray) and host.light.dtype == np.int32 and np.array_equal(st, e["st"])
        dev = ctx.emit_lights(_states(e["st"]), I.TIME_RANGES[1], index=idx)
        torch.cuda.synchronize()
        a, b = _np(host, EMIT), _np(dev, EMIT)
        assert not _mismatches(a, b, EMIT) and not _mismatches(a, e["res"], EMIT, rows)


def test_the_lifecycle(tor, oracle):
    e = _emit_case(oracle, "three", I.TIME_RANGES[0])
    g = _connect_case(oracle, "pinhole", (5, 7))
    world = tor.Scene.from_records(e["recs"]).list()
    ctx = tor.Context(0)
    con = ctx.connect_camera(I.camera_struct(tor, g["cam"]), 5, 7, g["pts"], g["st"])   # a context without a scene
    assert not _mismatches(_np(con, CONNECT), g["res"], CONNECT)
    with pytest.raises(tor.TorError) as err:                              # no scene
        ctx.emit_lights(e["st"])
    assert err.value.code == -1
    ctx.upload(world)
    with pytest.raises(tor.TorError) as err:                              # no table yet
        ctx.emit_lights(e["st"])
    assert err.value.code == -1 and "light table" in str(err.value)
    ctx.set_lights(e["lights"], e["weights"])
    assert not _mismatches(_np(ctx.emit_lights(e["st"]), EMIT), e["res"], EMIT)
    with pytest.raises(tor.TorError):                                     # an inverted time range
        ctx.emit_lights(e["st"], (1.0, 0.5))
    ctx.set_lights([4, 2], [1.0, 3.0])                                    # it follows a replaced table
    want = CR.emit(oracle, e["recs"], [4, 2], [1.0, 3.0], e["st"])
    assert not _mismatches(_np(ctx.emit_lights(e["st"]), EMIT), want, EMIT)
    ctx.set_lights([])
    with pytest.raises(tor.TorError):
        ctx.emit_lights(e["st"])
    bad = I.camera_struct(tor, g["cam"])
    bad.lens_radius = -1.0
    with pytest.raises(tor.TorError):
        ctx.connect_camera(bad, 5, 7, g["pts"], g["st"])
    with pytest.raises(tor.TorError):
        ctx.connect_camera(I.camera_struct(tor, g["cam"]), 1, 7, g["pts"], g["st"])


# ---- trace_light against trace_direct ---------------------------------------------------------------------------------------------------
SIDE, SPP, DEPTH, BATCHES = 8, 128, 8, 16
_frames = {}


class _Sum:
    """A splat that keeps the sum of the luminances it is offered and whether any was non-zero."""

    def __init__(self):
        self.total, self.nonzero, self.bad = 0.0, False, False

    def __call__(self, pixels, colors, index):
        at = index.long()
        c, p = colors[at], pixels[at]
        self.bad = self.bad or bool(((p < -1) | (p >= SIDE * SIDE)).any()) or bool((c[p < 0] != 0).any())
        self.nonzero = self.nonzero or bool((c != 0).any())
        self.total += float(c[p >= 0].mean(dim=1).sum())


def _frame(tor):
    """The 8 x 8 frame of camera_inputs.diffuse_scene: trace_direct's per-sample luminances at SPP samples per pixel, and the
    frame means of BATCHES batches of 64 * SPP / BATCHES light paths each.  Computed once."""
    if not _frames:
        recs, emission, lamp = I.diffuse_scene()
        scene = tor.Scene.from_records(recs)
        ctx = tor.Context(0)
        ctx.upload(scene.list())
        ctx.set_lights([lamp])
        cam = I.frame_camera(tor)
        rays, rng = ctx.camera_rays(cam, SIDE, SIDE, 0, SPP)
        diffuse = tor.diffuse_objects(scene)
        _frames["first_hits"] = ctx.hit(rays).object.cpu().numpy()
        _frames["kinds"] = recs[:, 10]
        _frames["direct"] = ctx.trace_direct(rays, rng.clone(), emission, diffuse, DEPTH)[0].mean(dim=1).reshape(SIDE * SIDE, SPP).cpu().numpy()
        per = SIDE * SIDE * SPP // BATCHES
        means = []
        for b in range(BATCHES):
            st = torch.from_numpy(tor.rng_seed2(np.full(per, b, dtype=np.uint64), np.arange(per, dtype=np.uint64)).view(np.int64)).cuda()
            acc = _Sum()
            offered, _, _ = ctx.trace_light(cam, SIDE, SIDE, st, emission, diffuse, DEPTH, splat=acc)
            assert not acc.bad and offered >= per
            means.append(acc.total / per)
        _frames["light"] = np.array(means)
        _frames["ctx"], _frames["cam"], _frames["scene"] = ctx, cam, (emission, diffuse)
    return _frames


def test_trace_light_agrees_with_trace_direct(tor):
    """The camera sees diffuse surfaces only (asserted on the first hits), so both estimators integrate the same frame: the
    frame means agree within 5 combined standard errors, trace_light's from its 16 batches, trace_direct's from its per-pixel
    sample variances.  The raw sums are compared, no film and no clamp.  (At depth 8 trace_light follows paths of up to 8
    surface vertices and trace_direct of up to 7; with albedos <= 0.7 the eighth vertex carries under 1 % of the mean, well
    inside the errors.)"""
    f = _frame(tor)
    first = f["first_hits"]
    assert (first >= 0).all() and (f["kinds"][first] == 0).all()          # no first hit is Metal or Dielectric, none misses
    lum = f["direct"]
    m0, e0 = lum.mean(), np.sqrt((lum.var(axis=1, ddof=1) / lum.shape[1]).sum()) / lum.shape[0]
    m1, e1 = f["light"].mean(), f["light"].std(ddof=1) / np.sqrt(BATCHES)
    print(f"trace_direct: {m0:.5f} +- {e0:.5f}; trace_light: {m1:.5f} +- {e1:.5f}")
    assert m1 > 0 and e1 > 0 and e0 > 0 and abs(m1 - m0) <= 5 * np.sqrt(e0 * e0 + e1 * e1)


def test_film_add_light_pass(tor):
    f = _frame(tor)
    ctx, cam = f["ctx"], f["cam"]
    emission, diffuse = f["scene"]
    film = tor.Film(ctx, SIDE, SIDE, max_value=128.0)
    film.add_light_pass(cam, 2, emission, diffuse, max_depth=DEPTH)
    film.add_light_pass(cam, 3, emission, diffuse, max_depth=DEPTH, chunk_paths=100)
    assert film.samples == 5 and film.rejected() == 0
    img = film.image().cpu().numpy()
    assert np.isfinite(img).all() and (img > 0).any() and img.shape == (SIDE, SIDE, 3)
    mean = float(film.sums.mean(dim=2).mean().item()) / film.samples
    print(f"film mean {mean:.5f}; trace_light batches {f['light'].mean():.5f}")
    assert abs(mean - f["light"].mean()) <= 0.5 * f["light"].mean()      # the same estimator, five samples per pixel
    state = film.state()
    again = tor.Film.from_state(ctx, state)
    assert again.samples == 5 and np.array_equal(again.sums.cpu().numpy(), state["sums"])
    assert np.array_equal(again.image().cpu().numpy(), img)


def test_all_zero_emission_splats_nothing_and_leaves_the_bounce_states_alone(tor):
    """With an all-zero emission no splat is non-zero, and the returned states are those of trace() over the emitted rays from
    the states the emission left: the connection draws come from a second stream."""
    recs, lights, weights = LI.table("three")
    scene = tor.Scene.from_records(recs)
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    ctx.set_lights(lights, weights)
    cam = tor.camera(look_from=(0.0, 1.5, 7.0), look_at=(0.0, 0.5, 0.0), vertical_field_of_view=50.0, aspect_ratio=1.0,
                     shutter_open=0.0, shutter_close=1.0)
    st = I.states(512)
    zero, diffuse = np.zeros((len(recs), 3)), tor.diffuse_objects(scene)
    em = ctx.emit_lights(_states(st), (0.0, 1.0))
    want = ctx.trace(em.rays, em.rng.clone(), DEPTH, time_range=(0.0, 1.0))[1]
    acc = _Sum()
    offered, got, mode = ctx.trace_light(cam, SIDE, SIDE, _states(st), zero, diffuse, DEPTH, splat=acc)
    torch.cuda.synchronize()
    assert offered > 512 and not acc.nonzero and not acc.bad
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    assert not np.array_equal(got.cpu().numpy().view(np.uint64), _np(em, ())["states"])                # the paths did bounce
    host = ctx.trace_light(cam, SIDE, SIDE, st, zero, diffuse, DEPTH)                                   # numpy states: through the device
    assert isinstance(host[1], np.ndarray) and np.array_equal(host[1], got.cpu().numpy().view(np.uint64)) and host[0] == offered
