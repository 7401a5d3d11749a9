"""Any-hit (occlusion) queries on the MI355X (tor_occluded_device / tor_occluded_host): in every mode the bit of every ray is
`world.hit(...)` of the numpy restatement (tests/hit_restatement.py, anchored to the CPU oracle by tests/test_hit_query.py) -- on
random_scene, an animation frame (two-level culling layout), a scene of several time groups, shadow segments, segments that end on a
surface ulp by ulp, rays from inside spheres, grazing rays, coincident duplicates, degenerate rays, empty and small scenes, waves
with live and dead lanes, and lists -- it equals `hit().object >= 0` over a million rays, and a query leaves the render path alone.
The kernel leaves its loops early; what that may break is a ray dropped because its wave's other rays were settled."""
import numpy as np
import pytest
import torch

import hit_restatement as R

pytestmark = pytest.mark.gpu
MODES = ("auto", "brute", "blocks")


def _ctx(tor, recs):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    return ctx


def _cuda(a, dtype=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _query(ctx, rays, t_range=None, time_range=None, mode="auto", index=None, out=None):
    res = ctx.occluded(_cuda(rays), _cuda(t_range), index, time_range, mode, out)
    torch.cuda.synchronize()
    raw = res.raw.cpu().numpy()
    assert raw.dtype == np.int32 and raw.shape == (len(rays),)
    if index is None and out is None:
        assert np.array_equal(res.occluded.cpu().numpy(), raw != 0)   # the bool view
    return raw, res.mode


def _want(recs, rays, t_range=None):
    return (R.fields(R.world_hit(recs, rays, t_range))["object"] >= 0).astype(np.int32)


def _check(ctx, recs, rays, t_range=None, time_range=None, modes=MODES, want=None):
    """Every mode against the restatement, bit for bit; returns ({mode: what ran}, want)."""
    want = _want(recs, rays, t_range) if want is None else want
    ran = {}
    for m in modes:
        got, ran[m] = _query(ctx, rays, t_range, time_range, m)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"mode {m} (ran: {ran[m]}): {bad.size} rays differ from the restatement, first {bad[:8]}: " \
                              f"got {got[bad[:8]]}, want {want[bad[:8]]}"
    return ran, want


@pytest.fixture(scope="module")
def rscene(tor):
    return tor.random_scene(0xFACADE).to_records()


@pytest.fixture(scope="module")
def anim_frame(tor):
    cam, scene, _ = next(iter(tor.Animation(108, 192).scenes(skip=6)))
    return np.frombuffer(bytes(cam), dtype=np.float64).copy(), scene.to_records()


def _scene_box(recs):
    """incoherent_rays' box: the 2nd / 98th percentile of centres -+ radius."""
    r = np.abs(recs[:, 9:10])
    lo = np.minimum(recs[:, 1:4], recs[:, 4:7]) - r
    hi = np.maximum(recs[:, 1:4], recs[:, 4:7]) + r
    return np.percentile(lo, 2, axis=0), np.percentile(hi, 98, axis=0)


def test_random_scene_camera_and_incoherent_rays(tor, oracle, rscene):
    ctx = _ctx(tor, rscene)
    cam_rays = R.camera_rays(oracle, oracle.camera(), 108, 192)
    ran, want = _check(ctx, rscene, cam_rays)
    assert ran["auto"] == "blocks" and ran["blocks"] == "blocks" and ran["brute"] == "brute force"
    assert 0.2 < want.mean() < 0.95
    _check(ctx, rscene, R.incoherent_rays(rscene, 32768, 1))


def test_animation_frame_two_level_layout(tor, oracle, anim_frame):
    cam, recs = anim_frame
    assert len(recs) == 1601
    lay = tor.debug_accel_layout(tor.Scene.from_records(recs).list(), min(0.0, cam[22]), max(0.0, cam[23]))
    assert lay is not None and lay[3], "the animation frame should have a two-level culling layout"
    ctx = _ctx(tor, recs)
    ran, _ = _check(ctx, recs, R.camera_rays(oracle, cam, 54, 96))
    assert ran["auto"] == "blocks"
    _check(ctx, recs, R.incoherent_rays(recs, 16384, 2))


def test_time_groups_and_rays_outside_the_time_range(tor):
    recs = R.group_scene(5)
    ctx = _ctx(tor, recs)
    rays = R.incoherent_rays(recs, 24576, 3, (-1.0, 2.5))
    want = _want(recs, rays)
    _check(ctx, recs, rays, want=want)                                   # the rays' own range
    ran, _ = _check(ctx, recs, rays, time_range=(-0.25, 1.0), want=want)   # most rays outside: they walk
    assert ran["blocks"] == "blocks"
    _check(ctx, recs, rays, time_range=(0.5, 0.5), want=want)


def test_shadow_segments(tor, rscene):
    """Segments between random points of the scene's box, range (0.001, 1.0): what a next-event estimator casts.  Then the same
    rays with cut and shifted ranges, negative, -inf and NaN t_min among them (those rays walk)."""
    rng = np.random.default_rng(40)
    lo, hi = _scene_box(rscene)
    n = 32768
    p, q = rng.uniform(lo, hi, (n, 3)), rng.uniform(lo, hi, (n, 3))
    rays, tr = tor.Context.shadow_segments(p, q, time=rng.uniform(0, 1, n))
    want = _want(rscene, rays, tr)                       # on the CPU, before anything runs on the GPU
    assert 0.05 <= want.mean() <= 0.95, f"occluded share {want.mean():.3f}: each outcome must be at least 5 % of the batch"
    ctx = _ctx(tor, rscene)
    ran, _ = _check(ctx, rscene, rays, tr, want=want)
    assert ran["auto"] == "blocks"
    t_min = rng.choice([0.0, 0.001, 0.5, 3.0, 20.0, -2.0, -np.inf, np.nan], n)   # as test_cut_and_shifted_t_ranges draws them,
    with np.errstate(invalid="ignore"):                                          # in units of the segment's length
        t_max = t_min + rng.choice([0.25, 1.0, 4.0, np.inf], n)
    t_max = np.where(np.isnan(t_max), 5.0, t_max)
    tr2 = np.stack([t_min, t_max], axis=1)
    want2 = _want(rscene, rays, tr2)
    assert 0.05 <= want2.mean() <= 0.95
    _check(ctx, rscene, rays, tr2, want=want2)
    # visible() is ~occluded of the same segments
    vis = ctx.visible(_cuda(p), _cuda(q), time=_cuda(rays[:, 6]))
    torch.cuda.synchronize()
    assert np.array_equal(vis.cpu().numpy(), want == 0)


@pytest.mark.parametrize("which", ["anim", "random"])
def test_segment_ends_on_a_surface(tor, rscene, anim_frame, which):
    """Origin outside sphere k, direction towards its centre, t_max at the restatement's root stepped -2 .. +2 ulps: `sol < t_max` is
    strict, so the bit flips exactly between step 0 and step +1.  A slab test clipped at t_max must still enter the sphere's box
    (and, in the animation frame's two-level layout, its super box).  The first 200 small static spheres of the animation frame;
    random_scene has 86 of them (its Lambertian spheres move), all taken."""
    rng = np.random.default_rng(41)
    rscene = anim_frame[1] if which == "anim" else rscene
    count = 200 if which == "anim" else 86
    small = [k for k, rec in enumerate(rscene) if rec[0] == 0 and abs(rec[9]) <= 0.5][:200]
    assert len(small) == count
    rays, tr, step_of = [], [], []
    for k in small:
        c, r = rscene[k, 1:4], abs(rscene[k, 9])
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        o = c + (r + rng.uniform(0.02, 0.3)) * u
        ray = np.array([[*o, *(c - o), 0.0]])
        alone = R.fields(R.world_hit(rscene[k:k + 1], ray))
        assert alone["object"][0] == 0
        t = alone["t"][0]
        for steps in (-2, -1, 0, 1, 2):
            ts = t
            for _ in range(abs(steps)):
                ts = np.nextafter(ts, np.inf if steps > 0 else -np.inf)
            rays.append(ray[0])
            tr.append([0.001, ts])
            step_of.append(steps)
    rays, tr, step_of = np.asarray(rays), np.asarray(tr), np.asarray(step_of)
    want = _want(rscene, rays, tr)
    assert (want[step_of > 0] == 1).all()
    clear = want.reshape(count, 5)[:, :3].sum(axis=1) == 0               # nothing else in the way: the bit flips at the root
    assert clear.sum() > 0.75 * count
    _check(_ctx(tor, rscene), rscene, rays, tr, want=want)


def test_rays_from_inside_spheres(tor, rscene):
    rng = np.random.default_rng(6)
    ctx = _ctx(tor, rscene)
    k = rng.integers(0, len(rscene), 8192)
    o = rscene[k, 1:4] + rng.uniform(-0.05, 0.05, (8192, 3)) * np.abs(rscene[k, 9:10])
    d = rng.normal(size=(8192, 3))
    rays = np.concatenate([o, d, rng.uniform(0, 1, (8192, 1))], axis=1)
    _, want = _check(ctx, rscene, rays)
    assert want.sum() > 4000
    # the way out of the sphere cut off: second roots beyond t_max
    tr = np.stack([np.full(8192, 0.001), rng.choice([0.01, 0.1, 1.0], 8192)], axis=1)
    _, want = _check(ctx, rscene, rays, tr)
    assert 0.05 < want.mean() < 0.95


def test_grazing_rays_and_coincident_duplicates(tor, rscene):
    """Rays that pass every sphere at its extreme coordinate along x, y and z (+- 2 ulps): the discriminant's sign is decided by
    rounding, and a box without a margin loses such hits.  Duplicates of the first 60 objects are appended."""
    recs = np.concatenate([rscene, rscene[:60]])
    ctx = _ctx(tor, recs)
    rng = np.random.default_rng(8)
    rays = []
    for rec in rscene:
        if rec[0] != 0 or abs(rec[9]) > 2.0:
            continue
        c, r = rec[1:4], abs(rec[9])
        for axis in range(3):
            others = [a for a in range(3) if a != axis]
            for sign in (-1.0, 1.0):
                x = c[axis] + sign * r
                for steps in (-2, -1, 0, 1, 2):
                    xs = x
                    for _ in range(abs(steps)):
                        xs = np.nextafter(xs, np.inf if steps > 0 else -np.inf)
                    u = rng.normal(size=2)
                    u /= np.linalg.norm(u)
                    o, d = np.zeros(3), np.zeros(3)
                    o[axis] = xs
                    o[others] = c[others] - 10.0 * u
                    d[others] = u
                    rays.append([*o, *d, 0.0])
    rays = np.asarray(rays)
    _, want = _check(ctx, recs, rays)
    assert want.sum() > 1000                      # (the hit test's condition on the same rays)
    assert 0.05 <= want.mean() <= 0.95            # ... and both outcomes are in the batch
    k = np.arange(60)
    o = np.tile([13.0, 2.0, 3.0], (60, 1))
    tie_rays = np.concatenate([o, rscene[k, 1:4] - o, np.zeros((60, 1))], axis=1)
    _, want = _check(ctx, recs, tie_rays)
    assert (want == 1).all()


@pytest.mark.parametrize("which", ["random", "groups"])
def test_far_origin_grazing_rays(tor, rscene, which):
    """From 1e4 .. 1e6 units away the reference accepts rays that pass several 1e-6 above a sphere, farther out than a culling
    box's margin: such origins walk, and the walk must not lose them."""
    recs = rscene if which == "random" else R.group_scene(19)
    ctx = _ctx(tor, recs)
    rays = R.far_grazing_rays(recs, 20)
    ran, want = _check(ctx, recs, rays, time_range=(0.0, 1.0))
    assert ran["auto"] == "blocks"
    assert want.sum() > 20 and (want == 0).sum() > 20


def test_degenerate_rays(tor, rscene):
    rng = np.random.default_rng(9)
    recs = np.concatenate([rscene, R.group_scene(10, 200)])   # movers too: NaN times must miss them and only them
    ctx = _ctx(tor, recs)
    rays = R.incoherent_rays(recs, 8192, 10, (0.0, 1.0))
    rays[0::7, 3:6] = 0.0                                   # zero directions
    rays[1::7, 6] = np.nan                                  # NaN times
    rays[2::7, 6] = rng.choice([-5.0, 7.0, np.inf, -np.inf], len(rays[2::7]))   # outside any range the bounds were built for
    rays[3::7, 3:6] *= 1e-150                               # tiny directions
    rays[4::7, 3] = 0.0                                     # axis-parallel
    want = _want(recs, rays)
    _check(ctx, recs, rays, want=want)
    _check(ctx, recs, rays, time_range=(0.0, 1.0), want=want)


def test_empty_scene_and_small_scenes(tor):
    rays = R.incoherent_rays(R.group_scene(11, 40), 1000, 12)
    ctx = _ctx(tor, np.zeros((0, 16)))
    for m in MODES:
        got, ran = _query(ctx, rays, mode=m)
        assert (got == 0).all()
        assert ran.startswith("brute force")
    recs = R.group_scene(11, 40)   # below the culling layout's minimum: every mode runs the brute force
    ran, want = _check(_ctx(tor, recs), recs, rays)
    assert all(ran[m].startswith("brute force") for m in MODES) and ran["blocks"].startswith("brute force (")
    assert 0 < want.sum() < len(want)


@pytest.mark.parametrize("n", [0, 1, 63, 65, 257])
def test_batch_sizes(tor, rscene, n):
    """Waves that hold live and dead lanes: the ballot that ends a loop must count the live ones only, and all of them."""
    ctx = _ctx(tor, rscene)
    rays = R.incoherent_rays(rscene, max(n, 1), 13)[:n]
    want = _want(rscene, rays)
    for m in MODES:
        got, _ = _query(ctx, rays, mode=m)
        assert got.shape == (n,) and np.array_equal(got, want)
    if n == 0:   # numpy in, too
        res = ctx.occluded(np.zeros((0, 7)))
        assert res.raw.shape == (0,) and res.occluded.shape == (0,)


def test_one_wave_where_all_rays_but_one_are_settled_at_once(tor, rscene):
    """64 rays, one wave: 63 are settled by the ground sphere (the first always-object of the culling layout) and one can be answered
    by the last spatial object alone.  A wave that leaves because most of its lanes are done would drop that ray."""
    lay = tor.debug_accel_layout(tor.Scene.from_records(rscene).list(), 0.0, 1.0)
    assert lay is not None
    slots = lay[0].reshape(-1)
    spatial = slots[slots >= 0]
    assert 0 not in spatial, "the ground sphere should be an always-object"
    last = int(spatial[-1])
    c, r = rscene[last, 1:4], abs(rscene[last, 9])
    assert r <= 0.5 and (rscene[last, 0] == 0 or rscene[last, 7] == 0.0)   # (a mover sits at its first centre at time 0)
    rng = np.random.default_rng(42)
    lo, hi = _scene_box(rscene)
    down = np.concatenate([rng.uniform([lo[0], 3.0, lo[2]], [hi[0], 4.0, hi[2]], (63, 3)),
                           np.tile([0.0, -1.0, 0.0], (63, 1)) + rng.uniform(-0.1, 0.1, (63, 3)), np.zeros((63, 1))], axis=1)
    o = c + np.array([0.0, r + 0.3, 0.0])
    lone = np.array([[*o, *(c - o), 0.0]])                               # from above the sphere to its centre ...
    for pos in (0, 37, 63):
        rays = np.insert(down, pos, lone[0], axis=0)
        tr = np.tile([0.001, np.inf], (64, 1))
        tr[pos] = [0.001, 1.0]                                           # ... and no farther: the ground below is out of range
        assert (_want(rscene[0:1], np.delete(rays, pos, axis=0)) == 1).all()        # the ground settles the 63
        assert _want(rscene[last:last + 1], lone, tr[pos:pos + 1])[0] == 1          # the last spatial object answers the lone ray
        assert _want(np.delete(rscene, last, axis=0), lone, tr[pos:pos + 1])[0] == 0   # ... and nothing else does
        ran, want = _check(_ctx(tor, rscene), rscene, rays, tr)
        assert want.all() and ran["blocks"] == "blocks"


def test_lists(tor, rscene):
    ctx = _ctx(tor, rscene)
    n = 3001
    rays = R.incoherent_rays(rscene, n, 43)
    want = _want(rscene, rays)
    assert 0 < want.sum() < n
    dr = _cuda(rays)
    for m in MODES:
        # a strided list
        out = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        idx = np.arange(1, n, 3, dtype=np.int32)
        res = ctx.occluded(dr, None, torch.from_numpy(idx).cuda(), None, m, out)
        torch.cuda.synchronize()
        assert res.raw is out
        got = out.cpu().numpy()
        listed = np.zeros(n, dtype=bool)
        listed[idx] = True
        assert np.array_equal(got[listed], want[listed]) and (got[~listed] == 7).all(), m
        # entries outside [0, n) are skipped; the list is unordered
        out = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        idx = np.array([n, 5, -1, 2999, 64, n + 100, 0, -(1 << 31), 3000, (1 << 31) - 1], dtype=np.int32)
        res = ctx.occluded(dr, None, idx, None, m, tor.OccludedResult(out, None, ""))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        listed[:] = False
        listed[[5, 2999, 64, 0, 3000]] = True
        assert np.array_equal(got[listed], want[listed]) and (got[~listed] == 7).all(), m
        # an empty list is a no-op
        res = ctx.occluded(dr, None, np.zeros(0, dtype=np.int32), None, m, out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), got) and res.mode == "nothing to do"


@pytest.mark.parametrize("which", ["random", "anim", "groups"])
def test_occluded_is_the_closest_hit_s_object_bit_over_a_million_rays(tor, rscene, anim_frame, which):
    recs = {"random": rscene, "anim": anim_frame[1], "groups": R.group_scene(15)}[which]
    ctx = _ctx(tor, recs)
    rt = torch.from_numpy(R.incoherent_rays(recs, 1 << 20, 16, (0.0, 1.0))).cuda()
    for m in ("brute", "blocks"):
        hit = ctx.hit(rt, None, (0.0, 1.0), m)
        occ = ctx.occluded(rt, None, None, (0.0, 1.0), m)
        torch.cuda.synchronize()
        assert occ.mode == hit.mode == {"brute": "brute force", "blocks": "blocks"}[m]
        want = hit.object >= 0
        assert torch.equal(occ.raw, want.to(torch.int32)), f"{which}, {m}"
        assert torch.equal(occ.occluded, want)
        assert int(want.sum()) > 100000 and int((~want).sum()) > 10000


def test_host_entry_equals_device_entry(tor, rscene):
    ctx = _ctx(tor, rscene)
    rng = np.random.default_rng(17)
    rays = R.incoherent_rays(rscene, 50000, 17)
    tr = np.stack([rng.choice([0.001, 1.0], len(rays)), rng.choice([np.inf, 6.0, 1.5], len(rays))], axis=1)
    idx = np.arange(0, 50000, 2, dtype=np.int32)
    for m in MODES:
        host = ctx.occluded(rays, tr, mode=m)               # numpy in: tor_occluded_host
        assert isinstance(host.raw, np.ndarray) and host.raw.dtype == np.int32 and host.occluded.dtype == np.bool_
        dev, ran = _query(ctx, rays, tr, mode=m)
        assert np.array_equal(host.raw, dev) and host.mode == ran, m
        assert np.array_equal(host.occluded, dev != 0)
        out = np.full(50000, 7, dtype=np.int32)
        ctx.occluded(rays, tr, index=idx, mode=m, out=out)   # the host entry keeps what is not listed, too
        assert np.array_equal(out[0::2], dev[0::2]) and (out[1::2] == 7).all()
    assert 0.05 < host.occluded.mean() < 0.95


def test_host_entry_waits_for_a_render_on_another_stream(tor, rscene):
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    side = torch.cuda.Stream()
    buf = torch.zeros((270, 480, 3), dtype=torch.float64, device="cuda")
    rays = R.incoherent_rays(rscene, 4096, 21)
    with torch.cuda.stream(side):
        ctx.render_device(cam, 270, 480, 64, 2.2, 50, tor.make_options(seeding=tor.SEED_SAMPLE), buf.data_ptr(), side.cuda_stream)
    res = ctx.occluded(rays)   # blocking host entry: waits for the render instead of refusing it
    assert np.array_equal(res.raw, _want(rscene, rays))
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ctx.occluded(torch.from_numpy(rays).cuda(), t_range=np.zeros((4096, 2)))   # numpy t_range with tensor rays


def test_a_query_between_renders_changes_no_canvas(tor, rscene):
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    stream = torch.cuda.current_stream().cuda_stream
    rays = R.incoherent_rays(rscene, 100000, 18, (0.0, 1.0))

    def query():
        for m in MODES:
            _query(ctx, rays, time_range=(-3.0, 0.5), mode=m)

    for seeding in (tor.SEED_PIXEL, tor.SEED_SAMPLE):
        opt = tor.make_options(seeding=seeding, accel=tor.ACCEL_BLOCKS | tor.ACCEL_F32)
        a = torch.zeros((54, 96, 3), dtype=torch.float64, device="cuda")
        b = torch.zeros_like(a)
        ctx.render_device(cam, 54, 96, 8, 2.2, 50, opt, a.data_ptr(), stream)
        torch.cuda.synchronize()
        query()
        ctx.render_device(cam, 54, 96, 8, 2.2, 50, opt, b.data_ptr(), stream)
        torch.cuda.synchronize()
        assert torch.equal(a, b), f"seeding {seeding}: a query between two renders changed the canvas"
    # a progressive pass on either side of a query: the one-shot canvas
    opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=tor.ACCEL_BLOCKS | tor.ACCEL_F32)
    pg = tor.Progressive(ctx, cam, 54, 96, 50, opt)
    pg.add(4)
    query()
    pg.add(4)
    one = torch.zeros((54, 96, 3), dtype=torch.float64, device="cuda")
    ctx.render_device(cam, 54, 96, 8, 2.2, 50, opt, one.data_ptr(), stream)
    img = pg.image(2.2)
    torch.cuda.synchronize()
    assert torch.equal(img, one)
    # and the queries still answer as before
    got, _ = _query(ctx, rays[:4096], mode="blocks")
    assert np.array_equal(got, _want(rscene, rays[:4096]))
