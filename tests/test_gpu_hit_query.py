"""Closest-hit queries on the MI355X (tor_hit_device / tor_hit_host): every mode equals the numpy restatement of world.hit
(tests/hit_restatement.py, anchored to the CPU oracle by tests/test_hit_query.py) bit for bit, field by field -- on random_scene,
an animation frame (two-level culling layout), a scene of several time groups, cut and shifted t ranges, rays from inside spheres,
grazing rays, coincident duplicates, degenerate rays and an empty scene -- and a query leaves the render path's canvases alone."""
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


def _query(ctx, rays, t_range=None, time_range=None, mode="auto"):
    dr = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64)).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(t_range, dtype=np.float64)).cuda() if t_range is not None else None
    res = ctx.hit(dr, dt, time_range, mode)
    torch.cuda.synchronize()
    return res.raw.cpu().numpy(), res.mode


def _check(ctx, recs, rays, t_range=None, time_range=None, modes=MODES):
    """Every mode against the restatement; returns {mode: what ran}."""
    want = R.world_hit(recs, rays, t_range)
    ran = {}
    for m in modes:
        got, ran[m] = _query(ctx, rays, t_range, time_range, m)
        bad = R.mismatches(got, want)
        assert not bad, f"mode {m} (ran: {ran[m]}) differs from the restatement: {bad}"
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
    cam_rays = R.camera_rays(oracle, oracle.camera(), 108, 192)
    ran, want = _check(ctx, rscene, cam_rays)
    assert ran["auto"] == "blocks" and ran["blocks"] == "blocks" and ran["brute"] == "brute force"
    assert 0.2 < (R.fields(want)["object"] >= 0).mean() < 0.95
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
    _check(ctx, recs, rays)                                # the rays' own range
    ran, _ = _check(ctx, recs, rays, time_range=(-0.25, 1.0))  # most rays outside: the brute-force walk answers them
    assert ran["blocks"] == "blocks"
    _check(ctx, recs, rays, time_range=(0.5, 0.5))


def test_cut_and_shifted_t_ranges(tor, rscene):
    rng = np.random.default_rng(4)
    ctx = _ctx(tor, rscene)
    rays = R.incoherent_rays(rscene, 32768, 5)
    n = len(rays)
    t_min = rng.choice([0.0, 0.001, 0.5, 3.0, 20.0, -2.0, -np.inf, np.nan], n)   # negative / NaN t_min: the brute-force walk
    t_max = t_min + rng.choice([0.25, 1.0, 4.0, np.inf], n)
    t_max = np.where(np.isnan(t_max), 5.0, t_max)
    tr = np.stack([t_min, t_max], axis=1)
    _, want = _check(ctx, rscene, rays, tr)
    assert (R.fields(want)["object"] >= 0).sum() > 1000


def test_rays_from_inside_spheres(tor, rscene):
    rng = np.random.default_rng(6)
    ctx = _ctx(tor, rscene)
    k = rng.integers(0, len(rscene), 8192)
    o = rscene[k, 1:4] + rng.uniform(-0.05, 0.05, (8192, 3)) * np.abs(rscene[k, 9:10])
    d = rng.normal(size=(8192, 3))
    rays = np.concatenate([o, d, rng.uniform(0, 1, (8192, 1))], axis=1)
    _, want = _check(ctx, rscene, rays)
    f = R.fields(want)
    assert ((f["object"] >= 0) & (f["front_face"] == 0)).sum() > 4000


def test_grazing_rays_and_coincident_duplicates(tor, rscene):
    """Rays that pass every sphere at its extreme coordinate along x, y and z (+- 2 ulps, the direction's component along that axis
    exactly 0): the discriminant's sign there is decided by rounding -- and a box that did not hold its spheres with a margin loses
    such hits.  Duplicates of the first 60 objects are appended: exact ties, which go to the lower index."""
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
    f = R.fields(want)
    assert (f["object"] >= 0).sum() > 1000
    # coincident duplicates: camera-like rays at the first 60 objects, whose copies sit at 485 + k
    k = np.arange(60)
    o = np.tile([13.0, 2.0, 3.0], (60, 1))
    d = rscene[k, 1:4] - o
    tie_rays = np.concatenate([o, d, np.zeros((60, 1))], axis=1)
    _, want = _check(ctx, recs, tie_rays)
    assert (R.fields(want)["object"] < 485).all()


@pytest.mark.parametrize("which", ["random", "groups"])
def test_far_origin_grazing_rays(tor, rscene, which):
    """From 1e4 .. 1e6 units away the reference's discriminant rounds by ~eps |oc|^2 and accepts rays that pass several 1e-6 above
    a sphere -- farther out than a culling box's margin.  Every mode must still give the reference's record: such origins walk."""
    recs = rscene if which == "random" else R.group_scene(19)
    ctx = _ctx(tor, recs)
    rays = R.far_grazing_rays(recs, 20)
    ran, want = _check(ctx, recs, rays, time_range=(0.0, 1.0))
    assert ran["auto"] == "blocks"
    f = R.fields(want)
    hit = f["object"] >= 0
    above = rays[:, 1] - (recs[np.maximum(f["object"], 0), 2] + np.abs(recs[np.maximum(f["object"], 0), 9]))
    assert (hit & (above > 2e-6)).sum() > 20, "the generator must produce hits beyond a box's margin"


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
    _check(ctx, recs, rays)
    _check(ctx, recs, rays, time_range=(0.0, 1.0))


def test_empty_scene_and_small_scenes(tor):
    rays = R.incoherent_rays(R.group_scene(11, 40), 1000, 12)
    ctx = _ctx(tor, np.zeros((0, 16)))
    for m in MODES:
        got, ran = _query(ctx, rays, mode=m)
        assert (R.fields(got)["object"] == -1).all() and not R.mismatches(got, R.world_hit(np.zeros((0, 16)), rays))
        assert ran.startswith("brute force")
    recs = R.group_scene(11, 40)   # below the culling layout's minimum: every mode runs the brute force
    ran, _ = _check(_ctx(tor, recs), recs, rays)
    assert ran["blocks"].startswith("brute force (")


@pytest.mark.parametrize("n", [0, 1, 63, 65])
def test_batch_sizes(tor, rscene, n):
    ctx = _ctx(tor, rscene)
    rays = R.incoherent_rays(rscene, max(n, 1), 13)[:n]
    for m in MODES:
        got, _ = _query(ctx, rays, mode=m)
        assert got.shape == (n, 8) and not R.mismatches(got, R.world_hit(rscene, rays))


def _gpu_raw(ctx, rays_t, mode, time_range=None):
    res = ctx.hit(rays_t, None, time_range, mode)
    return res.raw, res.mode


def test_four_million_rays(tor, rscene):
    n = 1 << 22
    rays = R.incoherent_rays(rscene, n, 14)
    rt = torch.from_numpy(rays).cuda()
    ctx = _ctx(tor, rscene)
    outs = {m: _gpu_raw(ctx, rt, m)[0] for m in MODES}
    torch.cuda.synchronize()
    ref = outs["brute"].view(torch.int64)
    for m in ("auto", "blocks"):
        assert torch.equal(outs[m].view(torch.int64), ref), f"mode {m} differs from the brute force over 4 M rays"
    sub = slice(0, n, 256)
    assert not R.mismatches(outs["blocks"][sub].cpu().numpy(), R.world_hit(rscene, rays[sub]))


@pytest.mark.parametrize("which", ["random", "anim", "groups"])
def test_brute_force_and_blocks_agree_over_a_million_rays(tor, rscene, anim_frame, which):
    recs = {"random": rscene, "anim": anim_frame[1], "groups": R.group_scene(15)}[which]
    ctx = _ctx(tor, recs)
    rays = R.incoherent_rays(recs, 1 << 20, 16, (0.0, 1.0))
    rt = torch.from_numpy(rays).cuda()
    brute, _ = _gpu_raw(ctx, rt, "brute")
    blocks, ran = _gpu_raw(ctx, rt, "blocks")
    torch.cuda.synchronize()
    assert ran == "blocks"
    assert torch.equal(brute.view(torch.int64), blocks.view(torch.int64))
    assert int((brute.view(torch.int32)[:, 14] >= 0).sum()) > 100000


def test_host_entry_equals_device_entry(tor, rscene):
    ctx = _ctx(tor, rscene)
    rng = np.random.default_rng(17)
    rays = R.incoherent_rays(rscene, 50000, 17)
    tr = np.stack([rng.choice([0.001, 1.0], len(rays)), rng.choice([np.inf, 6.0], len(rays))], axis=1)
    for m in MODES:
        host = ctx.hit(rays, tr, mode=m)               # numpy in: tor_hit_host
        assert isinstance(host.raw, np.ndarray)
        dev, _ = _query(ctx, rays, tr, mode=m)
        assert np.array_equal(host.raw.view(np.uint64), dev.view(np.uint64)), m
        assert host.object.dtype == np.int32 and np.array_equal(host.t, host.raw[:, 6])


def test_host_entry_waits_for_a_render_on_another_stream(tor, rscene):
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    side = torch.cuda.Stream()
    buf = torch.zeros((270, 480, 3), dtype=torch.float64, device="cuda")
    rays = R.incoherent_rays(rscene, 4096, 21)
    with torch.cuda.stream(side):
        ctx.render_device(cam, 270, 480, 64, 2.2, 50, tor.make_options(seeding=tor.SEED_SAMPLE), buf.data_ptr(), side.cuda_stream)
    res = ctx.hit(rays)   # blocking host entry: waits for the render instead of refusing it
    assert not R.mismatches(res.raw, R.world_hit(rscene, rays))
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ctx.hit(torch.from_numpy(rays).cuda(), t_range=np.zeros((4096, 2)))   # numpy t_range with tensor rays


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
    assert not R.mismatches(got, R.world_hit(rscene, rays[:4096]))
