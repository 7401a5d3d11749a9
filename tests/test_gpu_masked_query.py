"""Visibility groups and per-ray masks on the MI355X (tor_scene_groups, tor_hit_masked_device, tor_occluded_masked_device,
tor_bounce_masked_device and the _host twins): in every mode the hit record, the any-hit bit and one path step of every ray equal
the restatement on the sub-list the ray sees (tests/masked_restatement.py, worked by hand in tests/test_masked_query.py), bit for
bit.  The shapes are the smallest at which the kernels can go wrong: partial waves, masks that differ inside every wave, super boxes
and block boxes that some lanes of a wave skip and others enter, rays that walk, padding slots, scenes of 0, 1 and 9 objects.

Before it compares, every scene's test asserts from the restatement alone that the comparison means something: at least a tenth of
the rays change their answer against the unmasked query, at least a tenth keep a hit, and every mask value shares a wave with
another value."""
import hashlib

import numpy as np
import pytest
import torch

import bounce_restatement as BR
import hit_restatement as R
import masked_restatement as M

pytestmark = pytest.mark.gpu
MODES = ("auto", "brute", "blocks")
MASKS = np.array([0, 1, 2, 5, 8, 0xF, 0xFFFFFFFF], dtype=np.uint32)


def _ctx(tor, recs, groups=None):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    if groups is not None:
        ctx.set_groups(groups)
    return ctx


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _np(t):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def _states(n, seed):
    return np.asarray(np.random.default_rng(seed).integers(0, 2**63, (n, 4), dtype=np.uint64))


def _meaningful(recs, groups, rays, masks, t_range=None, mixed=True):
    changed, keeps, is_mixed = M.meaningful(recs, groups, rays, masks, t_range)
    assert changed >= 0.1, f"only {changed:.3f} of the rays change their answer against the unmasked query"
    assert keeps >= 0.1, f"only {keeps:.3f} of the rays keep a hit"
    assert is_mixed or not mixed, "a mask value never shares a wave with another value"


def _check(tor, oracle, ctx, recs, groups, rays, masks, t_range=None, time_range=None, modes=MODES, step=True, seed=77):
    """Hit records, any-hit bits and one step of ALL rays in every mode against the restatement; returns {mode: what ran}."""
    n = len(rays)
    want = M.world_hit(recs, groups, rays, masks, t_range)
    want_bit = (R.fields(want)["object"] >= 0).astype(np.int32)
    st = _states(n, seed)
    want_step = M.step(oracle, recs, groups, rays, st, masks) if step and t_range is None else None
    dm = masks if np.ndim(masks) == 0 else _dev(M.ray_masks(masks, n))
    ran = {}
    for m in modes:
        res = ctx.hit(_dev(rays), _dev(t_range), time_range, m, mask=dm)
        bad = R.mismatches(_np(res.raw), want)
        assert not bad, f"hit, mode {m} (ran: {res.mode}): {bad}"
        assert tor.last_note() == "hit (masked): " + res.mode
        ran[m] = res.mode
        occ = ctx.occluded(_dev(rays), _dev(t_range), None, time_range, m, mask=dm)
        got = _np(occ.raw)
        wrong = np.flatnonzero(got != want_bit)
        assert wrong.size == 0, f"occluded, mode {m} (ran: {occ.mode}): {wrong.size} rays differ, first {wrong[:8]}"
        assert tor.last_note() == "occluded (masked): " + occ.mode and occ.mode == res.mode
        if want_step is not None:
            b = ctx.bounce(_dev(rays), _dev(st), None, time_range, m, mask=dm)
            tag = ("step", m, b.mode)
            assert not R.mismatches(_np(b.raw), want_step["raw"]), tag
            assert np.array_equal(_np(b.status), want_step["status"]), tag
            assert _eq(_np(b.attenuation), want_step["attenuation"]), tag
            assert _eq(_np(b.rays), want_step["rays"]), tag
            assert np.array_equal(_np(b.rng), want_step["states"]), tag
            assert tor.last_note() == "bounce (masked): " + b.mode
    return ran


@pytest.fixture(scope="module")
def rscene(tor):
    return tor.random_scene(0xFACADE).to_records()


@pytest.fixture(scope="module")
def anim_frame(tor):
    cam, scene, _ = next(iter(tor.Animation(108, 192).scenes(skip=6)))
    return np.frombuffer(bytes(cam), dtype=np.float64).copy(), scene.to_records()


def _mod4(n):
    return (np.uint32(1) << (np.arange(n) % 4).astype(np.uint32)).astype(np.uint32)


@pytest.mark.parametrize("how", ["mod4", "material"])
def test_random_scene_camera_and_incoherent_rays(tor, oracle, rscene, how):
    groups = _mod4(len(rscene)) if how == "mod4" else tor.groups_by_material(rscene)
    ctx = _ctx(tor, rscene, groups)
    rng = np.random.default_rng(1)
    cam = R.camera_rays(oracle, oracle.camera(), 12, 20)[:197]            # partial waves
    cam_masks = rng.choice(MASKS, len(cam))
    _meaningful(rscene, groups, cam, cam_masks)
    ran = _check(tor, oracle, ctx, rscene, groups, cam, cam_masks)
    assert ran["auto"] == "blocks" and ran["blocks"] == "blocks" and ran["brute"] == "brute force"
    rays = R.incoherent_rays(rscene, 4096, 2)
    masks = rng.choice(MASKS, len(rays))                                  # differ inside every wave
    _meaningful(rscene, groups, rays, masks)
    _check(tor, oracle, ctx, rscene, groups, rays, masks, time_range=(0.0, 1.0))


def test_animation_frame_skips_whole_super_boxes_for_some_lanes(tor, oracle, anim_frame):
    cam, recs = anim_frame
    assert len(recs) == 1601
    lay = tor.debug_accel_layout(tor.Scene.from_records(recs).list(), 0.0, 1.0)
    assert lay is not None and lay[3], "the animation frame should have a two-level culling layout"
    slots = lay[0].reshape(-1)
    groups = _mod4(len(recs))
    first = slots[:64]                                                    # super box 0: block boxes 0..7, 8 slots each
    first = first[first >= 0]
    assert first.size >= 32
    groups[first] = 16                                                    # ... all in one group of their own
    masks_set = np.concatenate([MASKS, np.array([16, 17], dtype=np.uint32)])
    rng = np.random.default_rng(3)
    # half of the rays aim at the objects of super box 0, so that lanes that see it and lanes that do not share its waves
    rays = R.incoherent_rays(recs, 2048, 4)
    k = rng.choice(first, 1024)
    rays[::2, 3:6] = recs[k, 1:4] - rays[::2, 0:3]
    masks = rng.choice(masks_set, len(rays))
    _meaningful(recs, groups, rays, masks)
    sees16 = (masks & 16) != 0
    hit16 = np.isin(R.fields(M.world_hit(recs, groups, rays, masks))["object"], first)
    assert hit16.sum() > 100 and (~sees16).sum() > 500                    # some enter the super box and win there, others skip it
    ctx = _ctx(tor, recs, groups)
    ran = _check(tor, oracle, ctx, recs, groups, rays, masks, time_range=(0.0, 1.0))
    assert ran["auto"] == "blocks"
    cam_rays = R.camera_rays(oracle, cam, 9, 16)
    _check(tor, oracle, ctx, recs, groups, cam_rays, rng.choice(masks_set, len(cam_rays)))


def test_time_groups_most_rays_walk_and_padding_slots(tor, oracle):
    recs = R.group_scene(5)[:693]                                         # not a multiple of 8: padding slots in both layouts
    assert len(recs) % 8 != 0
    groups = _mod4(len(recs))
    rng = np.random.default_rng(5)
    rays = R.incoherent_rays(recs, 1536, 6, (-1.0, 2.5))
    masks = rng.choice(MASKS, len(rays))
    _meaningful(recs, groups, rays, masks)
    ctx = _ctx(tor, recs, groups)
    outside = ((rays[:, 6] < 0.4) | (rays[:, 6] > 0.6)).mean()
    assert outside > 0.9                                                  # most rays lie outside the range below: they walk
    ran = _check(tor, oracle, ctx, recs, groups, rays, masks, time_range=(0.4, 0.6))
    assert ran["blocks"] == "blocks"
    _check(tor, oracle, ctx, recs, groups, rays, masks, step=False)       # the rays' own range: most use the boxes


@pytest.mark.parametrize("n_obj", [0, 1, 9])
def test_tiny_scenes(tor, oracle, n_obj):
    recs = R.group_scene(11, 40)[1:1 + n_obj]
    groups = _mod4(n_obj)
    rng = np.random.default_rng(7)
    rays = R.incoherent_rays(R.group_scene(11, 40), 300, 8)
    if n_obj:                                                             # aim at the objects: a tiny scene is mostly sky
        k = rng.integers(0, n_obj, 300)
        rays[:, 3:6] = recs[k, 1:4] - rays[:, 0:3]
        rays[:, 6] = 0.0
    masks = rng.choice(MASKS, 300)
    if n_obj == 9:
        _meaningful(recs, groups, rays, masks)
    ran = _check(tor, oracle, _ctx(tor, recs, groups if n_obj else None), recs, groups, rays, masks)
    assert all(v.startswith("brute force") for v in ran.values())
    if n_obj == 0:
        assert (R.fields(M.world_hit(recs, groups, rays, masks))["object"] == -1).all()


def test_shadow_segments_that_end_on_a_hidden_lamp(tor, rscene):
    """Segments from points of the scene's box to points ON the surface of a lamp, range (0.001, 1.0): the lamp itself is in the way
    or not as the strict `sol < 1.0` falls -- unless the segment's mask leaves the lamp's group out."""
    LAMP, REST = 8, 1
    small = np.flatnonzero((rscene[:, 0] == 0) & (np.abs(rscene[:, 9]) <= 0.5))
    lamps = small[::6]
    groups = np.full(len(rscene), REST, dtype=np.uint32)
    groups[lamps] = LAMP
    rng = np.random.default_rng(9)
    n = 2048
    k = rng.choice(lamps, n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q = rscene[k, 1:4] + np.abs(rscene[k, 9:10]) * u                      # on the lamp's surface
    p = q + rng.uniform(0.5, 3.0, (n, 1)) * (u + 0.7 * rng.normal(size=(n, 3)))
    p[:, 1] = np.abs(p[:, 1]) + 0.05
    rays, tr = tor.Context.shadow_segments(p, q)
    masks = np.where(rng.random(n) < 0.75, REST, REST | LAMP).astype(np.uint32)
    want = M.occluded(rscene, groups, rays, masks, tr)
    plain = R.fields(R.world_hit(rscene, rays, tr))["object"] >= 0
    assert (want != plain).mean() >= 0.1 and 0.1 <= want.mean() <= 0.9    # the lamp's far side blocked many of them
    _meaningful(rscene, groups, rays, masks, tr)
    ctx = _ctx(tor, rscene, groups)
    for m in MODES:
        occ = ctx.occluded(_dev(rays), _dev(tr), None, None, m, mask=_dev(masks))
        assert np.array_equal(_np(occ.occluded), want), m
        vis = ctx.visible(_dev(p), _dev(q), mask=_dev(masks), mode=m)
        assert np.array_equal(_np(vis), ~want), m
        res = ctx.hit(_dev(rays), _dev(tr), None, m, mask=_dev(masks))
        assert not R.mismatches(_np(res.raw), M.world_hit(rscene, groups, rays, masks, tr)), m


def test_scalar_mask_equals_the_same_value_per_ray_and_lists_keep_unlisted_rays(tor, oracle, rscene):
    groups = _mod4(len(rscene))
    ctx = _ctx(tor, rscene, groups)
    n = 1001
    rays = R.incoherent_rays(rscene, n, 10)
    st = _states(n, 11)
    want = M.world_hit(rscene, groups, rays, 5)
    assert 0.1 < (R.fields(want)["object"] >= 0).mean() and R.mismatches(want, R.world_hit(rscene, rays))
    per_ray = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    idx = np.concatenate([np.arange(1, n, 3), [n, -1, n + 100]]).astype(np.int32)   # entries outside [0, n) are skipped
    listed = np.zeros(n, dtype=bool)
    listed[np.arange(1, n, 3)] = True
    want_step = M.step(oracle, rscene, groups, rays, st, 5, idx)
    for m in MODES:
        a, b = ctx.hit(_dev(rays), None, None, m, mask=5), ctx.hit(_dev(rays), None, None, m, mask=per_ray)
        assert not R.mismatches(_np(a.raw), want) and np.array_equal(_np(a.raw).view(np.uint64), _np(b.raw).view(np.uint64)), m
        a = ctx.occluded(_dev(rays), None, None, None, m, mask=np.uint32(5))
        b = ctx.occluded(_dev(rays), None, None, None, m, mask=np.full(n, 5, dtype=np.uint32))     # numpy words with tensor rays
        assert torch.equal(a.raw, b.raw), m
        # lists: rays that are not listed keep every bit
        out = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        ctx.occluded(_dev(rays), None, idx, None, m, out, mask=per_ray)
        got = _np(out)
        assert np.array_equal(got[listed], (R.fields(want)["object"] >= 0).astype(np.int32)[listed]) and (got[~listed] == 7).all(), m
        r, s = _dev(rays), _dev(st)
        res = ctx.bounce(r, s, idx, None, m, mask=5)
        assert not R.mismatches(_np(res.raw), want_step["raw"]) and np.array_equal(_np(res.status), want_step["status"]), m
        assert _eq(_np(res.rays), want_step["rays"]) and np.array_equal(_np(res.rng), want_step["states"]), m
        assert _eq(_np(res.rays)[~listed], rays[~listed]) and np.array_equal(_np(res.rng)[~listed], st[~listed]), m
        assert _eq(_np(res.attenuation), want_step["attenuation"]), m


def test_bounce_equals_masked_hit_then_scatter_and_mask_zero_draws_nothing(tor, rscene):
    groups = tor.groups_by_material(rscene)
    ctx = _ctx(tor, rscene, groups)
    n = 3000
    rays = R.incoherent_rays(rscene, n, 12)
    st = _states(n, 13)
    masks = np.random.default_rng(14).choice(MASKS, n)
    for m in ("brute", "blocks"):
        r1, s1 = _dev(rays), _dev(st)
        both = ctx.bounce(r1, s1, None, (0.0, 1.0), m, mask=_dev(masks))
        r2, s2 = _dev(rays), _dev(st)
        hit = ctx.hit(r2, None, (0.0, 1.0), m, mask=_dev(masks))
        two = ctx.scatter(r2, hit, s2)
        assert np.array_equal(_np(both.raw).view(np.uint64), _np(hit.raw).view(np.uint64)), m
        assert torch.equal(both.status, two.status) and _eq(_np(both.attenuation), _np(two.attenuation)), m
        assert _eq(_np(r1), _np(r2)) and torch.equal(s1, s2), m
        zero = masks == 0
        assert zero.sum() > 200
        assert (_np(both.status)[zero] == tor.BOUNCE_MISS).all() and (_np(both.object)[zero] == -1).all()
        assert not _np(both.raw)[zero, :7].any() and not _np(both.attenuation)[zero].any()
        assert _eq(_np(r1)[zero], rays[zero]) and np.array_equal(_np(s1)[zero], st[zero]), m
        assert (_np(both.status) == tor.BOUNCE_SCATTERED).sum() > 500


def test_trace_with_a_mask_per_step(tor, oracle, rscene):
    """Step 0 does not see the metal spheres (camera-invisible), the later steps see everything but glass."""
    groups = tor.groups_by_material(rscene)
    ctx = _ctx(tor, rscene, groups)
    rays = R.camera_rays(oracle, oracle.camera(), 10, 16)
    st = _states(len(rays), 15)
    per_ray = np.where(np.arange(len(rays)) % 2 == 0, 1 | 2, 0xFFFFFFFF).astype(np.uint32)

    def mask_of(step):
        return 1 | 4 if step == 0 else per_ray
    want_c, want_s = M.trace(oracle, rscene, groups, rays, st, 6, mask_of)
    plain_c, _ = BR.trace(oracle, rscene, rays, st, 6)
    assert (want_c != plain_c).any(axis=1).mean() >= 0.1
    for m in MODES:
        c, s, _ = ctx.trace(_dev(rays), _dev(st), 6, mode=m, mask=lambda k: 5 if k == 0 else _dev(per_ray))
        assert _eq(_np(c), want_c) and np.array_equal(_np(s), want_s), m
    c, s, _ = ctx.trace(_dev(rays), _dev(st), 6, mask=0xFFFFFFFF)           # every object visible: the unmasked trace
    assert _eq(_np(c), plain_c)


def test_reset_replacing_upload_and_identical_upload(tor, rscene):
    groups = _mod4(len(rscene))
    rays = R.incoherent_rays(rscene, 1024, 16)
    plain = R.world_hit(rscene, rays)
    want = M.world_hit(rscene, groups, rays, 3)
    assert R.mismatches(want, plain)
    scene = tor.Scene.from_records(rscene)
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    dr = _dev(rays)
    for m in MODES:
        assert not R.mismatches(_np(ctx.hit(dr, None, None, m, mask=3).raw), plain), m      # no words yet: every object in every group
    ctx.set_groups(groups)
    for m in MODES:
        assert not R.mismatches(_np(ctx.hit(dr, None, None, m, mask=3).raw), want), m
        assert not R.mismatches(_np(ctx.hit(dr, None, None, m).raw), plain), m               # the unmasked entry never reads them
    ctx.upload(scene.list())                                               # byte-identical: a no-op that keeps the words
    for m in MODES:
        assert not R.mismatches(_np(ctx.hit(dr, None, None, m, mask=3).raw), want), m
    ctx.set_groups(None)
    for m in MODES:
        assert not R.mismatches(_np(ctx.hit(dr, None, None, m, mask=3).raw), plain), m
        assert np.array_equal(_np(ctx.occluded(dr, mode=m, mask=3).raw), (R.fields(plain)["object"] >= 0).astype(np.int32)), m
    ctx.set_groups(groups)
    other = rscene[:-1]
    ctx.upload(tor.Scene.from_records(other).list())                       # a replacing upload resets the words
    for m in MODES:
        assert not R.mismatches(_np(ctx.hit(dr, None, None, m, mask=3).raw), R.world_hit(other, rays)), m


def test_a_render_before_and_after_set_groups_gives_the_same_canvas(tor, rscene):
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    stream = torch.cuda.current_stream().cuda_stream
    opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=tor.ACCEL_BLOCKS | tor.ACCEL_F32)
    hashes = []
    for groups in (None, _mod4(len(rscene)), np.zeros(len(rscene), dtype=np.uint32)):
        if groups is not None:
            ctx.set_groups(groups)
            ctx.hit(_dev(R.incoherent_rays(rscene, 256, 17)), mask=1)      # the words reach the device
        buf = torch.zeros((54, 96, 3), dtype=torch.float64, device="cuda")
        ctx.render_device(cam, 54, 96, 4, 2.2, 50, opt, buf.data_ptr(), stream)
        torch.cuda.synchronize()
        hashes.append(hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest())
    assert len(set(hashes)) == 1


def test_host_entries(tor, oracle, rscene):
    groups = _mod4(len(rscene))
    ctx = _ctx(tor, rscene, groups)
    rng = np.random.default_rng(18)
    n = 1500
    rays = R.incoherent_rays(rscene, n, 19)
    masks = rng.choice(MASKS, n)
    tr = np.stack([np.full(n, 0.001), rng.choice([np.inf, 6.0, 1.5], n)], axis=1)
    want = M.world_hit(rscene, groups, rays, masks, tr)
    _meaningful(rscene, groups, rays, masks, tr)
    idx = np.arange(0, n, 2, dtype=np.int32)
    for m in MODES:
        res = ctx.hit(rays, tr, None, m, mask=masks)                       # numpy in: tor_hit_masked_host
        assert isinstance(res.raw, np.ndarray) and not R.mismatches(res.raw, want), m
        assert not R.mismatches(ctx.hit(rays, tr, None, m, mask=masks.view(np.int32)).raw, want), m
        assert not R.mismatches(ctx.hit(rays, tr, None, m, mask=5).raw, M.world_hit(rscene, groups, rays, 5, tr)), m
        occ = ctx.occluded(rays, tr, mode=m, mask=masks)                   # tor_occluded_masked_host
        assert isinstance(occ.raw, np.ndarray) and np.array_equal(occ.occluded, R.fields(want)["object"] >= 0), m
        out = np.full(n, 7, dtype=np.int32)
        ctx.occluded(rays, tr, index=idx, mode=m, out=out, mask=masks)
        assert np.array_equal(out[0::2], occ.raw[0::2]) and (out[1::2] == 7).all(), m
    st = _states(200, 20)
    step = ctx.bounce(rays[:200], st, mask=masks[:200])                     # numpy in: through the device and back
    want_step = M.step(oracle, rscene, groups, rays[:200], st, masks[:200])
    assert isinstance(step.raw, np.ndarray) and not R.mismatches(step.raw, want_step["raw"])
    assert np.array_equal(step.status, want_step["status"]) and np.array_equal(step.rng, want_step["states"])


def test_refusals(tor, rscene):
    L = tor.lib()
    ctx = tor.Context(0)
    rays = _dev(R.incoherent_rays(rscene, 64, 21))
    with pytest.raises(tor.TorError, match="tor_scene_groups: no scene"):   # a context without a scene
        ctx.set_groups(np.ones(3, dtype=np.uint32))
    for call in (lambda: ctx.hit(rays, mask=1), lambda: ctx.occluded(rays, mask=1),
                 lambda: ctx.bounce(rays, _dev(_states(64, 22)), mask=1)):
        with pytest.raises(tor.TorError, match="no scene uploaded"):
            call()
    ctx.upload(tor.Scene.from_records(rscene).list())
    groups = _mod4(len(rscene))
    ctx.set_groups(groups)
    want = M.world_hit(rscene, groups, _np(rays), 2)
    for bad in (groups[:-1], np.concatenate([groups, groups[:1]]), np.zeros(0, dtype=np.uint32)):
        with pytest.raises(tor.TorError, match="n_objects"):               # the wrong count: nothing changes
            ctx.set_groups(bad)
        assert not R.mismatches(_np(ctx.hit(rays, mask=2).raw), want)
    with pytest.raises(ValueError):
        ctx.set_groups(np.ones(len(rscene)))                               # not integers
    with pytest.raises(ValueError):
        ctx.hit(rays, mask=torch.ones(63, dtype=torch.int32, device="cuda"))   # one word per ray
    with pytest.raises(ValueError):
        ctx.occluded(rays, mask=np.ones(65, dtype=np.uint32))
    with pytest.raises(ValueError):
        ctx.hit(_np(rays), mask=np.ones(5, dtype=np.uint32))
    # what the unmasked entries refuse, through the masked ones
    for kw in ({"time_range": (1.0, 0.5)}, {"time_range": (0.0, float("inf"))}, {"mode": 3}):
        for call in (ctx.hit, ctx.occluded):
            with pytest.raises(tor.TorError, match="tor_(hit|occluded)_masked_device"):
                call(rays, mask=1, **kw)
        with pytest.raises(tor.TorError, match="tor_bounce_masked_device"):
            ctx.bounce(rays, _dev(_states(64, 22)), mask=1, **kw)
    p = rays.data_ptr()
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    import ctypes as C
    rc = L.tor_occluded_masked_device(ctx._h, 64, C.c_void_p(p), None, None, 3, 0.0, 1.0, 0, C.c_void_p(out.data_ptr()), None, None, 1)
    assert rc == tor.ERR_INVALID_ARGUMENT and "n_list" in L.tor_last_error().decode()
    assert not R.mismatches(_np(ctx.hit(rays, mask=2).raw), want)          # and the context still answers
