"""Radiance queries on the MI355X (tor_radiance_device / tor_radiance_host / tor_camera_rays_device): camera rays and states equal the
restatement bit for bit; camera paths through every mode equal the CPU oracle's sample sums and moments; the reference's one stream
per pixel, chained through camera_rays and radiance on the device, resolves to tor_render_device's and the oracle's canvas; arbitrary
rays and states equal the numpy restatement of radiance() (tests/radiance_restatement.py, anchored by tests/test_radiance_query.py);
a query leaves renders alone, and bad arguments leave the outputs untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import hit_restatement as H
import radiance_restatement as RR

pytestmark = pytest.mark.gpu
MODES = ("auto", "brute", "blocks")


def _ctx(tor, recs):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    return ctx


def _cam(tor, cam24):
    return tor.Camera.from_buffer_copy(np.ascontiguousarray(cam24, dtype=np.float64).tobytes())


def _radiance(ctx, rays, states, depth, mode, time_range=None):
    dr = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64)).cuda()
    ds = torch.from_numpy(np.ascontiguousarray(np.asarray(states).view(np.int64))).cuda()
    color, st, ran = ctx.radiance(dr, ds, depth, time_range, mode)
    torch.cuda.synchronize()
    return color.cpu().numpy(), st.cpu().numpy().view(np.uint64), ran


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


@pytest.fixture(scope="module")
def rscene(tor):
    return tor.random_scene(0xFACADE).to_records()


@pytest.fixture(scope="module")
def anim_frame(tor):
    cam, scene, _ = next(iter(tor.Animation(108, 192).scenes(skip=6)))
    return np.frombuffer(bytes(cam), dtype=np.float64).copy(), scene.to_records()


def test_camera_rays_equal_the_restatement(tor, oracle, rscene):
    ctx = _ctx(tor, rscene)
    cam24 = oracle.camera()
    nrows, ncols = 18, 32
    rays, st = ctx.camera_rays(_cam(tor, cam24), nrows, ncols, 5, 2, tor.SEED_SAMPLE)
    torch.cuda.synchronize()
    want_r, want_s = RR.camera_rays(oracle, cam24, nrows, ncols, None, 5, 2)
    assert _same(rays.cpu().numpy(), want_r) and _same(st.cpu().numpy(), want_s)
    # sample 0 of every pixel: hit_restatement's camera rays
    rays0, _ = ctx.camera_rays(_cam(tor, cam24), nrows, ncols, 0, 1, tor.SEED_SAMPLE)
    assert _same(rays0.cpu().numpy(), H.camera_rays(oracle, cam24, nrows, ncols, 0))
    # TOR_SEED_PIXEL on seed2(row, col) states, through a pixel list (entries outside the canvas are skipped)
    pix = np.array([0, 7, 33, nrows * ncols - 1, 100, 5], dtype=np.int32)
    seeds = tor.rng_seed2(pix // ncols, pix % ncols)
    rp, sp = ctx.camera_rays(_cam(tor, cam24), nrows, ncols, 0, 1, tor.SEED_PIXEL, pix, torch.from_numpy(seeds.view(np.int64)).cuda())
    torch.cuda.synchronize()
    want_r, want_s = RR.camera_rays(oracle, cam24, nrows, ncols, pix, states=seeds)
    assert _same(rp.cpu().numpy(), want_r) and _same(sp.cpu().numpy(), want_s)


@pytest.mark.parametrize("depth", [0, 1, 2, 50])
def test_camera_paths_equal_the_oracle_sums(tor, oracle, rscene, depth):
    cam24 = oracle.camera()
    nrows, ncols, first, ns = 36, 64, 2, 4
    ctx = _ctx(tor, rscene)
    rays, st = ctx.camera_rays(_cam(tor, cam24), nrows, ncols, first, ns, tor.SEED_SAMPLE)
    want_s, want_m = oracle.accumulate(nrows, ncols, first, ns, cam24, rscene, max_depth=depth)
    for m in MODES:
        color, st_out, ran = ctx.radiance(rays, st.clone(), depth, None, m)
        torch.cuda.synchronize()
        s, mo = RR.sums_and_moments(color.cpu().numpy(), nrows * ncols, ns)
        assert _same(s, want_s.reshape(-1, 3)) and _same(mo, want_m.reshape(-1, 3)), (m, ran)
        if depth == 0:
            assert (color == 0).all() and torch.equal(st_out, st)
        assert ran == ("brute force" if m == "brute" else "blocks")


def test_pixel_list_and_time_groups_equal_the_oracle(tor, oracle, rscene):
    cam24 = oracle.camera()
    nrows, ncols, ns = 36, 64, 3
    pix = np.sort(np.random.default_rng(3).choice(nrows * ncols, 300, replace=False)).astype(np.int32)
    for recs, cam in ((rscene, cam24), (H.group_scene(5, 300), oracle.camera(look_from=(0, 6, 18), look_at=(0, 1, 0), vfov=50.0,
                                                                             shutter_open=-0.5, shutter_close=2.0))):
        ctx = _ctx(tor, recs)
        rays, st = ctx.camera_rays(_cam(tor, cam), nrows, ncols, 0, ns, tor.SEED_SAMPLE, pix)
        want_s, want_m = oracle.accumulate(nrows, ncols, 0, ns, cam, recs, max_depth=50, pixels=pix)
        for m in MODES:
            color, _, ran = ctx.radiance(rays, st.clone(), 50, None, m)
            torch.cuda.synchronize()
            s, mo = RR.sums_and_moments(color.cpu().numpy(), pix.size, ns)
            assert _same(s, want_s.reshape(-1, 3)[pix]) and _same(mo, want_m.reshape(-1, 3)[pix]), (m, ran)


def test_reference_streams_end_to_end(tor, oracle, rscene):
    """seed2(row, col) once; per sample camera_rays(SEED_PIXEL) -> radiance -> acc + color, in order: tor_resolve_device(acc) is
    tor_render_device's TOR_SEED_PIXEL canvas and the oracle's (SEED_PIXEL / SEQUENTIAL / PORTABLE / STRICT) -- the unquantised
    colours and the returned states, bit for bit."""
    cam24 = oracle.camera()
    nrows, ncols, spp, depth, gamma = 24, 40, 4, 50, 2.2
    ctx = _ctx(tor, rscene)
    cam = _cam(tor, cam24)
    pix = np.arange(nrows * ncols)
    st = torch.from_numpy(tor.rng_seed2(pix // ncols, pix % ncols).view(np.int64)).cuda()
    acc = torch.zeros((nrows * ncols, 3), dtype=torch.float64, device="cuda")
    for _ in range(spp):
        rays, st = ctx.camera_rays(cam, nrows, ncols, 0, 1, tor.SEED_PIXEL, None, st)
        color, st, _ = ctx.radiance(rays, st, depth)
        acc = acc + color
    got = torch.empty_like(acc)
    ctx.resolve_device(acc.data_ptr(), acc.numel(), spp, gamma, got.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ref = torch.empty_like(acc)
    ctx.render_device(cam, nrows, ncols, spp, gamma, depth, tor.make_options(seeding=tor.SEED_PIXEL), ref.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = oracle.render(nrows, ncols, spp, cam24, rscene, max_depth=depth, gamma=gamma, seeding=oracle.SEED_PIXEL,
                         math=oracle.MATH_PORTABLE, arith=oracle.ARITH_STRICT, accum=oracle.ACCUM_SEQUENTIAL).pixels
    assert _same(ref.cpu().numpy(), want.reshape(-1, 3))
    assert _same(got.cpu().numpy(), want.reshape(-1, 3))


def _arbitrary_rays(recs, seed):
    rng = np.random.default_rng(seed)
    inc = H.incoherent_rays(recs, 1500, seed, (-0.5, 1.5))
    far = H.far_grazing_rays(recs, seed)[:300]
    big = np.asarray(recs)[np.abs(np.asarray(recs)[:, 9]) > 0.3][:20]
    inside = np.concatenate([big[:, 1:4] + rng.uniform(-0.05, 0.05, (big.shape[0], 3)), rng.normal(size=(big.shape[0], 3)),
                             rng.uniform(0, 1, (big.shape[0], 1))], axis=1)
    odd = np.array([[0, 1, 0, 0, 0, 0, 0.5], [0, 1, 0, 1, 0.2, 0, np.nan], [0, 1, 0, -1, 0.1, 0.3, 7.0], [0, 1, 0, 0.3, -1, 0.1, -3.0],
                    [0, 0.5, 0, 1, 0, 0, np.inf]], dtype=np.float64)
    rays = np.concatenate([inc, far, inside, odd])
    st = np.asarray(np.random.default_rng(seed + 1).integers(0, 2**63, (rays.shape[0], 4), dtype=np.uint64))
    return rays, st


def test_arbitrary_rays_equal_the_restatement(tor, oracle, rscene, anim_frame):
    cases = [(rscene, _arbitrary_rays(rscene, 11), (0.0, 1.0)),
             (rscene, _arbitrary_rays(rscene, 12), (0.25, 0.75)),   # time_lo > 0: metal and glass bounces at time 0 stay exact
             (RR.three_material_scene(), _arbitrary_rays(RR.three_material_scene(), 13), None),
             (anim_frame[1], _arbitrary_rays(anim_frame[1], 14), None)]
    for recs, (rays, st), tr in cases:
        ctx = _ctx(tor, recs)
        for depth in (50, 1, 0):
            want_c, want_s = RR.radiance(oracle, recs, rays, st, depth)
            for m in MODES:
                color, st_out, ran = _radiance(ctx, rays, st, depth, m, tr)
                bad_c = ~((color.view(np.uint64) == want_c.view(np.uint64)) | (np.isnan(color) & np.isnan(want_c))).all(axis=1)
                assert not bad_c.any(), (m, ran, depth, np.nonzero(bad_c)[0][:10])
                assert _same(st_out, want_s), (m, ran, depth)
            if depth == 50 and len(recs) > 8:
                assert ran == "blocks"


def test_empty_scene_and_host_entry(tor, oracle, rscene):
    rays, st = _arbitrary_rays(rscene, 21)
    ctx = _ctx(tor, np.zeros((0, 16)))
    want_c, want_s = RR.radiance(oracle, np.zeros((0, 16)), rays, st, 50)
    assert _same(want_s, st)
    for m in MODES:
        color, st_out, _ = _radiance(ctx, rays, st, 50, m)
        assert ((color.view(np.uint64) == want_c.view(np.uint64)) | (np.isnan(color) & np.isnan(want_c))).all()
        assert _same(st_out, st)
    ctx = _ctx(tor, rscene)
    want_c, want_s = RR.radiance(oracle, rscene, rays, st, 50)
    color, st_out, ran = ctx.radiance(rays, st, 50)        # numpy: tor_radiance_host
    assert ((color.view(np.uint64) == want_c.view(np.uint64)) | (np.isnan(color) & np.isnan(want_c))).all() and _same(st_out, want_s)
    assert ran == "blocks" and st_out.dtype == np.uint64
    assert tor.last_note() == "radiance: blocks"


def test_query_leaves_renders_alone_and_bad_arguments_touch_nothing(tor, oracle, rscene):
    ctx = _ctx(tor, rscene)
    cam = _cam(tor, oracle.camera())
    nrows, ncols = 36, 64
    opts = tor.make_options(seeding=tor.SEED_SAMPLE)
    s = torch.cuda.current_stream().cuda_stream
    a = torch.empty((nrows * ncols, 3), dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    ctx.render_device(cam, nrows, ncols, 4, 2.2, 50, opts, a.data_ptr(), s)
    rays, st = ctx.camera_rays(cam, nrows, ncols, 0, 2, tor.SEED_SAMPLE)
    ctx.radiance(rays, st, 50, (0.3, 0.6))
    ctx.render_device(cam, nrows, ncols, 4, 2.2, 50, opts, b.data_ptr(), s)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    L = tor.lib()
    color = torch.full((rays.shape[0], 3), 7.0, dtype=torch.float64, device="cuda")
    st0 = st.clone()
    n = rays.shape[0]
    for args in ((n, rays.data_ptr(), st.data_ptr(), -1, 0.0, 1.0, 0), (n, rays.data_ptr(), st.data_ptr(), 5, 1.0, 0.0, 0),
                 (n, rays.data_ptr(), st.data_ptr(), 5, 0.0, 1.0, 3), (-1, rays.data_ptr(), st.data_ptr(), 5, 0.0, 1.0, 0),
                 (n, rays.data_ptr(), 0, 5, 0.0, 1.0, 0)):
        rc = L.tor_radiance_device(ctx._h, args[0], C.c_void_p(args[1]), C.c_void_p(args[2]), args[3], args[4], args[5], args[6],
                                   C.c_void_p(color.data_ptr()), C.c_void_p(s))
        assert rc == tor.ERR_INVALID_ARGUMENT, args
    torch.cuda.synchronize()
    assert (color == 7.0).all() and torch.equal(st, st0)
    out_r = torch.full((4, 7), 3.0, dtype=torch.float64, device="cuda")
    out_s = torch.full((4, 4), 3, dtype=torch.int64, device="cuda")
    for args in ((1, 64, 0, 4, 0, 1, 1), (36, 64, 0, 4, 0, 2, 0), (36, 64, 0, 4, 0, 1, 2), (36, 64, 0, 4, -1, 1, 1)):
        pix = torch.arange(4, dtype=torch.int32, device="cuda")
        rc = L.tor_camera_rays_device(ctx._h, C.byref(cam), args[0], args[1], C.c_void_p(pix.data_ptr()), args[3], args[4], args[5],
                                      args[6], C.c_void_p(out_s.data_ptr()), C.c_void_p(out_r.data_ptr()), C.c_void_p(s))
        assert rc == tor.ERR_INVALID_ARGUMENT, args
    torch.cuda.synchronize()
    assert (out_r == 3.0).all() and (out_s == 3).all()
