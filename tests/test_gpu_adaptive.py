"""Adaptive sampling on the MI355X: a pass over a pixel list gives the listed pixels exactly what a full-frame pass gives them
and leaves the others alone, the select is the documented test bit for bit, and an adaptive render is exact per pixel -- the
pixels that stopped at c samples are a uniform c-spp render there, whatever the schedule, shard, checkpoint or context."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTH = 50


@pytest.fixture(scope="module")
def torch():
    import torch as T
    return T


@pytest.fixture(scope="module")
def scene(tor):
    return tor.random_scene(0xFACADE)


@pytest.fixture(scope="module")
def ctx(tor, scene):
    c = tor.Context()
    c.upload(scene.list())
    yield c
    c.close()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _one_shot(tor, torch, ctx, h, w, n, **opt):
    rows = len(tor.shard_rows(h, max(opt.get("row_tile", 1), 1), opt.get("shard_index", 0), max(opt.get("shard_count", 1), 1)))
    buf = torch.empty((rows, w, 3), dtype=torch.float64, device="cuda")
    ctx.render_device(tor.camera(), h, w, n, 2.2, DEPTH, tor.make_options(seeding=tor.SEED_SAMPLE, **opt), buf.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _accumulate(tor, torch, ctx, h, w, first, n, opt, sums, mom, lst=None):
    if lst is None:
        ctx.accumulate_device(tor.camera(), h, w, first, n, DEPTH, opt, sums.data_ptr(), mom.data_ptr(), _stream(torch))
    else:
        ctx.accumulate_list_device(tor.camera(), h, w, lst.data_ptr(), lst.numel(), first, n, DEPTH, opt, sums.data_ptr(), mom.data_ptr(),
                                   _stream(torch))


@pytest.mark.parametrize("accel", [0, 3])
def test_full_list_equals_plain_accumulate(tor, torch, ctx, accel):
    h, w = 54, 96
    opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel)
    z = lambda: torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    s0, m0, s1, m1 = z(), z(), z(), z()
    full = torch.arange(h * w, dtype=torch.int32, device="cuda")
    for first, n in ((0, 24), (24, 40)):
        _accumulate(tor, torch, ctx, h, w, first, n, opt, s0, m0)
        _accumulate(tor, torch, ctx, h, w, first, n, opt, s1, m1, full)
    torch.cuda.synchronize()
    assert np.array_equal(s1.cpu().numpy(), s0.cpu().numpy())
    assert np.array_equal(m1.cpu().numpy(), m0.cpu().numpy())
    assert float(m0.sum()) > 0.0
    # an empty list is a no-op
    ctx.accumulate_list_device(tor.camera(), h, w, full.data_ptr(), 0, 64, 8, DEPTH, opt, s1.data_ptr(), m1.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(s1.cpu().numpy(), s0.cpu().numpy())


@pytest.mark.parametrize("accel", [0, 3])
def test_subset_list_touches_only_listed_pixels(tor, torch, ctx, accel):
    h, w = 61, 77
    opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel)
    rng = np.random.default_rng(100 + accel)
    pix = np.sort(rng.choice(h * w, size=h * w // 3, replace=False)).astype(np.int32)
    lst = torch.from_numpy(pix).cuda()
    z = lambda: torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    prior_s, prior_m, s, m, want_s, want_m = z(), z(), z(), z(), z(), z()
    _accumulate(tor, torch, ctx, h, w, 0, 8, opt, prior_s, prior_m)
    _accumulate(tor, torch, ctx, h, w, 0, 8, opt, s, m)
    _accumulate(tor, torch, ctx, h, w, 8, 19, opt, s, m, lst)
    _accumulate(tor, torch, ctx, h, w, 0, 27, opt, want_s, want_m)
    torch.cuda.synchronize()
    S, M = s.cpu().numpy().reshape(-1, 3), m.cpu().numpy().reshape(-1, 3)
    on = np.zeros(h * w, dtype=bool)
    on[pix] = True
    assert np.array_equal(S[on], want_s.cpu().numpy().reshape(-1, 3)[on])
    assert np.array_equal(M[on], want_m.cpu().numpy().reshape(-1, 3)[on])
    assert np.array_equal(S[~on], prior_s.cpu().numpy().reshape(-1, 3)[~on])
    assert np.array_equal(M[~on], prior_m.cpu().numpy().reshape(-1, 3)[~on])


H, W, PASS, MAXS, REL = 180, 320, 16, 256, 0.1


@pytest.fixture(scope="module")
def adaptive_run(tor, torch, ctx):
    ad = tor.Adaptive(ctx, tor.camera(), H, W, DEPTH, tor.make_options(seeding=tor.SEED_SAMPLE), rel_tol=REL, pass_samples=PASS,
                      max_samples=MAXS)
    assert ad.run() == MAXS
    img = ad.image(2.2)
    torch.cuda.synchronize()
    return ad, ad.counts().cpu().numpy(), img.cpu().numpy()


def test_adaptive_run_is_exact_per_pixel(tor, torch, ctx, adaptive_run):
    ad, counts, img = adaptive_run
    levels = np.unique(counts)
    assert set(levels.tolist()) <= set(range(PASS, MAXS + 1, PASS))
    assert len(levels) >= 2 and levels.min() < MAXS
    assert ad.total_samples() == int(counts.astype(np.int64).sum()) < H * W * MAXS
    for c in levels:
        sel = counts == c
        want = _one_shot(tor, torch, ctx, H, W, int(c))
        assert np.array_equal(img[sel], want[sel]), f"count {c}: {(img[sel] != want[sel]).sum()} values differ from a uniform render"
    # resolve_counts == resolve at one count, in place too
    sums = ad.sums
    flat = torch.full((H, W), 64, dtype=torch.int32, device="cuda")
    a, b = torch.empty_like(sums), sums.clone()
    ctx.resolve_device(sums.data_ptr(), sums.numel(), 64, 2.2, a.data_ptr(), _stream(torch))
    ctx.resolve_counts_device(b.data_ptr(), flat.data_ptr(), H * W, 2.2, b.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    cv = ad.to_canvas(tor.new_canvas(H, W, 1, 2.2))
    assert cv.samples_per_pixel == MAXS and np.array_equal(cv.pixels, img)


def test_select_matches_numpy(tor, torch, ctx):
    h, w, n = 54, 96, 32
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    sums = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    mom = torch.zeros_like(sums)
    _accumulate(tor, torch, ctx, h, w, 0, n, opt, sums, mom)
    torch.cuda.synchronize()
    S, M = sums.cpu().numpy(), mom.cpu().numpy()
    rng = np.random.default_rng(3)
    for pix in (np.arange(h * w, dtype=np.int32), np.sort(rng.choice(h * w, size=1500, replace=False)).astype(np.int32)):
        for abs_tol, rel_tol in ((0.0, 0.1), (2e-3, 0.02), (0.0, 0.0), (1.0, 0.0)):
            lst = torch.from_numpy(pix).cuda()
            out = torch.full_like(lst, -9)
            counts = torch.full((h, w), -7, dtype=torch.int32, device="cuda")
            k = ctx.adaptive_select_device(sums.data_ptr(), mom.data_ptr(), lst.data_ptr(), len(pix), n, abs_tol, rel_tol, out.data_ptr(),
                                           counts.data_ptr(), _stream(torch))
            want = tor.adaptive_select_host(S, M, pix, n, abs_tol, rel_tol)
            assert k == len(want) and np.array_equal(out.cpu().numpy()[:k], want), (abs_tol, rel_tol)
            assert np.all(out.cpu().numpy()[k:] == -9)
            c = counts.cpu().numpy().reshape(-1)
            on = np.zeros(h * w, dtype=bool)
            on[pix] = True
            assert np.all(c[on] == n) and np.all(c[~on] == -7)
    k = ctx.adaptive_select_device(sums.data_ptr(), mom.data_ptr(), lst.data_ptr(), 0, n, 0.0, 0.1, out.data_ptr(), counts.data_ptr(),
                                   _stream(torch))
    assert k == 0


def test_select_on_a_4k_list(tor, torch, ctx):
    # 8.3 M entries: more blocks than the scan kernel has threads
    h, w, n = 2160, 3840, 64
    g = torch.Generator(device="cuda").manual_seed(11)
    q = torch.rand((h * w, 3), generator=g, dtype=torch.float64, device="cuda")
    u = torch.rand((h * w, 3), generator=g, dtype=torch.float64, device="cuda")
    sums = torch.round(q * n * 2.0 ** 36) / 2.0 ** 36  # multiples of 2^-36 in [0, n], like n samples in [0, 1]
    mom = torch.round(sums * sums / n * (1.0 + 0.5 * u) * 2.0 ** 36) / 2.0 ** 36  # a variance up to sums^2 / (2 n (n - 1))
    lst = torch.arange(h * w, dtype=torch.int32, device="cuda")
    out = torch.empty_like(lst)
    counts = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    k = ctx.adaptive_select_device(sums.data_ptr(), mom.data_ptr(), lst.data_ptr(), h * w, n, 0.0, 0.05, out.data_ptr(), counts.data_ptr(),
                                   _stream(torch))
    want = tor.adaptive_select_host(sums.cpu().numpy(), mom.cpu().numpy(), np.arange(h * w), n, 0.0, 0.05)
    assert 0 < len(want) < h * w
    assert k == len(want) and np.array_equal(out[:k].cpu().numpy(), want)
    assert bool((counts == n).all())


def test_adaptive_row_matches_the_oracle(tor, oracle, ref_scene, ref_camera, adaptive_run):
    objs, _ = ref_scene
    _, counts, img = adaptive_run
    r = int(np.argmax([len(np.unique(counts[i])) for i in range(H)]))  # the row with the most count levels
    levels = np.unique(counts[r])
    assert len(levels) >= 2
    if len(levels) > 4:  # (the oracle is a CPU renderer: the lowest, the highest and two between)
        levels = levels[[0, len(levels) // 3, 2 * len(levels) // 3, -1]]
    for c in levels:
        want = oracle.render(H, W, int(c), ref_camera, objs, seeding=oracle.SEED_SAMPLE, math=1, arith=0, accum=1, rows=(r, r + 1)).pixels[r]
        sel = counts[r] == c
        assert np.array_equal(img[r][sel], want[sel]), f"row {r}, count {c}: differs from the oracle"


def test_checkpoint_and_resume_in_a_new_context(tor, torch, scene, adaptive_run, tmp_path):
    _, counts, img = adaptive_run
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    policy = dict(rel_tol=REL, pass_samples=PASS, max_samples=MAXS)
    first = tor.Context()
    first.upload(scene.list())
    ad = tor.Adaptive(first, tor.camera(), H, W, DEPTH, opt, **policy)
    for _ in range(4):
        ad.step()
    assert ad.samples == 4 * PASS and 0 < ad.active < H * W
    st = ad.state()
    np.savez(tmp_path / "ckpt.npz", **{k: np.asarray(v) for k, v in st.items()})
    del ad
    first.close()
    second = tor.Context()
    second.upload(scene.list())
    z = np.load(tmp_path / "ckpt.npz")
    ad = tor.Adaptive.from_state(second, tor.camera(), H, W, DEPTH, opt, {k: z[k] for k in z.files} | {"samples": int(z["samples"])},
                                 **policy)
    assert ad.samples == 4 * PASS and ad.active == len(st["list"])
    ad.run()
    got = ad.image(2.2)
    torch.cuda.synchronize()
    assert np.array_equal(ad.counts().cpu().numpy(), counts)
    assert np.array_equal(got.cpu().numpy(), img)
    second.close()


def test_row_shard_is_exact_per_pixel(tor, torch, ctx):
    h, w, count, tile = 90, 160, 2, 4
    for k in range(count):
        shard = dict(shard_index=k, shard_count=count, row_tile=tile)
        ad = tor.Adaptive(ctx, tor.camera(), h, w, DEPTH, tor.make_options(seeding=tor.SEED_SAMPLE, **shard), rel_tol=REL,
                          pass_samples=PASS, max_samples=128)
        ad.run()
        counts = ad.counts().cpu().numpy()
        img = ad.image(2.2).cpu().numpy()
        assert counts.shape == (len(tor.shard_rows(h, tile, k, count)), w)
        levels = np.unique(counts)
        assert len(levels) >= 2
        for c in levels:
            sel = counts == c
            want = _one_shot(tor, torch, ctx, h, w, int(c), **shard)
            assert np.array_equal(img[sel], want[sel]), f"shard {k}, count {c}"
