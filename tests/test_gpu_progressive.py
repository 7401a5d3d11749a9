"""Progressive rendering on the MI355X: passes of samples added into one buffer give the one-shot TOR_SEED_SAMPLE canvas bit
for bit -- whatever the split, the accel bits, the row shard, the context or the process that rendered a range -- and the
second moments give a reproducible per-pixel noise estimate."""
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


def _one_shot(tor, torch, ctx, h, w, n, accel=0, **opt):
    buf = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    ctx.render_device(tor.camera(), h, w, n, 2.2, DEPTH, tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel, **opt), buf.data_ptr(),
                      _stream(torch))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _accumulate(tor, torch, ctx, h, w, splits, accel=0, moments=False, first=0):
    opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel)
    sums = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    mom = torch.zeros_like(sums) if moments else None
    s = first
    for k in splits:
        ctx.accumulate_device(tor.camera(), h, w, s, k, DEPTH, opt, sums.data_ptr(), mom.data_ptr() if moments else 0, _stream(torch))
        s += k
    torch.cuda.synchronize()
    return sums, mom


def _resolve(ctx, torch, sums, total, gamma=2.2):
    out = torch.empty_like(sums)
    ctx.resolve_device(sums.data_ptr(), sums.numel(), total, gamma, out.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("h,w", [(37, 61), (54, 96)])
def test_split_passes_equal_one_shot(tor, torch, ctx, h, w):
    n = 80
    rng = np.random.default_rng(h * w)
    cuts = np.sort(rng.choice(np.arange(1, n), size=6, replace=False))
    random_split = [int(x) for x in np.diff(np.concatenate(([0], cuts, [n])))]
    splits = [[n], [1] * n, [1, 7, 64, n - 72], random_split]
    for accel in (0, 1, 2, 3):
        want = _one_shot(tor, torch, ctx, h, w, n, accel)
        ref_sums, _ = _accumulate(tor, torch, ctx, h, w, [n], accel)
        ref_sums = ref_sums.cpu().numpy()
        for sp in splits:
            assert sum(sp) == n
            sums, _ = _accumulate(tor, torch, ctx, h, w, sp, accel)
            assert np.array_equal(sums.cpu().numpy(), ref_sums), f"accel {accel}, split {sp}: raw sums differ"
            got = _resolve(ctx, torch, sums, n)
            assert np.array_equal(got, want), f"accel {accel}, split {sp}: {(got != want).sum()} values differ from the one-shot frame"
        # in place: pixels == sums
        sums, _ = _accumulate(tor, torch, ctx, h, w, [3, n - 3], accel)
        ctx.resolve_device(sums.data_ptr(), sums.numel(), n, 2.2, sums.data_ptr(), _stream(torch))
        torch.cuda.synchronize()
        assert np.array_equal(sums.cpu().numpy(), want)


def test_split_passes_match_the_quantised_oracle(tor, torch, ctx, oracle, ref_scene, ref_camera):
    objs, _ = ref_scene
    h, w, n = 1080, 1920, 32
    sums, _ = _accumulate(tor, torch, ctx, h, w, [8, 8, 8, 8])
    got = _resolve(ctx, torch, sums, n)
    assert np.array_equal(got, _one_shot(tor, torch, ctx, h, w, n))
    for r in (0, 731):
        want = oracle.render(h, w, n, ref_camera, objs, seeding=oracle.SEED_SAMPLE, math=1, arith=0, accum=1, rows=(r, r + 1)).pixels[r]
        assert np.array_equal(got[r], want), f"row {r}: {(got[r] != want).sum()} values differ from the oracle"


def test_row_shards_in_passes_assemble_to_one_shot(tor, torch, ctx):
    h, w, n, count, tile = 54, 96, 40, 3, 4
    want = _one_shot(tor, torch, ctx, h, w, n)
    frame = np.full((h, w, 3), -1.0)
    for k in range(count):
        rows = tor.shard_rows(h, tile, k, count)
        opt = tor.make_options(seeding=tor.SEED_SAMPLE, shard_index=k, shard_count=count, row_tile=tile, accel=k)
        sums = torch.zeros((len(rows), w, 3), dtype=torch.float64, device="cuda")
        s = 0
        for m in (5, 11, 24):
            ctx.accumulate_device(tor.camera(), h, w, s, m, DEPTH, opt, sums.data_ptr(), 0, _stream(torch))
            s += m
        torch.cuda.synchronize()
        frame[rows] = _resolve(ctx, torch, sums, n)
    assert np.array_equal(frame, want)


def test_sample_parallel_split_over_two_contexts(tor, torch, ctx, scene):
    h, w, n = 37, 61, 64
    want = _one_shot(tor, torch, ctx, h, w, n)
    other = tor.Context()
    other.upload(scene.list())
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    a = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    b = torch.zeros_like(a)
    for first in range(0, n, 16):  # interleaved ranges: [0,8) [16,24) ... on one context, [8,16) [24,32) ... on the other
        ctx.accumulate_device(tor.camera(), h, w, first, 8, DEPTH, opt, a.data_ptr(), 0, _stream(torch))
        other.accumulate_device(tor.camera(), h, w, first + 8, 8, DEPTH, opt, b.data_ptr(), 0, _stream(torch))
    torch.cuda.synchronize()
    total = a.cpu().numpy() + b.cpu().numpy()  # exact: both are multiples of 2^-36 far below 2^17
    other.close()
    got = _resolve(ctx, torch, torch.from_numpy(total).cuda(), n)
    assert np.array_equal(got, want)


def test_checkpoint_and_resume_in_a_new_context(tor, torch, ctx, scene, tmp_path):
    h, w, n, k = 37, 61, 48, 13
    want = _one_shot(tor, torch, ctx, h, w, n)
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    first = tor.Context()
    first.upload(scene.list())
    pg = tor.Progressive(first, tor.camera(), h, w, DEPTH, opt, moments=True)
    pg.add(k)
    st = pg.state()
    assert st["samples"] == k and st["sums"].shape == (h, w, 3) and st["moments"].shape == (h, w, 3)
    np.savez(tmp_path / "ckpt.npz", sums=st["sums"], moments=st["moments"], samples=st["samples"])
    del pg
    first.close()
    second = tor.Context()
    second.upload(scene.list())
    z = np.load(tmp_path / "ckpt.npz")
    pg = tor.Progressive.from_state(second, tor.camera(), h, w, DEPTH, opt,
                                    {"sums": z["sums"], "moments": z["moments"], "samples": int(z["samples"])})
    pg.add(n - k)
    assert pg.samples == n
    img = pg.image(2.2)
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy(), want)
    cv = pg.to_canvas(tor.new_canvas(h, w, 1, 2.2))
    assert cv.samples_per_pixel == n and np.array_equal(cv.pixels, want)
    # the moments went on where the checkpoint left them: the same as one pass of n samples
    _, mom = _accumulate(tor, torch, second, h, w, [n], moments=True)
    assert np.array_equal(pg.moments.cpu().numpy(), mom.cpu().numpy())
    second.close()


def _numpy_se(S, M, n):
    var = np.maximum(0.0, (M - S * S / n) / (n - 1))
    return np.sqrt(var / n).max(axis=-1)


def test_moments_noise_estimate(tor, torch, ctx):
    h, w, n = 54, 96, 40
    plain, _ = _accumulate(tor, torch, ctx, h, w, [n])
    for accel in (0, 3):
        sums, mom = _accumulate(tor, torch, ctx, h, w, [n], accel, moments=True)
        assert np.array_equal(sums.cpu().numpy(), plain.cpu().numpy()), "asking for moments changed the sums"
        for sp in ([1] * 8 + [32], [17, 23]):
            s2, m2 = _accumulate(tor, torch, ctx, h, w, sp, accel, moments=True)
            assert np.array_equal(s2.cpu().numpy(), sums.cpu().numpy())
            assert np.array_equal(m2.cpu().numpy(), mom.cpu().numpy()), f"split {sp}: moments differ from one pass"
    S, M = sums.cpu().numpy(), mom.cpu().numpy()
    assert np.all(M >= 0.0) and np.all(M <= S + 1e-300)  # q in [0, 1] -> q^2 <= q
    err = torch.full((h * w,), -1.0, dtype=torch.float64, device="cuda")
    mean, mx = ctx.accum_noise_device(sums.data_ptr(), mom.data_ptr(), h * w, n, err.data_ptr(), _stream(torch))
    want = _numpy_se(S, M, n).reshape(-1)
    np.testing.assert_allclose(err.cpu().numpy(), want, rtol=1e-12, atol=0)
    assert mx == float(want.max()) and mx > 0.0  # a max does not depend on the order: exact
    assert mean == pytest.approx(float(want.mean()), rel=1e-12) and 0.0 < mean < mx
    for _ in range(3):  # a fixed reduction order: the same bits every time
        again = ctx.accum_noise_device(sums.data_ptr(), mom.data_ptr(), h * w, n, 0, _stream(torch))
        assert np.array_equal(np.array(again), np.array([mean, mx]))
    # the Progressive helper: the same numbers, and render_until stops on the cap or on the noise target
    pg = tor.Progressive(ctx, tor.camera(), h, w, DEPTH, tor.make_options(seeding=tor.SEED_SAMPLE), moments=True)
    pg.add(n)
    assert pg.noise() == (mean, mx)
    assert pg.render_until(max_se=0.0, max_samples=n + 20, pass_samples=8) == n + 20
    pg2 = tor.Progressive(ctx, tor.camera(), h, w, DEPTH, tor.make_options(seeding=tor.SEED_SAMPLE), moments=True)
    assert pg2.render_until(max_se=1.0, max_samples=1000, pass_samples=8) == 8


def test_rejections_and_edges(tor, torch, ctx):
    h, w = 37, 61
    cam = tor.camera()
    sums = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    with pytest.raises(tor.TorError) as e:
        ctx.accumulate_device(cam, h, w, 0, 4, DEPTH, tor.make_options(seeding=tor.SEED_PIXEL), sums.data_ptr())
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "SEED_PIXEL" in str(e.value) and "RNG state" in str(e.value)
    for first, n in ((-1, 4), (0, 0), ((1 << 17) - 3, 4), (5, 1 << 17)):
        with pytest.raises(tor.TorError) as e:
            ctx.accumulate_device(cam, h, w, first, n, DEPTH, opt, sums.data_ptr())
        assert e.value.code == tor.ERR_INVALID_ARGUMENT and "2^17" in str(e.value)
    ctx.accumulate_device(cam, h, w, (1 << 17) - 1, 1, DEPTH, opt, sums.data_ptr(), 0, _stream(torch))  # the last sample there is
    mom = torch.zeros_like(sums)
    with pytest.raises(tor.TorError) as e:
        ctx.accum_noise_device(sums.data_ptr(), mom.data_ptr(), h * w, 1)
    assert e.value.code == tor.ERR_INVALID_ARGUMENT
    # max_depth 0: every sample is black, the buffers keep what they hold
    torch.cuda.synchronize()
    sums.fill_(0.25)
    mom.fill_(0.125)
    ctx.accumulate_device(cam, h, w, 0, 16, 0, opt, sums.data_ptr(), mom.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    assert bool((sums == 0.25).all()) and bool((mom == 0.125).all())
