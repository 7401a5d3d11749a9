"""Resumable rendering on the reference's per-pixel streams (tor_render_resume_device, PixelProgressive) on the MI355X.  Every
comparison is exact (np.array_equal on float64 / uint64 bit patterns, every pixel, every channel).  The arbiter is the CPU oracle in
the arithmetic the GPU is held to (SEED_PIXEL / MATH_PORTABLE / ACCUM_SEQUENTIAL): the first k samples of a pixel do not depend on spp,
so the oracle's k-spp canvas is what a resumed render must show after k samples.  A second, independent GPU path -- the query entries,
seed2 then camera_rays(SEED_PIXEL) + radiance per sample -- checks the per-pixel generator states, raw sums and moments."""
import ctypes as C

import numpy as np
import pytest
import torch

import hit_restatement as H
from output_restatement import noise as _numpy_noise      # tor_accum_noise_device restated, in the kernels' fixed order

pytestmark = pytest.mark.gpu

N = 32
SPLITS = ((N,), (1, N - 1), (3, 5, 24), (1,) * 8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cam24(cam):
    return np.frombuffer(bytes(cam), dtype=np.float64).copy()


def _ctx(tor, recs):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    return ctx


@pytest.fixture(scope="module")
def cases(tor):
    """(name, object records, camera, rows, columns, max_depth): random_scene at depth 50, movers in several time groups at a small depth"""
    mover_cam = tor.camera(look_from=(0, 6, 18), look_at=(0, 1, 0), vertical_field_of_view=50.0, shutter_open=-0.5, shutter_close=2.0)
    return (("random_scene", tor.random_scene(0xFACADE).to_records(), tor.camera(), 24, 32, 50),
            ("time groups", H.group_scene(5, 300), mover_cam, 36, 64, 3))


class _Oracle:
    """the reference's k-spp canvas, rendered once per k"""

    def __init__(self, oracle, recs, cam, h, w, depth):
        self.o, self.recs, self.cam, self.h, self.w, self.depth, self.seen = oracle, recs, _cam24(cam), h, w, depth, {}

    def at(self, k):
        if k not in self.seen:
            self.seen[k] = self.o.render(self.h, self.w, k, self.cam, self.recs, max_depth=self.depth, seeding=self.o.SEED_PIXEL,
                                         math=self.o.MATH_PORTABLE, accum=self.o.ACCUM_SEQUENTIAL).pixels
        return self.seen[k]


def _walk(tor, ctx, cam, h, w, pix, k, depth):
    """k samples of the listed pixels through the query entries: (states, sequential sums, sequential sums of c * c)"""
    pix = np.asarray(pix, dtype=np.int32)
    st = torch.from_numpy(tor.rng_seed2(pix // w, pix % w).view(np.int64)).cuda()
    dpix = torch.from_numpy(pix).cuda()
    s = np.zeros((pix.size, 3))
    m = np.zeros((pix.size, 3))
    for _ in range(k):
        rays, st = ctx.camera_rays(cam, h, w, 0, 1, tor.SEED_PIXEL, dpix, st)
        color, st, _ = ctx.radiance(rays, st, depth)
        torch.cuda.synchronize()
        c = color.cpu().numpy().reshape(-1, 3)
        s = s + c
        m = m + c * c
    return st.cpu().numpy().view(np.uint64).reshape(-1, 4), s, m


def test_splits_equal_the_oracle(tor, oracle, cases):
    for name, recs, cam, h, w, depth in cases:
        ctx = _ctx(tor, recs)
        want = _Oracle(oracle, recs, cam, h, w, depth)
        sums_ref = None
        for accel in (0, 3):
            for pk in (tor.PIXEL_KERNEL_LANE, tor.PIXEL_KERNEL_WAVE, tor.PIXEL_KERNEL_AUTO):
                opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=accel, pixel_kernel=pk)
                one = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
                ctx.render_device(cam, h, w, N, 2.2, depth, opt, one.data_ptr(), _stream())
                torch.cuda.synchronize()
                assert _same(one.cpu().numpy(), want.at(N)), (name, accel, pk)
                for split in SPLITS:
                    pp = tor.PixelProgressive(ctx, cam, h, w, depth, opt)
                    # (nothing needs clearing: a pass with first_sample == 0 reads none of the buffers)
                    pp.sums.fill_(float("nan")); pp.rng.fill_(-1)
                    for k in split:
                        pp.add(k)
                        got = pp.image().cpu().numpy()
                        assert _same(got, want.at(pp.samples)), (name, accel, pk, split, pp.samples, int((_bits(got) != _bits(want.at(pp.samples))).sum()))
                    if sum(split) == N:
                        raw = pp.sums.cpu().numpy()
                        sums_ref = raw if sums_ref is None else sums_ref
                        assert _same(raw, sums_ref), (name, accel, pk, split)
                        assert _same(pp.image().cpu().numpy(), one.cpu().numpy())
        ctx.close()


def test_kernel_choice_is_what_the_header_says(tor, cases):
    """LANE: integrate_kernel variant 5 (6 with moments); WAVE and AUTO on a small frame: the wave-per-pixel kernel, which leaves
    tor_debug_last_variant as it was (-1 on a fresh context)."""
    _, recs, cam, h, w, depth = cases[0]
    for pk, moments, want in ((tor.PIXEL_KERNEL_WAVE, False, -1), (tor.PIXEL_KERNEL_AUTO, True, -1), (tor.PIXEL_KERNEL_LANE, False, 5),
                              (tor.PIXEL_KERNEL_LANE, True, 6)):
        ctx = _ctx(tor, recs)
        pp = tor.PixelProgressive(ctx, cam, h, w, depth, tor.make_options(seeding=tor.SEED_PIXEL, accel=3, pixel_kernel=pk), moments=moments)
        pp.add(4).add(4)
        torch.cuda.synchronize()
        assert ctx.last_variant()[0] == want, (pk, moments, ctx.last_variant())
        assert ctx.handoff_stalled() == (False, 0)
        ctx.close()


def test_state_equals_an_independent_walk(tor, cases):
    for name, recs, cam, h, w, depth in cases:
        ctx = _ctx(tor, recs)
        pix = np.array([0, 1, w - 1, w, (h // 2) * w + w // 2, (h // 2) * w + w // 3, h * w - 2, h * w - 1], dtype=np.int32)
        k = 5
        want_st, want_s, want_m = _walk(tor, ctx, cam, h, w, pix, k, depth)
        for accel, pk in ((3, tor.PIXEL_KERNEL_LANE), (0, tor.PIXEL_KERNEL_LANE), (3, tor.PIXEL_KERNEL_WAVE), (3, tor.PIXEL_KERNEL_AUTO)):
            pp = tor.PixelProgressive(ctx, cam, h, w, depth, tor.make_options(seeding=tor.SEED_PIXEL, accel=accel, pixel_kernel=pk), moments=True)
            pp.add(2).add(3)
            torch.cuda.synchronize()
            st = pp.state()
            assert st["rng"].dtype == np.uint64 and st["rng"].shape == (h, w, 4)
            assert np.array_equal(st["rng"].reshape(-1, 4)[pix], want_st), (name, accel, pk)
            assert _same(st["sums"].reshape(-1, 3)[pix], want_s), (name, accel, pk)
            assert _same(st["moments"].reshape(-1, 3)[pix], want_m), (name, accel, pk)
        ctx.close()


def test_draws_are_never_skipped(tor, oracle, cases):
    """An empty scene and max_depth = 0: the reference still draws the pixel jitter, the lens and the time sample of every sample."""
    _, recs, cam, h, w, _ = cases[0]
    pix = np.array([0, 5, w + 3, h * w - 1], dtype=np.int32)
    for what, objs, depth in (("empty scene", np.zeros((0, 16)), 50), ("max_depth 0", recs, 0)):
        ctx = _ctx(tor, objs)
        want = _Oracle(oracle, objs, cam, h, w, depth)
        want_st, want_s, want_m = _walk(tor, ctx, cam, h, w, pix, 8, depth)
        seeds = tor.rng_seed2(pix // w, pix % w)
        assert not np.array_equal(want_st, seeds)
        for accel, pk in ((0, tor.PIXEL_KERNEL_LANE), (3, tor.PIXEL_KERNEL_LANE), (3, tor.PIXEL_KERNEL_WAVE), (3, tor.PIXEL_KERNEL_AUTO)):
            pp = tor.PixelProgressive(ctx, cam, h, w, depth, tor.make_options(seeding=tor.SEED_PIXEL, accel=accel, pixel_kernel=pk), moments=True)
            pp.add(3)
            assert _same(pp.image().cpu().numpy(), want.at(3)), (what, accel, pk)
            pp.add(5)
            assert _same(pp.image().cpu().numpy(), want.at(8)), (what, accel, pk)
            st = pp.state()
            assert np.array_equal(st["rng"].reshape(-1, 4)[pix], want_st), (what, accel, pk)
            assert _same(st["sums"].reshape(-1, 3)[pix], want_s) and _same(st["moments"].reshape(-1, 3)[pix], want_m), (what, accel, pk)
        if depth == 0:
            assert not want.at(8).any()
        else:
            assert want.at(8).min() > 0.0  # the sky
        ctx.close()


@pytest.mark.timeout(600)
def test_the_kernels_auto_picks_on_a_mid_size_frame(tor):
    """540 x 960, 64 spp, both exact accelerations: tor_render_device hands chains off here; a resume pass never does (tor_render.h) --
    AUTO runs the cost probe and the lane kernel's resume variant (the frame's most expensive tiles go to the wave-per-pixel resume
    kernel at the same time), and the two passes of 32 give the one-shot canvas."""
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    h, w = 540, 960
    opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=3)
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    one = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    ctx.render_device(cam, h, w, 64, 2.2, 50, opt, one.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert ctx.handoff_stalled() == (False, 0)
    assert ctx.last_variant()[0] == 0 and ctx.last_split_tiles() == 0   # (the one-shot frame runs the hand-off, not the split)
    for moments, seeding in ((False, 5), (True, 6)):
        pp = tor.PixelProgressive(ctx, cam, h, w, 50, opt, moments=moments)
        pp.add(32)
        torch.cuda.synchronize()
        assert ctx.last_variant() == (seeding, 0, ctx.last_variant()[2], 1, 1)
        assert ctx.last_pixel_cost(h * w).size == h * w      # the cost probe ran
        assert 0 < ctx.last_split_tiles() < (h * w + 63) // 64   # the frame was shared: these tiles went to coop_pixel_resume_kernel
        hc = ctx.last_handoff_counters()
        assert hc["pushed"] == 0 and hc["served"] == 0       # ... and nothing was handed over
        pp.add(32)   # (first_sample > 0 under the split: the wave kernel's pixels come from the tile order)
        torch.cuda.synchronize()
        assert ctx.last_split_tiles() > 0
        assert ctx.handoff_stalled() == (False, 0)
        assert torch.equal(pp.image(), one), int((pp.image() != one).sum().item())
    ctx.close()


def test_row_shards(tor, cases):
    _, recs, cam, h, w, depth = cases[0]
    ctx = _ctx(tor, recs)
    whole = tor.PixelProgressive(ctx, cam, h, w, depth, moments=True)
    whole.add(3).add(5)
    torch.cuda.synchronize()
    ws = whole.state()
    for pk in (tor.PIXEL_KERNEL_AUTO, tor.PIXEL_KERNEL_LANE, tor.PIXEL_KERNEL_WAVE):
        for k in range(3):
            rows = tor.shard_rows(h, 2, k, 3)
            pp = tor.PixelProgressive(ctx, cam, h, w, depth, tor.make_options(seeding=tor.SEED_PIXEL, accel=3, shard_index=k, shard_count=3, row_tile=2,
                                                                              pixel_kernel=pk), moments=True)
            pp.add(3).add(5)
            torch.cuda.synchronize()
            st = pp.state()
            assert st["rng"].shape == (len(rows), w, 4)
            assert np.array_equal(st["rng"], ws["rng"][rows]) and _same(st["sums"], ws["sums"][rows]) and _same(st["moments"], ws["moments"][rows]), (pk, k)
            assert torch.equal(pp.image().cpu(), whole.image().cpu()[torch.from_numpy(np.asarray(rows, dtype=np.int64))])
    ctx.close()


def test_checkpoint(tor, cases):
    _, recs, cam, h, w, depth = cases[0]
    ctx = _ctx(tor, recs)
    opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=3)
    full = tor.PixelProgressive(ctx, cam, h, w, depth, opt, moments=True).add(32)
    plain = tor.PixelProgressive(ctx, cam, h, w, depth, opt, moments=False).add(32)
    first = tor.PixelProgressive(ctx, cam, h, w, depth, opt, moments=True).add(8)
    torch.cuda.synchronize()
    saved = first.state()
    assert saved["samples"] == 8
    other = _ctx(tor, recs)
    again = tor.PixelProgressive.from_state(other, cam, h, w, depth, opt, saved).add(24)
    torch.cuda.synchronize()
    a, f, p = again.state(), full.state(), plain.state()
    assert a["samples"] == 32
    for key in ("rng", "sums", "moments"):
        assert _same(a[key], f[key]), key
    assert p["moments"] is None and _same(p["sums"], f["sums"]) and np.array_equal(p["rng"], f["rng"])
    assert torch.equal(again.image().cpu(), full.image().cpu())
    other.close()
    ctx.close()


def test_noise(tor, cases):
    _, recs, cam, h, w, depth = cases[0]
    ctx = _ctx(tor, recs)
    pp = tor.PixelProgressive(ctx, cam, h, w, depth, moments=True)
    pp.add(8).add(12)
    torch.cuda.synchronize()
    st = pp.state()
    e, mean, mx = _numpy_noise(st["sums"], st["moments"], 20)
    err = torch.full((h * w,), -1.0, dtype=torch.float64, device="cuda")
    got = ctx.accum_noise_device(pp.sums.data_ptr(), pp.moments.data_ptr(), h * w, 20, err.data_ptr(), _stream())
    assert _same(err.cpu().numpy(), e)
    assert pp.noise() == got == (mean, mx) and 0.0 < mean < mx
    assert pp.render_until(max_se=0.0, max_samples=45, pass_samples=8) == 45 and pp.samples == 45
    pp2 = tor.PixelProgressive(ctx, cam, h, w, depth, moments=True)
    assert pp2.render_until(max_se=1.0, max_samples=1000, pass_samples=8) == 8
    with pytest.raises(tor.TorError):
        tor.PixelProgressive(ctx, cam, h, w, depth).noise()
    ctx.close()


def test_rejections_write_nothing(tor, cases):
    _, recs, cam, h, w, depth = cases[0]
    ctx = _ctx(tor, recs)
    L = tor.lib()
    rng = torch.full((h, w, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    sums = torch.full((h, w, 3), -7.25, dtype=torch.float64, device="cuda")
    mom = torch.full((h, w, 3), -9.5, dtype=torch.float64, device="cuda")
    pix = tor.make_options(seeding=tor.SEED_PIXEL, accel=3)
    smp = tor.make_options(seeding=tor.SEED_SAMPLE, accel=3)
    bare = tor.Context(0)  # no scene uploaded

    def call(c=ctx, opt=pix, rows=h, cols=w, first=0, n=4, r=rng.data_ptr(), s=sums.data_ptr()):
        return L.tor_render_resume_device(c._h, C.byref(cam), rows, cols, first, n, depth, C.byref(opt), C.c_void_p(r), C.c_void_p(s),
                                          C.c_void_p(mom.data_ptr()), C.c_void_p(_stream()))

    bad = (("SEED_SAMPLE", dict(opt=smp), "tor_render_accumulate_device"), ("first < 0", dict(first=-1), "2^17"), ("n < 1", dict(n=0), "2^17"),
           ("beyond 2^17", dict(first=(1 << 17) - 3, n=4), "2^17"), ("NULL d_rng", dict(r=0), "NULL"), ("NULL d_sums", dict(s=0), "NULL"),
           ("one row", dict(rows=1), "nrows >= 2"), ("one column", dict(cols=1), "ncols >= 2"), ("no scene", dict(c=bare), "no scene"))
    for what, kw, word in bad:
        assert call(**kw) == tor.ERR_INVALID_ARGUMENT, what
        msg = L.tor_last_error().decode()
        assert word in msg and "tor_render_resume_device" in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((rng == 0x5A5A5A5A).all()) and bool((sums == -7.25).all()) and bool((mom == -9.5).all())
    with pytest.raises(tor.TorError) as e:
        tor.PixelProgressive(ctx, cam, h, w, depth, smp)
    assert "Progressive" in str(e.value)
    # the sample-stream entries keep refusing the pixel streams
    with pytest.raises(tor.TorError) as e:
        ctx.accumulate_device(cam, h, w, 0, 4, depth, pix, sums.data_ptr(), 0, _stream())
    assert "per-pixel RNG state" in str(e.value)
    assert call(first=(1 << 17) - 1, n=1, rows=2, cols=2) == tor.OK  # the last sample there is
    torch.cuda.synchronize()
    bare.close()
    ctx.close()


def test_one_stream_per_context_is_enforced_before_any_state_moves(tor):
    """The one-stream-per-context rule of the other render entries: a resume pass on a second stream while the context's previous
    launch is still running is refused -- with first_sample > 0, and with nothing written to the state it would have advanced in
    place -- and the same call on the first stream is accepted."""
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    h, w = 540, 960
    opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=0, pixel_kernel=tor.PIXEL_KERNEL_LANE)
    big = tor.PixelProgressive(ctx, cam, h, w, 50, opt, moments=True)
    small = tor.PixelProgressive(ctx, cam, 24, 32, 50, opt, moments=True)
    with torch.cuda.stream(s1):
        small.add(4)
    torch.cuda.synchronize()
    before = small.state()
    rng = torch.full((24, 32, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    sums = torch.full((24, 32, 3), -7.25, dtype=torch.float64, device="cuda")
    mom = torch.full((24, 32, 3), -9.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        big.add(600)                                   # ~150 ms of float64 brute force on s1
    with pytest.raises(tor.TorError) as e:
        ctx.resume_device(cam, 24, 32, 4, 4, 50, opt, rng.data_ptr(), sums.data_ptr(), mom.data_ptr(), s2.cuda_stream)
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "ONE stream" in str(e.value) and "tor_render_resume_device" in str(e.value)
    with pytest.raises(tor.TorError) as e:             # ... and a real state is left where it was
        ctx.resume_device(cam, 24, 32, 4, 4, 50, opt, small.rng.data_ptr(), small.sums.data_ptr(), small.moments.data_ptr(), s2.cuda_stream)
    assert "ONE stream" in str(e.value)
    with torch.cuda.stream(s1):
        small.add(4)                                   # the same stream may queue
    torch.cuda.synchronize()
    assert bool((rng == 0x5A5A5A5A).all()) and bool((sums == -7.25).all()) and bool((mom == -9.5).all())
    # the accepted pass continued from the state the refused one did not touch: 4 + 4 equals 8 in one
    ref = tor.PixelProgressive(ctx, cam, 24, 32, 50, opt, moments=True)
    with torch.cuda.stream(s2):
        ref.add(8)                                     # idle context: any stream
    torch.cuda.synchronize()
    a, r = small.state(), ref.state()
    assert a["samples"] == 8 and not np.array_equal(a["rng"], before["rng"])
    for key in ("rng", "sums", "moments"):
        assert _same(a[key], r[key]), key
    ctx.close()
