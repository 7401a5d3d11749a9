"""Adaptive sampling on the reference's per-pixel streams (tor_render_resume_list_device, PixelAdaptive) on the MI355X.  Every
comparison is exact (bit patterns of float64 / uint64, every pixel, every channel).  The arbiter is the CPU oracle in the arithmetic the
GPU is held to (SEED_PIXEL / MATH_PORTABLE / ACCUM_SEQUENTIAL): pixel p of an adaptive frame must be the oracle's pixel p at counts[p]
samples per pixel.  Two more witnesses check the state itself: a PixelProgressive advanced uniformly (schedule independence) and the
query entries -- seed2, then camera_rays(SEED_PIXEL) + radiance per sample (an independent walk).

The policy of the runs (rel_tol 0.15, passes of 8, at most 40 samples) was chosen from the CPU oracle alone so that the counts spread:
replaying the select on the oracle's 1 .. 40-spp canvases gives, on random_scene 24 x 32, {8: 279, 16: 83, 24: 88, 32: 62, 40: 256} pixels
and, on the time-group movers 36 x 64, {8: 1260, 16: 477, 24: 213, 32: 99, 40: 255} -- five distinct k for the oracle to render."""
import ctypes as C

import numpy as np
import pytest
import torch

import hit_restatement as H

pytestmark = pytest.mark.gpu

POLICY = dict(rel_tol=0.15, min_samples=8, pass_samples=8, max_samples=40)


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


def _kernels(tor):
    return (tor.PIXEL_KERNEL_LANE, tor.PIXEL_KERNEL_WAVE, tor.PIXEL_KERNEL_AUTO)


def _opt(tor, accel, pk, **kw):
    return tor.make_options(seeding=tor.SEED_PIXEL, accel=accel, pixel_kernel=pk, **kw)


@pytest.fixture(scope="module")
def cases(tor):
    """(name, object records, camera, rows, columns, max_depth): random_scene at depth 50, movers in several time groups at a small depth
    (the two scenes of test_gpu_resume.py)"""
    mover_cam = tor.camera(look_from=(0, 6, 18), look_at=(0, 1, 0), vertical_field_of_view=50.0, shutter_open=-0.5, shutter_close=2.0)
    return (("random_scene", tor.random_scene(0xFACADE).to_records(), tor.camera(), 24, 32, 50),
            ("time groups", H.group_scene(5, 300), mover_cam, 36, 64, 3))


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


def _uniform_snapshots(tor, ctx, cam, h, w, depth, step, top):
    """{k: state of a PixelProgressive(moments=True) after k samples} for every multiple k of step up to top"""
    pp = tor.PixelProgressive(ctx, cam, h, w, depth, moments=True)
    snaps = {}
    while pp.samples < top:
        pp.add(step)
        torch.cuda.synchronize()
        snaps[pp.samples] = pp.state()
    return snaps


def test_oracle_schedule_and_select(tor, oracle, cases):
    """Items 1, 2 and 5: per count k the pixels equal the oracle's k-spp canvas; every pixel's state, sums and moments equal a uniform
    PixelProgressive's at counts[p]; the active list after every step is adaptive_select_host's on the downloaded sums and moments."""
    for name, recs, cam, h, w, depth in cases:
        ctx = _ctx(tor, recs)
        snaps = _uniform_snapshots(tor, ctx, cam, h, w, depth, POLICY["pass_samples"], POLICY["max_samples"])
        want = {}
        ref_counts = None
        for accel in (0, 3):
            for pk in _kernels(tor):
                tag = (name, accel, pk)
                ad = tor.PixelAdaptive(ctx, cam, h, w, depth, _opt(tor, accel, pk), **POLICY)
                # (nothing needs clearing: the first pass reads none of the buffers)
                ad.sums.fill_(float("nan")); ad.moments.fill_(float("nan")); ad.rng.fill_(-1)
                while ad.active > 0 and ad.samples < ad.max_samples:
                    before = ad.active_list().cpu().numpy()
                    ad.step()
                    torch.cuda.synchronize()
                    keep = tor.adaptive_select_host(ad.sums.cpu().numpy(), ad.moments.cpu().numpy(), before, ad.samples, ad.abs_tol, ad.rel_tol)
                    got = ad.active_list().cpu().numpy()
                    assert got.dtype == np.int32 and np.array_equal(got, keep), tag + (ad.samples,)
                st = ad.state()
                counts = st["counts"]
                ks, n_of = np.unique(counts, return_counts=True)
                print(name, accel, pk, dict(zip(ks.tolist(), n_of.tolist())), "samples", ad.total_samples())
                # not vacuous: the counts spread, some pixels stopped at once, some ran to the end
                assert len(ks) >= 3 and len(ks) <= 6, tag + (ks,)
                assert ks[0] == POLICY["min_samples"] and ks[-1] == POLICY["max_samples"], tag + (ks,)
                assert ad.total_samples() == int(counts.astype(np.int64).sum()) < h * w * POLICY["max_samples"]
                if ref_counts is None:
                    ref_counts = counts
                assert np.array_equal(counts, ref_counts), tag   # the same bits decide the same way under every kernel
                img = ad.image().cpu().numpy()
                for k in ks.tolist():
                    if k not in want:
                        want[k] = oracle.render(h, w, k, _cam24(cam), recs, max_depth=depth, seeding=oracle.SEED_PIXEL,
                                                math=oracle.MATH_PORTABLE, accum=oracle.ACCUM_SEQUENTIAL).pixels
                    at = counts == k
                    assert _same(img[at], want[k][at]), tag + (k, int((_bits(img[at]) != _bits(want[k][at])).sum()))
                    for key in ("rng", "sums", "moments"):
                        assert _same(st[key][at], snaps[k][key][at]), tag + (k, key)
        ctx.close()


def test_state_equals_an_independent_walk(tor, cases):
    """Item 3: a handful of pixels with different counts, against seed2 + camera_rays + radiance per sample."""
    for name, recs, cam, h, w, depth in cases:
        ctx = _ctx(tor, recs)
        for accel, pk in ((3, tor.PIXEL_KERNEL_LANE), (0, tor.PIXEL_KERNEL_WAVE), (3, tor.PIXEL_KERNEL_AUTO)):
            ad = tor.PixelAdaptive(ctx, cam, h, w, depth, _opt(tor, accel, pk), **POLICY)
            ad.run()
            torch.cuda.synchronize()
            st = ad.state()
            counts = st["counts"].reshape(-1)
            ks = np.unique(counts)
            assert len(ks) >= 3
            for k in ks.tolist():
                at = np.flatnonzero(counts == k)
                pix = at[[0, len(at) // 2, len(at) - 1]].astype(np.int32)
                want_st, want_s, want_m = _walk(tor, ctx, cam, h, w, pix, k, depth)
                assert np.array_equal(st["rng"].reshape(-1, 4)[pix], want_st), (name, accel, pk, k)
                assert _same(st["sums"].reshape(-1, 3)[pix], want_s), (name, accel, pk, k)
                assert _same(st["moments"].reshape(-1, 3)[pix], want_m), (name, accel, pk, k)
        ctx.close()


def test_unlisted_pixels_keep_every_bit(tor, cases):
    """Item 4: sentinels in all three buffers; a start over every third pixel, then a continued pass over a sub-list; entries outside
    the shard (and negative ones) write nothing."""
    RNG, SUM, MOM = 0x5A5A5A5A5A5A5A5A, -7.25, -9.5
    for name, recs, cam, h, w, depth in cases:
        ctx = _ctx(tor, recs)
        npix = h * w
        snaps = _uniform_snapshots(tor, ctx, cam, h, w, depth, 3, 6)
        third = np.arange(0, npix, 3, dtype=np.int32)
        sub = third[1::2].copy()
        for accel in (0, 3):
            for pk in _kernels(tor):
                tag = (name, accel, pk)
                opt = _opt(tor, accel, pk)
                rng = torch.full((h, w, 4), RNG, dtype=torch.int64, device="cuda")
                sums = torch.full((h, w, 3), SUM, dtype=torch.float64, device="cuda")
                mom = torch.full((h, w, 3), MOM, dtype=torch.float64, device="cuda")

                def run(lst, first, n):
                    d = torch.from_numpy(np.asarray(lst, dtype=np.int32)).cuda()
                    ctx.resume_list_device(cam, h, w, d.data_ptr(), d.numel(), first, n, depth, opt, rng.data_ptr(), sums.data_ptr(),
                                           mom.data_ptr(), _stream())
                    torch.cuda.synchronize()
                    return rng.cpu().numpy().view(np.uint64).reshape(-1, 4), sums.cpu().numpy().reshape(-1, 3), mom.cpu().numpy().reshape(-1, 3)

                r, s, m = run(third, 0, 3)
                rest = np.setdiff1d(np.arange(npix), third)
                assert (r[rest] == np.uint64(RNG)).all() and (s[rest] == SUM).all() and (m[rest] == MOM).all(), tag
                for got, key in ((r, "rng"), (s, "sums"), (m, "moments")):
                    assert _same(got[third], snaps[3][key].reshape(npix, -1)[third]), tag + (key,)
                # a continued pass over a sub-list, with entries outside the shard in it (ascending: they come last; and one below 0)
                lst = np.concatenate(([-1], sub, [npix, npix + 7, 1 << 30])).astype(np.int32)
                r2, s2, m2 = run(lst, 3, 3)
                others = np.setdiff1d(np.arange(npix), sub)
                assert np.array_equal(r2[others], r[others]) and _same(s2[others], s[others]) and _same(m2[others], m[others]), tag
                for got, key in ((r2, "rng"), (s2, "sums"), (m2, "moments")):
                    assert _same(got[sub], snaps[6][key].reshape(npix, -1)[sub]), tag + (key,)
                # an empty list is a no-op, with or without a pointer
                ctx.resume_list_device(cam, h, w, 0, 0, 6, 3, depth, opt, rng.data_ptr(), sums.data_ptr(), mom.data_ptr(), _stream())
                r3, s3, m3 = run(np.zeros(0, dtype=np.int32), 6, 3)
                assert np.array_equal(r3, r2) and _same(s3, s2) and _same(m3, m2), tag
        ctx.close()


def test_row_shards(tor, cases):
    """Item 6: two row shards with shard-local lists reproduce the unsharded per-pixel results."""
    for name, recs, cam, h, w, depth in cases:
        ctx = _ctx(tor, recs)
        whole = tor.PixelAdaptive(ctx, cam, h, w, depth, **POLICY)
        whole.run()
        torch.cuda.synchronize()
        ws, wimg = whole.state(), whole.image().cpu().numpy()
        for pk in _kernels(tor):
            for k in range(2):
                rows = np.asarray(tor.shard_rows(h, 4, k, 2), dtype=np.int64)
                ad = tor.PixelAdaptive(ctx, cam, h, w, depth, _opt(tor, 3, pk, shard_index=k, shard_count=2, row_tile=4), **POLICY)
                ad.run()
                torch.cuda.synchronize()
                st = ad.state()
                assert st["rng"].shape == (len(rows), w, 4) and st["counts"].shape == (len(rows), w)
                assert np.array_equal(st["counts"], ws["counts"][rows]), (name, pk, k)
                for key in ("rng", "sums", "moments"):
                    assert _same(st[key], ws[key][rows]), (name, pk, k, key)
                assert _same(ad.image().cpu().numpy(), wimg[rows]), (name, pk, k)
        ctx.close()


def test_kernel_choice_is_what_the_header_says(tor, cases):
    """Item 7: LANE is integrate_kernel variant 7; WAVE and AUTO on these small lists run the wave-per-pixel kernel, which leaves
    tor_debug_last_variant as it was (-1 on a fresh context); no hand-off, no split."""
    _, recs, cam, h, w, depth = cases[0]
    for pk, want in ((tor.PIXEL_KERNEL_WAVE, -1), (tor.PIXEL_KERNEL_AUTO, -1), (tor.PIXEL_KERNEL_LANE, 7)):
        for accel in (0, 3):
            ctx = _ctx(tor, recs)
            ad = tor.PixelAdaptive(ctx, cam, h, w, depth, _opt(tor, accel, pk), **POLICY)
            ad.step().step()
            torch.cuda.synchronize()
            assert 0 < ad.active < h * w
            assert ctx.last_variant()[0] == want, (pk, accel, ctx.last_variant())
            if want == 7:
                assert ctx.last_variant()[3:] == ((1, 1) if accel else (0, 0))
            assert ctx.handoff_stalled() == (False, 0)
            assert ctx.last_split_tiles() == 0
            # tor_last_kernel_ms reports the listed pass: its list was the pixels the first select kept, the ones now above 8 samples
            ms, samples = ctx.last_kernel_ms()
            listed = int((ad.counts() > ad.pass_samples).sum().item())
            assert ms > 0.0 and samples == listed * ad.pass_samples, (pk, accel, ms, samples, listed)
            ctx.close()


def test_a_second_stream_is_refused_before_any_state_moves(tor):
    """Item 7, the launch rule: a listed pass on a second stream while the context's previous launch is still running is refused and
    changes nothing; the same call on the first stream is accepted."""
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=0, pixel_kernel=tor.PIXEL_KERNEL_LANE)
    big = tor.PixelProgressive(ctx, cam, 540, 960, 50, opt, moments=True)
    small = tor.PixelAdaptive(ctx, cam, 24, 32, 50, opt, rel_tol=0.0, min_samples=4, pass_samples=4, max_samples=64)
    with torch.cuda.stream(s1):
        small.step()
    torch.cuda.synchronize()
    before = small.state()
    lst = torch.arange(0, 24 * 32, 2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        big.add(2000)                                  # ~0.5 s of float64 brute force on s1
        busy = torch.cuda.Event()
        busy.record(s1)
    with pytest.raises(tor.TorError) as e:
        ctx.resume_list_device(cam, 24, 32, lst.data_ptr(), lst.numel(), 4, 4, 50, opt, small.rng.data_ptr(), small.sums.data_ptr(),
                               small.moments.data_ptr(), s2.cuda_stream)
    assert not busy.query()                            # the refusal was made while s1's launch was still in flight, not after it
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "ONE stream" in str(e.value) and "tor_render_resume_list_device" in str(e.value)
    torch.cuda.synchronize()
    after = small.state()
    for key in ("rng", "sums", "moments"):
        assert _same(after[key], before[key]), key
    assert np.array_equal(after["counts"], before["counts"]) and np.array_equal(after["list"], before["list"])
    with torch.cuda.stream(s1):
        small.step()                                   # the same stream may queue
    torch.cuda.synchronize()
    ref = tor.PixelProgressive(ctx, cam, 24, 32, 50, opt, moments=True).add(8)
    torch.cuda.synchronize()
    a, r = small.state(), ref.state()
    on = a["counts"] == 8
    assert a["samples"] == 8 and on.any()
    for key in ("rng", "sums", "moments"):
        assert _same(a[key][on], r[key][on]), key
    ctx.close()


def test_draws_are_never_skipped(tor, cases):
    """Item 8: max_depth = 0 and an empty scene still advance the listed states exactly as tor_render_resume_device does over the
    same pixels."""
    _, recs, cam, h, w, _ = cases[0]
    npix = h * w
    lst = np.arange(1, npix, 5, dtype=np.int32)
    for what, objs, depth in (("empty scene", np.zeros((0, 16)), 50), ("max_depth 0", recs, 0)):
        ctx = _ctx(tor, objs)
        snaps = _uniform_snapshots(tor, ctx, cam, h, w, depth, 3, 6)
        seeds = tor.rng_seed2(lst // w, lst % w)
        assert not np.array_equal(snaps[3]["rng"].reshape(-1, 4)[lst], seeds)
        for accel in (0, 3):
            for pk in _kernels(tor):
                opt = _opt(tor, accel, pk)
                rng = torch.zeros((h, w, 4), dtype=torch.int64, device="cuda")
                sums = torch.full((h, w, 3), -1.0, dtype=torch.float64, device="cuda")
                mom = torch.full((h, w, 3), -1.0, dtype=torch.float64, device="cuda")
                d = torch.from_numpy(lst).cuda()
                for first in (0, 3):
                    ctx.resume_list_device(cam, h, w, d.data_ptr(), d.numel(), first, 3, depth, opt, rng.data_ptr(), sums.data_ptr(),
                                           mom.data_ptr(), _stream())
                    torch.cuda.synchronize()
                    want = snaps[first + 3]
                    assert np.array_equal(rng.cpu().numpy().view(np.uint64).reshape(-1, 4)[lst], want["rng"].reshape(-1, 4)[lst]), (what, accel, pk, first)
                    assert _same(sums.cpu().numpy().reshape(-1, 3)[lst], want["sums"].reshape(-1, 3)[lst]), (what, accel, pk, first)
                    assert _same(mom.cpu().numpy().reshape(-1, 3)[lst], want["moments"].reshape(-1, 3)[lst]), (what, accel, pk, first)
                rest = np.setdiff1d(np.arange(npix), lst)
                assert not rng.cpu().numpy().reshape(-1, 4)[rest].any() and (sums.cpu().numpy().reshape(-1, 3)[rest] == -1.0).all()
        if depth == 0:
            assert not snaps[6]["sums"].any()
        else:
            assert snaps[6]["sums"].min() > 0.0  # the sky
        ctx.close()


def test_checkpoint(tor, cases):
    """Item 9: state(), from_state on a fresh context, run() equals the uninterrupted run."""
    for name, recs, cam, h, w, depth in cases:
        ctx = _ctx(tor, recs)
        full = tor.PixelAdaptive(ctx, cam, h, w, depth, **POLICY)
        full.run()
        first = tor.PixelAdaptive(ctx, cam, h, w, depth, **POLICY)
        first.step().step()
        torch.cuda.synchronize()
        saved = first.state()
        assert saved["samples"] == 16 and 0 < saved["list"].size < h * w and saved["rng"].dtype == np.uint64
        other = _ctx(tor, recs)
        again = tor.PixelAdaptive.from_state(other, cam, h, w, depth, None, saved, **POLICY)
        assert again.active == saved["list"].size
        again.run()
        torch.cuda.synchronize()
        a, f = again.state(), full.state()
        assert a["samples"] == f["samples"] and np.array_equal(a["counts"], f["counts"]) and np.array_equal(a["list"], f["list"]), name
        for key in ("rng", "sums", "moments"):
            assert _same(a[key], f[key]), (name, key)
        assert torch.equal(again.image().cpu(), full.image().cpu())
        other.close()
        ctx.close()


def test_bystanders_keep_their_bits(tor, cases):
    """Item 10: a one-shot render_device and a PixelProgressive run before and after listed passes give their usual bits."""
    _, recs, cam, h, w, depth = cases[0]
    ctx = _ctx(tor, recs)
    for accel in (0, 3):
        for pk in _kernels(tor):
            opt = _opt(tor, accel, pk)

            def bystanders():
                one = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
                ctx.render_device(cam, h, w, 12, 2.2, depth, opt, one.data_ptr(), _stream())
                pp = tor.PixelProgressive(ctx, cam, h, w, depth, opt, moments=True).add(5).add(7)
                torch.cuda.synchronize()
                return one.cpu().numpy(), pp.state(), pp.image().cpu().numpy()

            one0, st0, img0 = bystanders()
            assert _same(one0, img0)
            tor.PixelAdaptive(ctx, cam, h, w, depth, opt, **POLICY).run()
            one1, st1, img1 = bystanders()
            assert _same(one1, one0) and _same(img1, img0), (accel, pk)
            for key in ("rng", "sums", "moments"):
                assert _same(st1[key], st0[key]), (accel, pk, key)
    ctx.close()


def test_rejections_write_nothing(tor, cases):
    _, recs, cam, h, w, depth = cases[0]
    ctx = _ctx(tor, recs)
    L = tor.lib()
    rng = torch.full((h, w, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    sums = torch.full((h, w, 3), -7.25, dtype=torch.float64, device="cuda")
    mom = torch.full((h, w, 3), -9.5, dtype=torch.float64, device="cuda")
    lst = torch.arange(0, h * w, dtype=torch.int32, device="cuda")
    pix = tor.make_options(seeding=tor.SEED_PIXEL, accel=3)
    smp = tor.make_options(seeding=tor.SEED_SAMPLE, accel=3)
    bare = tor.Context(0)  # no scene uploaded

    def call(c=ctx, opt=pix, rows=h, cols=w, first=0, n=4, li=lst.data_ptr(), nl=h * w, r=rng.data_ptr(), s=sums.data_ptr(), m=mom.data_ptr()):
        return L.tor_render_resume_list_device(c._h, C.byref(cam), rows, cols, C.c_void_p(li), nl, first, n, depth, C.byref(opt), C.c_void_p(r),
                                               C.c_void_p(s), C.c_void_p(m), C.c_void_p(_stream()))

    bad = (("SEED_SAMPLE", dict(opt=smp), "TOR_SEED_PIXEL"), ("first < 0", dict(first=-1), "2^17"), ("n < 1", dict(n=0), "2^17"),
           ("beyond 2^17", dict(first=(1 << 17) - 3, n=4), "2^17"), ("NULL d_rng", dict(r=0), "NULL"), ("NULL d_sums", dict(s=0), "NULL"),
           ("NULL d_moments", dict(m=0), "NULL"), ("NULL d_list", dict(li=0), "NULL"), ("n_list < 0", dict(nl=-1), "n_list"),
           ("n_list above the shard", dict(nl=h * w + 1), "above the shard"), ("one row", dict(rows=1, nl=1), "nrows >= 2"),
           ("one column", dict(cols=1, nl=1), "ncols >= 2"), ("no scene", dict(c=bare), "no scene"))
    for what, kw, word in bad:
        assert call(**kw) == tor.ERR_INVALID_ARGUMENT, what
        msg = L.tor_last_error().decode()
        assert word in msg and "tor_render_resume_list_device" in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((rng == 0x5A5A5A5A).all()) and bool((sums == -7.25).all()) and bool((mom == -9.5).all())
    with pytest.raises(tor.TorError) as e:
        tor.PixelAdaptive(ctx, cam, h, w, depth, smp)
    assert "Adaptive's" in str(e.value)
    # the sample-stream list entry keeps refusing the pixel streams
    with pytest.raises(tor.TorError):
        ctx.accumulate_list_device(cam, h, w, lst.data_ptr(), 4, 0, 4, depth, pix, sums.data_ptr(), mom.data_ptr(), _stream())
    bare.close()
    ctx.close()
