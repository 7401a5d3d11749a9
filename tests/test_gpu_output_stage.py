"""The output stage and the shared math on every input, on the MI355X: the kernels of csrc/kernel/output_stage.hpp (resolve,
resolve-by-counts, the noise estimate, the adaptive select, the 8-bit quantiser, the fused RGB -> Y'CbCr -> I_PCM encoder) and the device
build of csrc/tor_math.hpp and quantize36 against the restatements of tests/output_restatement.py on the inputs of
tests/output_inputs.py -- bit for bit, NaN placement compared separately (a NaN's sign and payload are nobody's contract).

One small context throughout, no scene; test_rendered_nan_goes_out_black alone renders (one 20 x 34 frame of tests/render_regimes.py
whose oracle canvas holds NaNs) to tie the render's NaNs to the quantiser's and the encoder's black.

What a wrong build fails here is recorded in profiles/output_stage_mutants.txt: nine deliberately wrong builds, eight caught; the
ninth, the quantiser without its NaN branch, gives the same bytes on this hardware (the branch removes an undefined conversion,
not a wrong value) and is argued there.

Measured wall time on the MI355X, 51 cases in 4.8 s: test_accum_noise[2073600-17] 0.54 s, [2073600-2] 0.33 s, [2073600-131072] 0.26 s
(most of it the inputs and the restatement on the CPU), test_device_math_is_the_hosts_and_the_oracles 0.37 s, the four
test_accum_noise[262143 .. 262919-17] 0.15 .. 0.18 s each, test_resolve[unit] 0.04 s, every other case 0.05 s or less."""
import ctypes as C

import numpy as np
import pytest
import torch

import output_inputs as I
import output_restatement as R
import render_regimes as RR

pytestmark = pytest.mark.gpu

GUARD = 8                                                   # elements behind every output that must keep their sentinel
SENTINEL = -7.25


@pytest.fixture(scope="module")
def ctx(tor):
    c = tor.Context(0)
    yield c
    c.close()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()    # (a copy: the inputs are read-only)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_device_math_is_the_hosts_and_the_oracles(tor, oracle):
    L = oracle.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    a = np.ascontiguousarray(I.sincos_arguments())
    s, c = tor.selftest_math(0, a)
    hs, hc = tor.selftest_math(0, a, where="host")
    os_, oc = np.empty_like(a), np.empty_like(a)
    L.oracle_port_sincos(dp(a), dp(os_), dp(oc), a.size)
    assert R.same_bits(s, hs) and R.same_bits(c, hc) and R.same_bits(s, os_) and R.same_bits(c, oc)
    p, _ = tor.selftest_math(1, a)
    op = np.empty_like(a)
    L.oracle_port_pow5(dp(a), dp(op), a.size)
    assert R.same_bits(p, tor.selftest_math(1, a, where="host")[0]) and R.same_bits(p, op)
    for gamma in I.GAMMAS:
        y = I.exponent_of(gamma)
        x = np.concatenate([I.values(name) for name in I.VALUE_SETS])
        yy = np.full_like(x, y)
        got, _ = tor.selftest_math(2, x, yy)
        assert R.same_bits(got, tor.selftest_math(2, x, yy, where="host")[0]) and R.same_bits(got, oracle.port_pow(x, y)), gamma
    q = np.ascontiguousarray(I.quantize36_inputs())
    got, _ = tor.selftest_math(5, q)
    assert R.same_bits(got, tor.selftest_math(5, q, where="host")[0]) and R.same_bits(got, R.quantize36(q))
    assert R.same_bits(got, np.array([L.oracle_quantize36(float(v)) for v in q]))
    fq = q[np.isfinite(q)]
    for x_, y_ in ((a, a[::-1].copy()), (fq, fq[::-1].copy())):
        d, u = tor.selftest_math(6, x_, y_)
        hd, hu = tor.selftest_math(6, x_, y_, where="host")
        od, ou = oracle.unit_vector_probe(x_, y_)
        rd, ru = R.unit_vector_probe(x_, y_)
        assert R.same_bits(d, hd) and R.same_bits(u, hu) and R.same_bits(d, od) and R.same_bits(u, ou) and R.same_bits(d, rd) and R.same_bits(u, ru)


def _check_resolve(call, sums, want, what):
    """call(d_sums_ptr, d_pixels_ptr) out of place into a guarded buffer, then in place in a guarded copy of the sums."""
    n = sums.size
    src = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    src[:n] = _dev(sums)
    dst = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    call(src.data_ptr(), dst.data_ptr())
    out, kept = _host(dst), _host(src)
    assert R.same_bits(out[:n], want), f"{what}, out of place: {int((~np.isnan(want) & (out[:n] != want)).sum())} of {n} values differ"
    assert (out[n:] == SENTINEL).all() and R.same_bits(kept[:n], sums) and (kept[n:] == SENTINEL).all(), what
    call(src.data_ptr(), src.data_ptr())
    out = _host(src)
    assert R.same_bits(out[:n], want) and (out[n:] == SENTINEL).all(), f"{what}, in place"


@pytest.mark.parametrize("name", I.VALUE_SETS)
def test_resolve(tor, oracle, ctx, name):
    v = I.values(name)
    for gamma in I.GAMMAS:
        for k, n in enumerate(I.SIZES + (v.size,)):
            total = I.TOTALS[k % len(I.TOTALS)]
            sums = np.resize(v, n) if n else np.zeros(0)
            want = R.resolve(oracle, sums, 1.0 / total, gamma)
            _check_resolve(lambda s, p: ctx.resolve_device(s, n, total, gamma, p, _stream()), sums, want, f"{name} gamma {gamma} n {n} / {total}")


@pytest.mark.parametrize("name", I.VALUE_SETS)
def test_resolve_counts(tor, oracle, ctx, name):
    v = I.values(name)
    for gamma in I.GAMMAS:
        for npix in I.COUNTS_NPIX:
            counts = I.counts_strip(npix)
            sums = np.resize(v, npix * 3) if npix else np.zeros(0)
            if npix == 257:
                assert set(counts.tolist()) == set(I.COUNTS)
                sums = sums.copy()
                sums[:257 * 3:3] = 0.0                                      # a sum of 0 under every count: inf * 0 and -x * 0
            dc = _dev(counts) if npix else torch.zeros(1, dtype=torch.int32, device="cuda")
            want = R.resolve(oracle, sums, counts, gamma)
            _check_resolve(lambda s, p: ctx.resolve_counts_device(s, dc.data_ptr(), npix, gamma, p, _stream()), sums, want,
                           f"{name} gamma {gamma} npix {npix}")


@pytest.mark.parametrize("n", I.NOISE_N)
@pytest.mark.parametrize("npix", I.NOISE_NPIX)
def test_accum_noise(tor, ctx, npix, n):
    for wild in (False, True):
        if wild and npix > 300000 and n != 17:
            continue                                                        # (the 1920 x 1080 frame: the wild variant once)
        S, M = I.noise_case(npix, n, wild)
        e, mean, mx = R.noise(S, M, n)
        dS, dM = _dev(S), _dev(M)
        err = torch.full((npix + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        got = ctx.accum_noise_device(dS.data_ptr(), dM.data_ptr(), npix, n, err.data_ptr(), _stream())
        first = _host(err)
        print(f"noise npix {npix} n {n} wild {wild}: device {got}, restated {(mean, mx)}")
        assert np.array_equal(first[:npix].view(np.uint64), e.view(np.uint64)) and (first[npix:] == SENTINEL).all(), (npix, n, wild)
        assert got == (mean, mx), (npix, n, wild, got, (mean, mx))
        again = ctx.accum_noise_device(dS.data_ptr(), dM.data_ptr(), npix, n, err.data_ptr(), _stream())
        assert again == got and np.array_equal(_host(err).view(np.uint64), first.view(np.uint64))
        assert ctx.accum_noise_device(dS.data_ptr(), dM.data_ptr(), npix, n, 0, _stream()) == got     # without err
        assert R.same_bits(_host(dS), S) and R.same_bits(_host(dM), M)


def test_adaptive_select(tor, ctx):
    dS = dM = None
    for name, S, M, lst, n, abs_tol, rel_tol in I.select_cases():
        if dS is None:
            dS, dM = _dev(S), _dev(M)
        before = np.full(I.SELECT_NPIX, -7, dtype=np.int32)
        keep, counts, survivors = R.select(S, M, lst, n, abs_tol, rel_tol, before)
        dl = _dev(lst)
        dout = torch.full((len(lst) + GUARD,), -9, dtype=torch.int32, device="cuda")
        dcounts = _dev(before)
        n_out = ctx.adaptive_select_device(dS.data_ptr(), dM.data_ptr(), dl.data_ptr(), len(lst), n, abs_tol, rel_tol, dout.data_ptr(),
                                           dcounts.data_ptr(), _stream())
        out = _host(dout)
        assert n_out == len(survivors), (name, n_out, len(survivors))
        assert np.array_equal(out[:n_out], survivors) and (out[n_out:] == -9).all(), name
        assert np.array_equal(_host(dcounts), counts), name                  # listed pixels at n, every other one untouched
        assert np.array_equal(_host(dl), lst)


@pytest.mark.parametrize("name", I.VALUE_SETS)
def test_quantize_rgb8(tor, ctx, name):
    v = I.values(name)
    for n in I.SIZES + (v.size,):
        px = np.resize(v, n) if n else np.zeros(0)
        d = _dev(px) if n else torch.zeros(1, dtype=torch.float64, device="cuda")
        out = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.quantize_rgb8_device(d.data_ptr(), n, out.data_ptr(), _stream())
        got = _host(out)
        assert np.array_equal(got[:n], R.quantize_rgb8(px)) and (got[n:] == 0xA5).all(), (name, n)


def _encode_on_device(tor, ctx, px, planes):
    h, w, _ = px.shape
    nbytes = tor.h264_frame_bytes(w, h)
    d = _dev(px)
    sl = torch.full((nbytes + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    Y = torch.full((h, w), 0xA5, dtype=torch.uint8, device="cuda")
    Cb = torch.full((h // 2, w // 2), 0xA5, dtype=torch.uint8, device="cuda")
    Cr = torch.full((h // 2, w // 2), 0xA5, dtype=torch.uint8, device="cuda")
    if planes:
        ctx.encode_frame_device(d.data_ptr(), h, w, sl.data_ptr(), Y.data_ptr(), Cb.data_ptr(), Cr.data_ptr(), _stream())
    else:
        ctx.encode_frame_device(d.data_ptr(), h, w, sl.data_ptr(), stream_ptr=_stream())
    return _host(sl), _host(Y), _host(Cb), _host(Cr)


@pytest.mark.parametrize("h,w", I.FRAMES)
def test_encode_frame(tor, ctx, h, w):
    for content in I.FRAME_CONTENTS:
        px = I.frame(h, w, content)
        _, wY, wCb, wCr, wsl = R.encode(px)
        for planes in (True, False):
            sl, Y, Cb, Cr = _encode_on_device(tor, ctx, px, planes)
            assert sl[:-1].tobytes() == wsl and sl[-1] == 0xA5, (content, planes)
            if planes:
                assert np.array_equal(Y, wY) and np.array_equal(Cb, wCb) and np.array_equal(Cr, wCr), content
            else:
                assert (Y == 0xA5).all() and (Cb == 0xA5).all() and (Cr == 0xA5).all()


def test_rendered_nan_goes_out_black(tor, oracle):
    """A NaN that a render produced goes out as black: the `dense` regime from 1e9 units away (tests/render_regimes.py), rendered at
    20 x 34 as tests/test_gpu_render_regimes.py renders it, quantised and encoded on the device, against the restatements applied to the
    ORACLE's canvas."""
    name, cam = "dense", "tele_1e+09"
    recs = RR.scene(name, 0)
    kw = RR.camera(name, cam, recs)
    tcam, ocam = tor.camera(**kw), RR.oracle_camera(oracle, kw)
    want = oracle.render(RR.H, RR.W, RR.SPP, ocam, recs, max_depth=RR.DEPTH, seeding=oracle.SEED_PIXEL, math=oracle.MATH_PORTABLE,
                         accum=oracle.ACCUM_SEQUENTIAL).pixels
    assert np.isnan(want).sum() >= 100 and np.isfinite(want).sum() >= 100
    ctx = tor.Context(0)
    try:
        ctx.upload(tor.Scene.from_records(recs).list())
        buf = torch.zeros((RR.H, RR.W, 3), dtype=torch.float64, device="cuda")
        ctx.render_device(tcam, RR.H, RR.W, RR.SPP, 2.2, RR.DEPTH, tor.make_options(seeding=tor.SEED_PIXEL), buf.data_ptr(), _stream())
        assert R.same_bits(_host(buf), want)
        out = torch.full((RR.H, RR.W, 3), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.quantize_rgb8_device(buf.data_ptr(), buf.numel(), out.data_ptr(), _stream())
        rgb = R.quantize_rgb8(want)
        assert np.array_equal(_host(out), rgb) and (rgb[np.isnan(want)] == 0).all() and rgb.max() > 0
        nbytes = tor.h264_frame_bytes(RR.W, RR.H)
        sl = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        Y = torch.zeros((RR.H, RR.W), dtype=torch.uint8, device="cuda")
        Cb = torch.zeros((RR.H // 2, RR.W // 2), dtype=torch.uint8, device="cuda")
        Cr = torch.zeros_like(Cb)
        ctx.encode_frame_device(buf.data_ptr(), RR.H, RR.W, sl.data_ptr(), Y.data_ptr(), Cb.data_ptr(), Cr.data_ptr(), _stream())
        _, wY, wCb, wCr, wsl = R.encode(want)
        assert _host(sl).tobytes() == wsl and np.array_equal(_host(Y), wY) and np.array_equal(_host(Cb), wCb) and np.array_equal(_host(Cr), wCr)
        black = np.isnan(want[::-1]).all(axis=2)                            # (video rows: top scanline first)
        assert black.any() and (wY[black] == 16).all()                      # BT.601 limited range: black is Y' = 16
    finally:
        ctx.close()
