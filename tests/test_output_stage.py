"""The output stage and the shared math on every input, CPU half: the host twins (tor_selftest_math_host, tor_canvas_to_rgb8) and the
oracle against the restatements of tests/output_restatement.py, on the inputs of tests/output_inputs.py.  No GPU, no render.

What each test holds, and what it found when it was written:
  * host math == oracle, bit for bit, on the arguments the sincos error budget names as worst, on every value set x gamma for pow
    (the wild set included: before this sweep the oracle handed x > 2^1000 to libm and returned (2^1001)^0.4545 = 9.0e136 where the
    kernel returns inf), on the quantize36 inputs, and op 6 against both the oracle's unit vector and a numpy restatement;
  * port_pow against mpmath at 300 bits on 2 000 points of unit / lit / tiny per gamma: every result within 1 ulp (the hard
    assertion).  Correct rounding is the expectation and holds on all 12 000 points: NOT_CORRECTLY_ROUNDED, the named list of the
    points that miss it, holds 0 (worst measured: 0.4998 ulp).  Before this sweep pow_pos(2^-1030, 2) was inf and pow_pos(2^-1023.5, 2) NaN on both the host and the device build
    (the exit for a result below the subnormals stood at n < -2100, and from n = -2047 down the scale factor's exponent field went
    negative); both points are in the `tiny` set;
  * quantize36: float trick == rational statement on |x| < 2^15, oracle == float trick everywhere;
  * the quantiser copies on steps / unit / wild: a NaN is 0, every other value the byte it always was;
  * oracle.encode_frame == encode on every frame's planes, and on the slice wherever the oracle writes one (whole macroblocks: its
    flushFrame drops partial ones as the reference's does); the spec decoder recovers the restated planes from the restated slice
    at every size, with the crops the sizes imply;
  * the inputs do what their names say.
Wall time here: about 6 s for the module."""
import ctypes as C

import numpy as np
import pytest

import h264_spec_decoder as dec
import output_inputs as I
import output_restatement as R

# of the 12 000 points of test_port_pow_against_mpmath, the ones that are within 1 ulp but not correctly rounded, as (gamma, x, result,
# ulps): none -- the worst point is 0.4998 ulp from the exact value.  A point that ever lands here stays under the 1-ulp assertion.
NOT_CORRECTLY_ROUNDED = []


def _host(tor, op, x, y=None):
    return tor.selftest_math(op, x, y, where="host")


def test_inputs_do_what_their_names_say():
    w = I.values("wild")
    bits = w.view(np.uint64)
    for b in (I.NAN_POS, I.NAN_NEG, I.NAN_PAYLOAD):
        assert (bits == np.uint64(b)).any() and np.isnan(w[bits == np.uint64(b)]).all()
    for v in (np.inf, -np.inf, -1e-300, -1.0, 2.0 ** 1000, np.nextafter(2.0 ** 1000, 0), np.nextafter(2.0 ** 1000, np.inf), np.finfo(np.float64).max):
        assert (w == v).any(), v
    assert (np.signbit(w) & (w == 0)).any()                                 # -0.0
    assert I.values("unit").min() >= 0 and I.values("unit").max() < 1
    assert I.values("lit").min() == 1.0 and I.values("lit").max() == 2.0 ** 17
    t = I.values("tiny")
    assert t.min() == 5e-324 and (t == 2.0 ** -1022).any() and (t < 2.0 ** -1022).sum() > 900 and t.max() <= np.nextafter(2.0 ** -1022, 1)
    s = I.values("steps")
    assert all((s == k / 256.0).any() for k in range(257)) and (s == 0.999).any() and (s == np.nextafter(0.999, 1)).any() and (s < 0).any()
    assert I.exponent_of(I.GAMMAS[-1]) < 2.0 ** 20 < 1.05 * I.exponent_of(I.GAMMAS[-1])
    # the noise cases cross the 1024-block cap, from both sides and by one pixel
    blocks = [(n + 255) // 256 for n in I.NOISE_NPIX]
    assert 1023 < max(b for b in blocks if b <= 1024) == 1024 and min(b for b in blocks if b > 1024) == 1025 and max(blocks) == 8100
    assert 262144 in I.NOISE_NPIX and 262145 in I.NOISE_NPIX and 262143 in I.NOISE_NPIX
    for npix in (1, 257, 262144 + 256 * 3 + 7):
        for n in I.NOISE_N:
            S, M = I.noise_case(npix, n, wild=True)
            planted = I.wild_pixels(npix)
            with np.errstate(invalid="ignore", over="ignore"):
                var = (M - S * S / n) / (n - 1.0)
            clamp = [p for p, k in planted.items() if k in ("clamp", "all")]
            assert clamp and all(var[p, 2] < 0 for p in clamp)              # a planted M < S^2/n pixel clamps
            assert any(np.isnan(S[p]).any() for p in planted) and any(np.isinf(S[p]).any() for p in planted)
            if npix > 262144:
                assert any(p >= 262144 for p in planted) and any(p < 256 for p in planted) and any(p >= npix - 256 for p in planted)
            plain, _ = I.noise_case(npix, n)
            with np.errstate(invalid="ignore"):
                pv = (I.noise_case(npix, n)[1] - plain * plain / n)
            assert npix < 200 or ((pv < 0).any() and (pv > 0).any())        # real accumulations: M - S^2/n sometimes just below 0
    # select: kept and dropped entries in the first and in the last tile
    seen_last = False
    for name, S, M, lst, n, a, r in I.select_cases():
        keep, _, _ = R.select(S, M, lst, n, a, r, np.zeros(I.SELECT_NPIX, np.int32))
        if name.endswith(("/mixed", "/relative")) and len(lst) >= 1023:
            first = keep[:I.SELECT_TILE]
            assert first.any() and not first.all(), name
            last = keep[(len(lst) - 1) // I.SELECT_TILE * I.SELECT_TILE:]
            if last.size >= 2:
                assert last.any() and not last.all(), name
                seen_last = seen_last or len(lst) > I.SELECT_TILE
        if name.startswith("repeated"):
            assert np.unique(lst).size < len(lst) // 2
    assert seen_last
    # encoder frames: every wild value somewhere, the first ones where the padding replicates
    for h, w in I.FRAMES:
        px = I.frame(h, w, "wild")
        k = min(len(I.WILD), px.size)
        have = set(px.view(np.uint64).reshape(-1).tolist())
        assert all(int(b) in have for b in I.WILD[:k].view(np.uint64)), (h, w)
        assert np.isnan(px[0, w - 1, 0]) and np.isnan(px[h - 1, w - 1, 1])
    a = I.sincos_arguments()
    assert a.min() == 0 and a.max() < I.SINCOS_SLOW_END and (a >= I.SINCOS_FAST_END).sum() > 3000 and (np.signbit(a) & (a == 0)).any()
    assert (a == np.pi).any() and (a == np.pi / 2).any() and (a == 2 * np.pi).any() and (a == np.nextafter(I.SINCOS_FAST_END, 0)).any()


def test_host_math_is_the_oracles(tor, oracle):
    L = oracle.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    a = np.ascontiguousarray(I.sincos_arguments())
    s, c = _host(tor, 0, a)
    s2, c2 = np.empty_like(a), np.empty_like(a)
    L.oracle_port_sincos(dp(a), dp(s2), dp(c2), a.size)
    assert R.same_bits(s, s2) and R.same_bits(c, c2)
    p, _ = _host(tor, 1, a)
    p2 = np.empty_like(a)
    L.oracle_port_pow5(dp(a), dp(p2), a.size)
    assert R.same_bits(p, p2)
    for gamma in I.GAMMAS:
        y = I.exponent_of(gamma)
        for name in I.VALUE_SETS:
            x = I.values(name)
            got, _ = _host(tor, 2, x, np.full_like(x, y))
            assert R.same_bits(got, oracle.port_pow(x, y)), (name, gamma)
    # the exits, in pow_pos's order, by value: what both comments state
    x = np.array([np.nan, -1.0, -1e-300, -np.inf, -0.0, 0.0, 2.0 ** 1000, np.nextafter(2.0 ** 1000, np.inf), 2.0 ** 1001, np.inf, 2.0 ** -1030, 5e-324])
    for y, want in ((I.exponent_of(2.2), [np.nan] * 4 + [0.0, 0.0, None, np.inf, np.inf, np.inf, None, None]),
                    (2.0, [np.nan] * 4 + [0.0, 0.0, np.inf, np.inf, np.inf, np.inf, 0.0, 0.0])):
        got = oracle.port_pow(x, y)
        for g, w_ in zip(got, want):
            assert w_ is None or (np.isnan(g) if np.isnan(w_) else g == w_), (y, got)
        assert np.isfinite(got[6]) or y == 2.0
    for y in (0.0, -1.0, np.nan):
        assert np.isnan(oracle.port_pow(np.array([0.5, 0.0, 2.0]), y)).all()
    q = np.ascontiguousarray(I.quantize36_inputs())
    got, _ = _host(tor, 5, q)
    assert R.same_bits(got, np.array([L.oracle_quantize36(float(v)) for v in q])) and R.same_bits(got, R.quantize36(q))
    ux, uy = a, a[::-1].copy()
    for x_, y_ in ((ux, uy), (q[np.isfinite(q)], q[np.isfinite(q)][::-1].copy())):
        d, u = _host(tor, 6, x_, y_)
        od, ou = oracle.unit_vector_probe(x_, y_)
        rd, ru = R.unit_vector_probe(x_, y_)
        assert R.same_bits(d, od) and R.same_bits(u, ou) and R.same_bits(d, rd) and R.same_bits(u, ru)


def test_port_pow_against_mpmath(oracle):
    import mpmath
    rng = np.random.default_rng(I.SEED)
    pts = np.concatenate([rng.choice(I.values("unit"), 700, replace=False), rng.choice(I.values("lit"), 700, replace=False),
                          I.values("tiny")[:12], rng.choice(I.values("tiny")[12:], 588, replace=False)])
    assert pts.size == 2000 and (pts > 0).all()
    worst, misses = 0.0, []
    with mpmath.workprec(300):
        overflow = mpmath.mpf(2) ** 1024 - mpmath.mpf(2) ** 970             # from here up the nearest double is inf
    for gamma in I.GAMMAS:
        y = I.exponent_of(gamma)
        got = oracle.port_pow(pts, y)
        exact = R.pow_exact(pts, y)
        big = np.array([e >= overflow for e in exact])
        assert np.array_equal(np.isinf(got), big), gamma                    # inf exactly where the exact value rounds to inf
        ulps = R.ulps_from_exact(got[~big], [e for e, b in zip(exact, big) if not b])
        worst = max(worst, float(ulps.max()))
        assert ulps.max() <= 1.0, (gamma, float(ulps.max()), pts[~big][int(np.argmax(ulps))])
        for x, g, u in zip(pts[~big], got[~big], ulps):
            if u > 0.5:
                misses.append((gamma, float(x), float(g), float(u)))
    print(f"port_pow against mpmath: worst {worst:.4f} ulp over {len(I.GAMMAS) * pts.size} points, {len(misses)} not correctly rounded")
    assert misses == NOT_CORRECTLY_ROUNDED, misses[:5]


def test_quantize36_float_trick_is_the_rational_statement(oracle):
    L = oracle.lib()
    x = I.quantize36_inputs()
    trick = R.quantize36(x)
    inside = np.isfinite(x) & (np.abs(x) < 2.0 ** 15)
    assert inside.sum() > 3000
    exact = np.array([R.quantize36_exact(v) for v in x[inside]])
    assert np.array_equal(trick[inside].view(np.uint64), exact.view(np.uint64))          # (no -0.0 either way)
    assert R.same_bits(trick, np.array([L.oracle_quantize36(float(v)) for v in x]))
    ties = x[inside][np.abs(x[inside] * 2.0 ** 37 % 2) == 1]
    assert ties.size > 200 and ((R.quantize36(ties) * 2.0 ** 36) % 2 == 0).all()         # ties went to the even multiple


@pytest.mark.parametrize("name", ("steps", "unit", "wild"))
def test_quantiser_copies(tor, oracle, name):
    v = I.values(name)
    px = np.resize(v, (-(-v.size // 6), 2, 3))                              # rows x 2 columns: both copies flip the rows
    want = R.quantize_rgb8(px)[::-1]
    cv = tor.new_canvas(px.shape[0], 2, 1, 2.2)
    cv.pixels[:] = px
    assert np.array_equal(tor.export_rgb8(cv), want)
    assert np.array_equal(oracle.quantize_ppm(px), want)
    if name == "wild":
        assert (want.reshape(-1)[np.isnan(px[::-1]).reshape(-1)] == 0).all() and want.max() == 255
    if name == "steps":                                                      # every byte value, and the edges of each
        assert set(want.reshape(-1).tolist()) == set(range(256))


@pytest.mark.parametrize("h,w", I.FRAMES)
def test_encoder_restatement(tor, oracle, h, w):
    for content in I.FRAME_CONTENTS:
        px = I.frame(h, w, content)
        rgb, Y, Cb, Cr, sl = R.encode(px)
        orgb, oY, oCb, oCr, osl = oracle.encode_frame(px)
        assert np.array_equal(rgb, orgb) and np.array_equal(Y, oY) and np.array_equal(Cb, oCb) and np.array_equal(Cr, oCr), content
        assert len(sl) == tor.h264_frame_bytes(w, h)
        if h % 16 == 0 and w % 16 == 0:
            assert sl == osl, content
        sps, pps, pics = dec.decode_stream(tor.h264_stream_header(w, h) + sl)
        assert len(pics) == 1 and sps["frame_cropping"] == int(any(R.crop_of(h, w))) and sps.get("crop", [0, 0, 0, 0]) == R.crop_of(h, w)
        assert sps["pic_width_in_mbs"] == (w + 15) // 16 and sps["pic_height_in_map_units"] == (h + 15) // 16
        _, dy, dcb, dcr = pics[0]
        assert np.array_equal(dy, Y) and np.array_equal(dcb, Cb) and np.array_equal(dcr, Cr), content
        if content == "primaries" and h * w >= 36:                                         # BT.601 limited range, and chroma on both sides of 128
            assert Y.min() >= 16 and Y.max() <= 235 and Cb.min() < 60 and Cb.max() > 200 and Cr.min() < 60 and Cr.max() > 200
        if content == "wild":
            assert (rgb.reshape(-1)[np.isnan(px[::-1]).reshape(-1)] == 0).all()


def test_noise_restatement_keeps_the_kernel_order():
    """The vectorised noise() against the loop that walks one block and one thread at a time, at 1024 blocks with a second-level walk of
    four rounds, on both sides of the cap, and on the small frames."""
    for npix in (1, 255, 257, 262143, 262144, 262145, 262144 + 256 * 3 + 7):
        for wild in (False, True):
            S, M = I.noise_case(npix, 17, wild)
            e, mean, mx = R.noise(S, M, 17)
            assert not np.isnan(e).any() and mean == R.noise_in_kernel_order(S, M, 17) and mx == e.max() and (npix < 200 or 0 < mean < mx)
            if wild:
                for p, kind in I.wild_pixels(npix).items():
                    assert e[p] == 0.0 or kind in ("inf", "clamp")          # NaN and infinite sums report 0
    # the order matters: the same errors summed one after the other give other bits (so the comparison above can fail)
    S, M = I.noise_case(262144 + 256 * 3 + 7, 17)
    e, mean, _ = R.noise(S, M, 17)
    assert mean != float(np.cumsum(e)[-1]) / e.size


def test_select_restatement_against_the_packages(tor):
    for name, S, M, lst, n, a, r in I.select_cases():
        keep, counts, out = R.select(S, M, lst, n, a, r, np.full(I.SELECT_NPIX, -7, np.int32))
        with np.errstate(all="ignore"):
            assert np.array_equal(out, tor.adaptive_select_host(S, M, lst, n, a, r)), name
        assert (counts[np.unique(lst)] == n).all() and (np.delete(counts, np.unique(lst)) == -7).all()
        planted = I.wild_pixels(I.SELECT_NPIX)
        for i, p in enumerate(lst):
            if planted.get(int(p)) == "nan":
                assert keep[i], name                                         # a NaN pixel never converges
