"""The oracle's raw sample-range sums (oracle.accumulate): the reference the GPU's progressive and adaptive passes are held to.
Resolved, they are the oracle's quantised one-shot render bit for bit; ranges add exactly; the pixel-list and row-range forms
agree; the second moments are consistent with the sums."""
import numpy as np
import pytest

H, W, DEPTH = 12, 20, 50


@pytest.fixture(scope="module")
def objs(ref_scene):
    return ref_scene[0]


def test_resolved_sums_equal_the_quantised_render(oracle, objs, ref_camera):
    n = 11
    S, _ = oracle.accumulate(H, W, 0, n, ref_camera, objs, DEPTH)
    want = oracle.render(H, W, n, ref_camera, objs, DEPTH, seeding=oracle.SEED_SAMPLE, math=oracle.MATH_PORTABLE,
                         arith=oracle.ARITH_STRICT, accum=oracle.ACCUM_QUANTIZED).pixels
    got = oracle.port_pow((1.0 / n) * S, 1.0 / float(np.float32(2.2)))  # canvas.nim:47-54 with the float32 gamma field
    assert np.array_equal(got, want)
    assert float(S.min()) >= 0.0 and float(S.max()) > 0.0


def test_ranges_add_exactly(oracle, objs, ref_camera):
    a, b, c = 3, 10, 17   # a total of 14: not a power of two
    S1, M1 = oracle.accumulate(H, W, a, b - a, ref_camera, objs, DEPTH)
    S2, M2 = oracle.accumulate(H, W, b, c - b, ref_camera, objs, DEPTH)
    S, M = oracle.accumulate(H, W, a, c - a, ref_camera, objs, DEPTH)
    assert np.array_equal(S1 + S2, S) and np.array_equal(M1 + M2, M)
    # every value is a multiple of 2^-36
    for x in (S, M):
        k = x * 2.0 ** 36
        assert np.array_equal(k, np.round(k))
    # a different range is a different set of samples
    assert not np.array_equal(S1, S2)


def test_pixel_list_and_row_range_agree(oracle, objs, ref_camera):
    r0, r1 = 4, 9
    Sr, Mr = oracle.accumulate(H, W, 5, 7, ref_camera, objs, DEPTH, rows=(r0, r1))
    rows_pix = np.arange(r0 * W, r1 * W, dtype=np.int32)
    Sp, Mp = oracle.accumulate(H, W, 5, 7, ref_camera, objs, DEPTH, pixels=rows_pix)
    assert np.array_equal(Sr, Sp) and np.array_equal(Mr, Mp)
    out = np.ones(H, dtype=bool)
    out[r0:r1] = False
    assert np.all(Sr[out] == 0.0) and np.all(Mr[out] == 0.0) and float(Sr[r0:r1].min()) > 0.0
    # a sparse list (pixel 0, the last pixel, gaps) is the whole image's sums at those pixels and zero elsewhere
    Sa, Ma = oracle.accumulate(H, W, 5, 7, ref_camera, objs, DEPTH)
    pix = np.array([0, 1, 7, W, 3 * W + 5, H * W - 2, H * W - 1], dtype=np.int32)
    Sl, Ml = oracle.accumulate(H, W, 5, 7, ref_camera, objs, DEPTH, pixels=pix)
    on = np.zeros(H * W, dtype=bool)
    on[pix] = True
    for got, full in ((Sl, Sa), (Ml, Ma)):
        g, f = got.reshape(-1, 3), full.reshape(-1, 3)
        assert np.array_equal(g[on], f[on]) and np.all(g[~on] == 0.0)
    assert np.array_equal(Sr[r0:r1], Sa[r0:r1])


def test_moments_are_consistent_with_the_sums(oracle, objs, ref_camera):
    for first, n in ((0, 1), (2, 5), (7, 24)):
        S, M = oracle.accumulate(H, W, first, n, ref_camera, objs, DEPTH)
        assert np.all(M >= 0.0) and np.all(M <= S)          # q in [0, 1]: q^2 <= q
        # Cauchy-Schwarz, n * sum(q^2) >= (sum q)^2, up to the rounding of each q^2 to 2^-36 (at most n * 2^-37 per channel)
        assert np.all(n * M - S * S >= -n * n * 2.0 ** -37)
        if n == 1:
            assert np.array_equal(M, np.vectorize(oracle.lib().oracle_quantize36)(S * S))
        else:
            assert np.any(n * M - S * S > 1e-6)                # some pixels do vary between samples


def test_rejects_bad_arguments(oracle, objs, ref_camera):
    with pytest.raises(AssertionError):
        oracle.accumulate(H, W, 0, 2, ref_camera, objs, DEPTH, pixels=np.array([H * W], dtype=np.int32))
    with pytest.raises(AssertionError):
        oracle.accumulate(H, W, 0, 2, ref_camera, objs, DEPTH, rows=(3, H + 1))
