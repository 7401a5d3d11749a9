"""Plain numpy / Python-int restatements of the output stage (csrc/kernel/output_stage.hpp), of quantize36 (tor_device.hpp) and of the
math self-test's unit_vector -- second texts: nothing here imports the product or calls the oracle's encoder, quantiser or selftest.
resolve() alone goes through oracle.port_pow (the bit-level twin of pow_pos, itself held to mpmath by tests/test_output_stage.py);
resolve_exact() says in 300-bit arithmetic what the value should be.

The reference's line numbers are cited the way output_stage.hpp cites them."""
from fractions import Fraction

import numpy as np

import output_inputs as I


def same_bits(a, b):
    """Equal as bit patterns wherever neither is a NaN, and NaNs in the same places (a NaN's sign and payload are not compared)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    an, bn = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(an, bn) and ((a.view(np.uint64) == b.view(np.uint64)) | an).all())


# ---- quantiser: io/ppm.nim:15-16, safe_math.nim:10-14 ----------------------------------------------------------------------------
def quantize_rgb8(px):
    """uint8, the shape of px: int(256 * clip(c, 0, 0.999)), a NaN 0.  The NaN branch is explicit: numpy's cast of NaN is not used."""
    px = np.asarray(px, dtype=np.float64)
    out = np.zeros(px.shape, dtype=np.uint8)
    flat, oflat = px.reshape(-1), out.reshape(-1)
    nan = np.isnan(flat)
    ok = ~nan
    oflat[ok] = np.floor(256.0 * np.clip(flat[ok], 0.0, 0.999)).astype(np.int64).astype(np.uint8)   # (>= 0: floor is int's truncation)
    oflat[nan] = 0
    return out


# ---- encoder: io/rgb.nim:17-31, io/color_conversions.nim:180-252, io/h264.nim:189-259 --------------------------------------------
def _fixed(x, precision):
    return int(x * (1 << precision) + 0.5)                                  # color_conversions.nim:107-108


KR, KB = _fixed(0.299, 8), _fixed(0.114, 8)                                 # :110-120 BT.601
KG = 256 - KR - KB
FB = _fixed((224.0 / 255.0) / (2.0 * (1.0 - 0.114)), 8)                     # :176-178
FR = _fixed((224.0 / 255.0) / (2.0 * (1.0 - 0.299)), 8)
Y_SCALE, Y_MIN = _fixed((235.0 - 16.0) / 255.0, 7), 16
assert (KR, KG, KB, FB, FR, Y_SCALE) == (77, 150, 29, 127, 160, 110)
SLICE_HEADER = bytes([0x00, 0x00, 0x00, 0x01, 0x05, 0x88, 0x84, 0x21, 0xa0])  # h264.nim:38


def crop_of(h, w):
    """frame_crop_{left, right, top, bottom}_offset of the SPS for an h x w frame, in chroma samples (H.264 7.4.2.1.1)."""
    return [0, (-w % 16) // 2, 0, (-h % 16) // 2]


def encode(px):
    """(rgb (h, w, 3) top scanline first, Y (h, w), Cb (h/2, w/2), Cr, slice bytes) of an (h, w, 3) canvas whose row 0 is the bottom
    scanline; h and w even.  int64 throughout, >> is the floor shift.  A size that is not a multiple of 16 is padded to whole macroblocks
    by replicating the last row and column of the RGB picture (what encode_ipcm_kernel documents: `sr = vr < nrows ? vr : nrows - 1`);
    the planes are returned cropped, the slice holds the padded macroblocks."""
    px = np.asarray(px, dtype=np.float64)
    h, w, _ = px.shape
    assert h % 2 == 0 and w % 2 == 0 and h >= 2 and w >= 2
    rgb = quantize_rgb8(px)[::-1]                                           # rgb.nim:29-31, the intended flip nrows - 1 - i
    full = np.pad(rgb.astype(np.int64), ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge")
    R, G, B = full[..., 0], full[..., 1], full[..., 2]
    tY = (KR * R + KG * G + KB * B) >> 8                                    # color_conversions.nim:218-220
    Y = (((tY * Y_SCALE) >> 7) + Y_MIN) & 0xFF                              # :223
    dU, dV = B - tY, R - tY                                                 # :221-222
    tU = dU[0::2, 0::2] + dU[0::2, 1::2] + dU[1::2, 0::2] + dU[1::2, 1::2]
    tV = dV[0::2, 0::2] + dV[0::2, 1::2] + dV[1::2, 0::2] + dV[1::2, 1::2]
    assert np.abs(tU).max() < 2 ** 15 and np.abs(tV).max() < 2 ** 15 and np.abs((tV >> 2) * FR).max() < 2 ** 15   # int16 never wraps
    U = ((((tU >> 2) * FB) >> 8) + 128) & 0xFF                              # :249
    V = ((((tV >> 2) * FR) >> 8) + 128) & 0xFF                              # :250
    Y, U, V = Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)
    out = bytearray(SLICE_HEADER)
    for i in range(full.shape[0] // 16):                                    # h264.nim:249-259 flushFrame, :189-202 encodeMacroblock
        for j in range(full.shape[1] // 16):
            if i or j:
                out += b"\x0d\x00"                                          # h264.nim:39,191-192
            out += Y[16 * i:16 * i + 16, 16 * j:16 * j + 16].tobytes()
            out += U[8 * i:8 * i + 8, 8 * j:8 * j + 8].tobytes()
            out += V[8 * i:8 * i + 8, 8 * j:8 * j + 8].tobytes()
    out += b"\x80"                                                          # h264.nim:40,259
    return (rgb, np.ascontiguousarray(Y[:h, :w]), np.ascontiguousarray(U[:h // 2, :w // 2]), np.ascontiguousarray(V[:h // 2, :w // 2]),
            bytes(out))


# ---- resolve: canvas.nim:47-54 ---------------------------------------------------------------------------------------------------
def resolve_argument(sums, scale_or_counts):
    """scale * sums as the kernels form it: a float scale (tor_resolve_device: 1.0 / total_samples, computed by the caller), or an
    integer array of per-pixel counts (resolve_counts_kernel: (1.0 / (double)counts[i / 3]) * sums[i]; a count of 0 gives scale inf)."""
    sums = np.asarray(sums, dtype=np.float64)
    if isinstance(scale_or_counts, np.ndarray) and scale_or_counts.dtype.kind == "i":
        with np.errstate(divide="ignore"):
            scale = np.repeat(1.0 / scale_or_counts.astype(np.float64), 3)[:sums.size].reshape(sums.shape)
    else:
        scale = float(scale_or_counts)
    with np.errstate(invalid="ignore", over="ignore"):
        return scale * sums


def resolve(oracle, sums, scale_or_counts, gamma):
    """pow(scale * sums, 1 / gamma) through oracle.port_pow: for bit comparisons."""
    x = resolve_argument(sums, scale_or_counts)
    return oracle.port_pow(x.reshape(-1), I.exponent_of(gamma)).reshape(x.shape)


def pow_exact(x, y, bits=300):
    """[mpmath.mpf] x^y for finite x > 0 at `bits` bits."""
    import mpmath
    with mpmath.workprec(bits):
        return [mpmath.power(mpmath.mpf(float(v)), mpmath.mpf(float(y))) for v in np.asarray(x).reshape(-1)]


def ulps_from_exact(got, exact, bits=300):
    """|got - exact| in units of the spacing of doubles at `exact` (2^-1074 in and below the subnormals), as floats."""
    import mpmath
    out = []
    with mpmath.workprec(bits):
        for g, e in zip(np.asarray(got, dtype=np.float64).reshape(-1), exact):
            if e == 0:
                out.append(0.0 if g == 0 else np.inf)
                continue
            ex = max(int(mpmath.floor(mpmath.log(abs(e), 2))), -1022)
            out.append(float(abs(mpmath.mpf(float(g)) - e) / mpmath.ldexp(1, ex - 52)) if np.isfinite(g) else np.inf)
    return np.array(out)


# ---- noise: accum_noise_kernel + accum_noise_finish_kernel ------------------------------------------------------------------------
def _tree(v):
    """The kernels' shared-memory tree over the last axis (256 wide): v[t] += v[t + w] for w = 128, 64, .., 1."""
    v = v.copy()
    w = 128
    while w > 0:
        v[..., :w] = v[..., :w] + v[..., w:2 * w]
        w >>= 1
    return v[..., 0]


def _strided_sum(e, lanes):
    """Thread t of `lanes` threads adds e[t], e[t + lanes], .. in that order (a missing entry adds nothing: + 0.0 on a sum that is never
    -0.0 is the same bits) -> (lanes,)."""
    rounds = max((e.size + lanes - 1) // lanes, 1)
    ep = np.zeros(rounds * lanes)
    ep[:e.size] = e
    ep = ep.reshape(rounds, lanes)
    acc = np.zeros(lanes)
    for k in range(rounds):
        acc = acc + ep[k]
    return acc


def noise(S, M, n):
    """tor_accum_noise_device restated: (the per-pixel error (npix,), the frame's mean, its maximum).  The sum runs in the kernels'
    fixed order -- a grid of min(ceil(npix / 256), 1024) blocks, thread t of block b adds pixels b 256 + t + k grid 256 in order, a tree
    per block of 256, then one block walks the partials the same way (four per thread at 1024) -- vectorised over the blocks, not
    reordered.  `var > 0 ? var : 0` takes a NaN variance to 0 (np.where does the same), so no NaN reaches the sums."""
    n = float(n)
    S, M = np.asarray(S, dtype=np.float64), np.asarray(M, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        var = (M - S * S / n) / (n - 1.0)
        var = np.where(var > 0.0, var, 0.0)
        e = np.sqrt(var / n).max(axis=-1).reshape(-1)
    npix = e.size
    blocks = min((npix + I.NOISE_BLOCK - 1) // I.NOISE_BLOCK, I.NOISE_MAX_BLOCKS)
    partial = _tree(_strided_sum(e, blocks * I.NOISE_BLOCK).reshape(blocks, I.NOISE_BLOCK))
    total = _tree(_strided_sum(partial, I.NOISE_BLOCK))
    return e, float(total) / npix, float(e.max())


def noise_in_kernel_order(S, M, n):
    """noise()'s mean once more, one block and one thread at a time (the loop tests/test_gpu_resume.py carried): slow, for small frames."""
    e = noise(S, M, n)[0]
    npix = e.size
    blocks = min((npix + 255) // 256, 1024)
    partial = np.zeros(blocks)
    for b in range(blocks):
        acc = np.zeros(256)
        for i0 in range(b * 256, npix, blocks * 256):
            chunk = e[i0:i0 + 256]
            acc[:chunk.size] = acc[:chunk.size] + chunk
        partial[b] = _tree(acc)
    acc = np.zeros(256)
    for b0 in range(0, blocks, 256):
        chunk = partial[b0:b0 + 256]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    return float(_tree(acc)) / npix


# ---- select: adaptive_still_active + the ordered compaction -----------------------------------------------------------------------
def select(S, M, lst, n, abs_tol, rel_tol, counts):
    """(keep (len(lst),) bool, counts after the call, the survivors in input order): a pixel has converged iff
    sqrt(max(0, (M - S S / n) / (n - 1)) / n) <= abs_tol + rel_tol (S / n) in all three channels, a comparison with a NaN being false."""
    n = float(n)
    lst = np.asarray(lst, dtype=np.int64)
    s, m = np.asarray(S).reshape(-1, 3)[lst], np.asarray(M).reshape(-1, 3)[lst]
    with np.errstate(invalid="ignore", over="ignore"):
        mean = s / n
        var = (m - s * s / n) / (n - 1.0)
        var = np.where(var > 0.0, var, 0.0)
        se = np.sqrt(var / n)
        converged = (se <= abs_tol + rel_tol * mean).all(axis=1)
    keep = ~converged
    counts = np.array(counts, dtype=np.int32, copy=True)
    counts[lst] = np.int32(n)
    return keep, counts, lst[keep].astype(np.int32)


# ---- quantize36 -----------------------------------------------------------------------------------------------------------------
def quantize36(x):
    """(x + 98304.0) - 98304.0: the float trick, as tor_device.hpp writes it."""
    return I.q36(x)


def quantize36_exact(x):
    """The rational statement, for one finite |x| < 2^15: the nearest multiple of 2^-36, ties to the even multiple."""
    assert abs(x) < 2.0 ** 15
    f = Fraction(float(x)) * 2 ** 36
    k = f.numerator // f.denominator                                        # floor
    rest = f - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k % 2 == 1):
        k += 1
    return float(Fraction(k, 2 ** 36))                                      # |k| < 2^51: exact


# ---- the math self-test's op 6 ----------------------------------------------------------------------------------------------------
def unit_vector_probe(x, y):
    """tor_kernels.hpp selftest_math_one op 6 over tor_device.hpp: u = unit_vector((x, y, 0.5)) = a * (1.0 / sqrt(len2(a))) -- the
    reciprocal once, then three multiplications (div_s, vec3s.nim:93-94), not three divisions --, len2 and dot summed left to right,
    every operation one rounding -> (u . (1, 2, 3), u.x)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        len2 = x * x + y * y + 0.5 * 0.5
        inv = 1.0 / np.sqrt(len2)
        ux, uy, uz = x * inv, y * inv, 0.5 * inv
        return ux * 1.0 + uy * 2.0 + uz * 3.0, ux
