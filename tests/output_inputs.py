"""Named, seeded inputs of the output-stage sweep (tests/test_output_stage.py, tests/test_gpu_output_stage.py): the kernels of
csrc/kernel/output_stage.hpp, the shared math of csrc/tor_math.hpp and quantize36 of tor_device.hpp, fed what a well-behaved small
render never produces.  Synthetic throughout, numpy only; every function returns the same arrays on every call.

values(name)        the value domain of resolve, the quantiser and pow: unit, lit, tiny, steps, wild
GAMMAS              the float32 gamma fields; tor_resolve_device bounds none (valid_options and the canvas checks read no gamma), so
                    the smallest one is 1e-6: y = 1 / gamma lands just under 2^20, the edge of pow_pos's stated domain
SIZES               n_values of the element-wise kernels: empty, one thread, one block less / exactly / more than one, three blocks + 3
noise_case          sums and moments of n samples as accumulations leave them (multiples of 2^-36 below 2^17, M - S^2/n sometimes just
                    below 0), npix from one pixel across the 1024-block cap of launch_accum_noise to the 1920 x 1080 frame
select_cases        pixel lists over such sums, with the wild pixels, repeated pixels and the degenerate tolerances
COUNTS, counts_strip sample counts inside and outside tor_resolve_counts_device's [1, 2^17]
FRAMES, frame       encoder frames smaller than a macroblock in either direction, with padding in one and in both directions
sincos_arguments    the arguments the error budget of sincos_2pi_fast names as worst, and the slow path's [6.2890625, 8).  The contract
                    of sincos_2pi_slow (its comment, and the oracle's guard) is 0 <= a < 8: nothing here is negative, NaN or >= 8
quantize36_inputs   ties, their neighbours, the coarser grid from 2^15 on, negatives and the wild values"""
import zlib
from fractions import Fraction

import numpy as np

SEED = 20261020
INT32_MAX = 2 ** 31 - 1
Q36 = 98304.0                                            # 1.5 * 2^16: ulp = 2^-36


def _rng(*key):
    return np.random.default_rng([SEED] + [zlib.crc32(str(k).encode()) for k in key])


def q36(x):
    """quantize36 in numpy (the float trick; tests/output_restatement.py checks it against the rational statement)"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, dtype=np.float64) + Q36) - Q36


def _bits(u):
    return np.array(u, dtype=np.uint64).view(np.float64)


def _around(x):
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


NAN_POS, NAN_NEG, NAN_PAYLOAD = 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF80000DEADBEEF
WILD = np.concatenate([_bits([NAN_POS, NAN_NEG, NAN_PAYLOAD]),
                       np.array([np.inf, -np.inf, -0.0, -1e-300, -1.0] + _around(2.0 ** 1000) + [np.finfo(np.float64).max])])
WILD.setflags(write=False)
VALUE_SETS = ("unit", "lit", "tiny", "steps", "wild")


def values(name):
    """float64 (n,), read-only."""
    rng = _rng("values", name)
    if name == "unit":
        v = rng.random(4096)
    elif name == "lit":
        v = np.concatenate([[1.0, 2.0 ** 17], 2.0 ** rng.uniform(0.0, 17.0, 4094)])
    elif name == "tiny":
        sub = 5e-324 * np.array([1.0, 2.0, 3.0, 2.0 ** 20, 2.0 ** 44, 2.0 ** 51, 2.0 ** 52 - 1.0])      # subnormals, exact
        v = np.concatenate([sub, _around(2.0 ** -1022), [2.0 ** -1030, 2.0 ** -1023.5], 2.0 ** rng.uniform(-1074.0, -1022.0, 1012)])
    elif name == "steps":
        k = np.arange(257) / 256.0
        v = np.concatenate([np.nextafter(k, -np.inf), k, np.nextafter(k, np.inf), _around(0.999), [1.0]])
    elif name == "wild":
        v = WILD.copy()
    else:
        raise KeyError(name)
    v = np.ascontiguousarray(v, dtype=np.float64)
    v.setflags(write=False)
    return v


GAMMAS = tuple(float(np.float32(g)) for g in (2.2, 1.0, 1.8, 2.4, 0.5, 1e-6))
SIZES = (0, 1, 3, 255, 256, 257, 3 * 257)
TOTALS = (1, 3, 131072)                                   # total_samples of tor_resolve_device: scale 1, 1/3 (rounded), 2^-17


def exponent_of(gamma):
    """The y of pow(x, y) that the library hands its kernels for a float gamma field (tor_api.cpp: 1.0 / (double)gamma_correction)."""
    return 1.0 / float(np.float32(gamma))


# ---- noise --------------------------------------------------------------------------------------------------------------------
NOISE_BLOCK, NOISE_MAX_BLOCKS = 256, 1024                 # accum_noise_kernel's block, launch_accum_noise's kNoiseMaxBlocks
NOISE_NPIX = (1, 255, 256, 257, 262143, 262144, 262145, 262144 + 256 * 3 + 7, 2073600)
NOISE_N = (2, 17, 131072)
_DRAWN = 1 << 23                                          # up to this many pixel-samples the sums are really accumulated


def wild_pixels(npix):
    """{pixel: kind} of the planted pixels: 'nan' (every channel), 'inf' (channel 0), 'clamp' (channel 2: M < S^2/n), or 'all'
    (one kind per channel, for frames too small to hold three apart) -- in the first block, the last block, and, where a grid of
    1024 blocks strides, in the second round's tail."""
    if npix < 16:
        return {0: "all", npix - 1: "all"}
    out = {}
    bases = [2, npix - 9] + ([NOISE_MAX_BLOCKS * NOISE_BLOCK + 3] if npix >= NOISE_MAX_BLOCKS * NOISE_BLOCK + 16 else [])
    for b in bases:
        out.update({b: "nan", b + 1: "inf", b + 2: "clamp"})
    return out


_noise_cache = {}


def noise_case(npix, n, wild=False):
    """(S, M), both (npix, 3) float64, read-only.  One pixel in eight is flat (every sample the same colour c): its M - S^2/n is
    n (quantize36(c^2) - c^2) and a rounding, negative about half the time.  For n <= 17 and up to 2^23 pixel-samples the n draws are made
    and summed as the accumulation kernels sum them (S += q, M += quantize36(q q), q = quantize36(draw)); beyond that S = n c and
    M = n quantize36(c^2) + quantize36(n v) with a per-channel variance v, the same grid and the same range."""
    key = (npix, n, wild)
    if key in _noise_cache:
        return _noise_cache[key]
    rng = _rng("noise", npix, n)
    c = q36(0.9 * rng.random((npix, 3)))                 # (below 0.9: c^2 + v < 1, so M stays below n as a sum of squares <= 1 does)
    flat = (rng.random(npix) < 0.125)[:, None]
    if n <= 17 and n * npix <= _DRAWN:
        S, M = np.zeros((npix, 3)), np.zeros((npix, 3))
        for _ in range(n):
            q = q36(np.where(flat, c, np.clip(c + 0.3 * (rng.random((npix, 3)) - 0.5), 0.0, 1.0)))
            S += q
            M += q36(q * q)
    else:
        v = np.where(flat, 0.0, 0.02 * rng.random((npix, 3)))
        S = n * c
        M = n * q36(c * c) + q36(n * v)
    on_grid = lambda a: bool((a * 2.0 ** 36 == np.floor(a * 2.0 ** 36)).all())      # (a 2^36 < 2^53: exact)
    assert S.max() <= 2.0 ** 17 and M.max() <= 2.0 ** 17 and on_grid(S) and on_grid(M)
    if wild:
        for p, kind in wild_pixels(npix).items():
            if kind in ("nan", "all"):
                ch = slice(None) if kind == "nan" else 1
                S[p, ch] = M[p, ch] = np.nan
            if kind in ("inf", "all"):
                S[p, 0] = M[p, 0] = np.inf
            if kind in ("clamp", "all"):
                S[p, 2] = n * 0.5
                M[p, 2] = n * 0.25 - 2.0 ** -10           # S^2/n = n/4 exactly: the variance is -2^-10 / (n - 1)
    S.setflags(write=False)
    M.setflags(write=False)
    if npix <= 4096:                                     # (the large ones are cheaper to make again than to keep)
        _noise_cache[key] = (S, M)
    return S, M


# ---- select -------------------------------------------------------------------------------------------------------------------
SELECT_NPIX, SELECT_N, SELECT_TILE = 2600, 17, 1024       # kSelTile
SELECT_LENGTHS = (1, 1023, 1025)
SELECT_REPEATED = 2 * SELECT_TILE + 37                    # a list with repeated pixels: three tiles, the last one of 37 entries


def select_cases():
    """[(name, S, M, list int32, n, abs_tol, rel_tol)] over one wild noise case.  `mixed` tolerances sit at the median error of the
    frame, so that about half of every tile converges; (0, 0) keeps whatever has any error at all; abs_tol = inf drops everything
    whose right-hand side is not NaN."""
    S, M = noise_case(SELECT_NPIX, SELECT_N, wild=True)
    wild = np.array(sorted(wild_pixels(SELECT_NPIX)), dtype=np.int32)
    rng = _rng("select")
    with np.errstate(invalid="ignore"):
        var = np.maximum((M - S * S / SELECT_N) / (SELECT_N - 1.0), 0.0)
    mixed = float(np.nanmedian(np.sqrt(var / SELECT_N).max(axis=1)))
    out = []
    for length in SELECT_LENGTHS + (SELECT_REPEATED,):
        if length == 1:
            lists = {"one_nan": wild[:1], "one_plain": np.array([7], dtype=np.int32)}
        elif length == SELECT_REPEATED:
            body = rng.integers(0, 300, length).astype(np.int32)            # 300 pixels drawn 2085 times: every one repeated
            body[[0, 5, SELECT_TILE - 1, SELECT_TILE, 2 * SELECT_TILE + 1, length - 1]] = wild[[0, 1, 2, 3, 4, 5]]
            lists = {f"repeated_{length}": body}
        else:
            body = np.sort(rng.choice(SELECT_NPIX, length, replace=False)).astype(np.int32)
            body[[0, 1, 2, length - 3, length - 2, length - 1]] = wild[[0, 1, 2, 3, 4, 5]]   # the wild pixels in the first and last tile
            lists = {f"unique_{length}": body}
        for lname, lst in lists.items():
            for tname, (a, r) in (("mixed", (mixed, 0.0)), ("relative", (0.25 * mixed, 0.02)), ("zero", (0.0, 0.0)), ("abs_inf", (np.inf, 0.0)),
                                  ("abs_inf_rel", (np.inf, 0.5))):
                lst = np.ascontiguousarray(lst, dtype=np.int32)
                lst.setflags(write=False)
                out.append((f"{lname}/{tname}", S, M, lst, SELECT_N, float(a), float(r)))
    return out


# ---- counts -------------------------------------------------------------------------------------------------------------------
COUNTS = (0, -1, 1, 2, 3, 131072, INT32_MAX)
COUNTS_NPIX = (0, 1, 85, 86, 257)                         # n_values = 3 npix: 0, 3, 255, 258, 771


def counts_strip(npix=257):
    c = _rng("counts").permutation(np.resize(np.array(COUNTS, dtype=np.int32), 257))[:npix]
    return np.ascontiguousarray(c, dtype=np.int32)


# ---- encoder ------------------------------------------------------------------------------------------------------------------
FRAMES = ((2, 2), (2, 34), (18, 2), (16, 16), (34, 18), (32, 48))          # (rows, columns)
FRAME_CONTENTS = ("primaries", "primaries_fine", "steps", "uniform", "wild")
PRIMARIES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=np.float64)


def frame(h, w, content):
    """(h, w, 3) float64 canvas, row 0 = bottom scanline, read-only.  `primaries`: the six saturated colours in 2 x 2 checkers (every
    chroma sample sees one colour: tU and tV at their extremes, negative for half of them); `primaries_fine`: the same per pixel
    (every chroma sample averages four colours).  `wild`: uniform with every value of WILD somewhere -- the first ones in canvas row 0,
    the video's LAST row, and in the last column: what the padding of a partial macroblock replicates."""
    rng = _rng("frame", h, w, content)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if content == "primaries":
        px = PRIMARIES[((i // 2) * 5 + (j // 2)) % 6]
    elif content == "primaries_fine":
        px = PRIMARIES[(i * 5 + j) % 6]
    elif content == "steps":
        px = np.resize(values("steps"), h * w * 3).reshape(h, w, 3)
    elif content == "uniform":
        px = rng.uniform(-0.1, 1.1, (h, w, 3))
    elif content == "wild":
        px = rng.uniform(-0.1, 1.1, (h, w, 3))
        flat = px.reshape(-1)                                              # (a view)
        k = min(len(WILD), flat.size)
        spots = np.concatenate([[(w - 1) * 3, ((h - 1) * w + w - 1) * 3 + 1, 2],      # row 0 last column; last row last column; row 0 first
                                rng.permutation(flat.size)])
        _, first = np.unique(spots, return_index=True)
        spots = spots[np.sort(first)][:k]
        flat[spots] = WILD[:k]
    else:
        raise KeyError(content)
    px = np.ascontiguousarray(px, dtype=np.float64)
    px.setflags(write=False)
    return px


# ---- math arguments -----------------------------------------------------------------------------------------------------------
PI = Fraction(3141592653589793238462643383279502884197169399375105820974944592, 10 ** 63)
SINCOS_FAST_END = 6.2890625                               # sincos_2pi_fast: a < 6.2890625 (j <= 256)
SINCOS_SLOW_END = 8.0                                     # sincos_2pi_slow: 0 <= a < 8


def _ulps_around(centres, reach=64):
    """Every double within `reach` ulps of each centre (>= 0), nothing below 0."""
    b = np.asarray(centres, dtype=np.float64).view(np.int64)[:, None] + np.arange(-reach, reach + 1, dtype=np.int64)[None, :]
    return b[b >= 0].view(np.float64)


def sincos_arguments():
    """float64 (n,), every one in [0, 8) (-0.0 included: the fast path's `a >= 0.0` takes it)."""
    nodes = np.array([float(Fraction(j) * PI / 128) for j in range(257)])
    halves = np.array([float((Fraction(j) + Fraction(1, 2)) * PI / 128) for j in range(257)])
    rng = _rng("sincos")
    a = np.concatenate([_ulps_around(nodes), _ulps_around(halves), _ulps_around([float(2 * PI)]),
                        [np.nextafter(SINCOS_FAST_END, 0.0), SINCOS_FAST_END, np.nextafter(SINCOS_SLOW_END, 0.0), -0.0, 2.0 ** -1022, 1e-300],
                        rng.uniform(SINCOS_FAST_END, SINCOS_SLOW_END, 4000), rng.uniform(0.0, SINCOS_FAST_END, 4000)])
    a = a[(a < SINCOS_SLOW_END)]
    a.setflags(write=False)
    return a


def quantize36_inputs():
    """float64 (n,): ties (2k + 1) 2^-37 for small and large k with both neighbours, the range [2^15, 2^17) where the grid of
    x + 98304 coarsens (131072 - 98304 = 32768 and its neighbours: the binade edge of the sum), negatives of all of it, the wild values."""
    rng = _rng("quantize36")
    k = np.concatenate([np.arange(0, 40), 2 ** np.arange(6, 51), 2 ** np.arange(6, 51) + 1, rng.integers(0, 2 ** 51, 400)]).astype(np.float64)
    ties = (2.0 * k + 1.0) * 2.0 ** -37                                    # exact: 2k + 1 < 2^53
    ties = ties[ties < 2.0 ** 15]
    edge = 131072.0 - 98304.0
    big = np.concatenate([_around(edge), _around(2.0 ** 15 + 2.0 ** -36), _around(2.0 ** 15 + 3 * 2.0 ** -36), _around(2.0 ** 16),
                          [np.nextafter(2.0 ** 17, 0.0)], rng.uniform(2.0 ** 15, 2.0 ** 17, 400)])
    pos = np.concatenate([np.nextafter(ties, -np.inf), ties, np.nextafter(ties, np.inf), big, rng.random(400) * 2.0, values("tiny")[:16]])
    x = np.concatenate([pos, -pos, WILD, [0.0]])
    x.setflags(write=False)
    return x
