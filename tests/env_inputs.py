"""Shared inputs of the environment-light tests (test_env_query.py on the CPU, test_gpu_env_query.py on the GPU): octahedral maps,
points with generator states, and directions -- the smallest shapes at which the kernels of tor_env.hip can still go wrong.

Maps (MAPS): n = 1 (no search at all), 2, 5 (not a power of two), 64 (whole rows of importance 0, isolated zero texels, one texel
-- the "sun" -- holding almost all of the importance, values from 1e-200 to 1e200 with finite sums), 64 again with a sun of nine
tenths (so that the picks still spread over the map), 257 (one more than a block's threads, and a last group of ONE running sum),
`dyadic4` (a caller importance of small integers, so that a crafted draw times a running sum IS a running sum, and a first row
whose only importance is the smallest denormal) and `tiny2` (every importance denormal: the total itself is 2^-1074).

Points (points_and_states): 3 * 64 + 8 -- three full waves and a partial one --, the last eight with crafted states.  xoshiro256+'s
output is s0 + s3 and the next state's s0' = s0 ^ s3 ^ s1, s3' = rotl(s3 ^ s1, 45), so
    (2^63, 0, w, 0)             draws u0 = u1 = 0.5              (a tie against a dyadic running sum: `>` against `>=`)
    (2^64 - 1, w, w', 0)        draws the largest u0 = 1 - 2^-52
    (0, 0x5555.., w, 0)         draws u0 = 0 and the largest u1  (0x5555.. + rotl(0x5555.., 45) = 2^64 - 1)
    (0, 0, w, 0)                draws u0 = u1 = 0                (the first texel of positive importance)
The largest draw times a DENORMAL sum rounds to the sum itself, so no running sum is above it: the fallbacks."""
import numpy as np

MAPS = ("n1", "n2", "n5", "n64", "n64soft", "n257", "dyadic4", "tiny2")
N_POINTS = 3 * 64 + 8
TINY = 2.0 ** -1074
SUN64 = (41, 23)                                                         # (row, col) of the sun of the 64 x 64 maps
CRAFTED = {"half": -8, "half_b": -7, "max0": -6, "max0_b": -5, "zero_max": -4, "zero_max_b": -3, "zero": -2, "nan": -1}


def _random_rgb(n, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(0.05, 1.0, size=(n, n, 3))


def env_map(name):
    """(rgb (n, n, 3), importance (n, n) or None)."""
    if name == "n1":
        return np.array([[[0.3, 0.5, 0.9]]]), None
    if name == "n2":
        return _random_rgb(2, 2), None
    if name == "n5":
        rgb = _random_rgb(5, 5)
        rgb[2, 3] = 0.0                                                   # an isolated zero texel
        return rgb, None
    if name in ("n64", "n64soft"):
        rgb = _random_rgb(64, 64)
        rgb[0] = 0.0                                                      # whole rows of importance 0: the first, two inside, the last
        rgb[17:19] = 0.0
        rgb[63] = 0.0
        rgb[5, 0:3] = 0.0                                                 # zero texels at the start and at the end of a row, and isolated ones
        rgb[9, 61:64] = 0.0
        rgb[np.arange(20, 60, 7), np.arange(3, 43, 7)] = 0.0
        rgb[30, 10:12] *= 1e-200                                          # the small end of the range (still > 0)
        if name == "n64":
            rgb[SUN64] = (1e200, 0.9e200, 0.7e200)
        else:
            lum = (0.2126 * rgb[:, :, 0] + 0.7152 * rgb[:, :, 1]) + 0.0722 * rgb[:, :, 2]
            rgb[SUN64] = np.array([1.0, 0.9, 0.7]) * (9.0 * lum.sum() / 0.9)   # about nine tenths of the importance
        return rgb, None
    if name == "n257":
        rgb = _random_rgb(257, 257)
        rgb[100] = 0.0
        rgb[256, 256] = 0.0                                               # the last group of the last row: one texel, importance 0
        rgb[200, 250:257] = 0.0
        return rgb, None
    if name == "dyadic4":
        # S_0 = 2^-1074, and its last texel of positive importance is column 1
        imp = np.array([[0.0, TINY, 0.0, 0.0], [2.0, 2.0, 2.0, 2.0], [1.0, 1.0, 1.0, 1.0], [0.0, 3.0, 1.0, 0.0]])
        return _random_rgb(4, 4), imp                                     # M = (2^-1074, 8, 12, 16)
    if name == "tiny2":
        return _random_rgb(2, 22), np.array([[TINY, 0.0], [0.0, 0.0]])    # T = 2^-1074; the last row with S_r > 0 is row 0
    raise KeyError(name)


def points_and_states(seed=0xE27):
    """((N_POINTS, 4) float64 {x, y, z, time}, (N_POINTS, 4) uint64 xoshiro256+ states): random ones, then the crafted states
    (CRAFTED names their rows, counted from the end); the last point has a NaN coordinate."""
    rs = np.random.RandomState(seed)
    pts = np.empty((N_POINTS, 4))
    pts[:, 0:3] = rs.normal(scale=3.0, size=(N_POINTS, 3))
    pts[:, 3] = rs.uniform(0.0, 1.0, size=N_POINTS)
    w = rs.randint(0, 1 << 32, size=(N_POINTS, 4, 2), dtype=np.int64).astype(np.uint64)
    st = (w[:, :, 0] << np.uint64(32)) | w[:, :, 1] | np.uint64(1)
    ones, fives = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x5555555555555555)
    for name, row in CRAFTED.items():
        if name.startswith("half"):
            st[row, 0], st[row, 1], st[row, 3] = np.uint64(1 << 63), 0, 0
        elif name.startswith("max0"):
            st[row, 0], st[row, 3] = ones, 0
        elif name.startswith("zero_max"):
            st[row, 0], st[row, 1], st[row, 3] = 0, fives, 0
        elif name == "zero":
            st[row, 0], st[row, 1], st[row, 3] = 0, 0, 0
    pts[-1, 0] = np.nan
    return pts, st


def directions(sampled=None, seed=0xD1):
    """(m, 7) rays whose directions are the evaluation's cases: the six axes, the fold lines |s| + |t| = 1 (y = 0), s = 0 and
    t = 0, the four corners (straight down, told apart by the signs of two zeros), -0.0 in y, random directions of any length,
    then the unusable ones (UNUSABLE rows, counted from the end: zero, NaN, infinite, an L1 that overflows) after a denormal
    that IS usable -- and every direction of `sampled` ((k, 3), the sample tests' directions) in front."""
    rs = np.random.RandomState(seed)
    d = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
         (1, 0, 1), (0.3, 0, -0.7), (-0.25, 0.0, 0.75), (-3, 0, -1), (0.5, -0.0, 0.5), (-2.0, -0.0, 6.0),     # the fold: y = +-0
         (0, 0.4, 0.6), (0, -0.4, 0.6), (0.0, 2.0, -1.0), (-0.0, -2.0, -1.0),                                    # s = 0
         (0.6, 0.4, 0), (-0.6, -0.4, 0), (1.0, 3.0, -0.0), (-1.0, -3.0, -0.0),                                   # t = 0
         (0.0, -1.0, 0.0), (-0.0, -1.0, 0.0), (0.0, -1.0, -0.0), (-0.0, -1.0, -0.0),                             # the four corners
         (0.3, -0.0, 0.4), (-0.3, -0.0, -0.4), (0.25, 0.5, 0.25), (0.25, -0.5, 0.25),
         (5e-324, 0.0, 0.0), (1e-310, -2e-310, 3e-310)]                                                          # denormals: usable
    v = rs.normal(size=(64, 3)) * 10.0 ** rs.uniform(-3, 3, size=(64, 1))
    bad = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (np.nan, 1.0, 0.0), (1.0, 0.0, np.nan), (np.inf, 1.0, 1.0), (1.0, -np.inf, 0.0),
           (1e308, 1e308, 1e308), (-1.7e308, 1.0, 1e308)]
    parts = ([] if sampled is None else [np.asarray(sampled, dtype=np.float64).reshape(-1, 3)]) + [np.array(d, dtype=np.float64), v,
                                                                                                  np.array(bad, dtype=np.float64)]
    dirs = np.concatenate(parts)
    rays = np.zeros((len(dirs), 7))
    rays[:, 0:3] = rs.normal(size=(len(dirs), 3))
    rays[:, 3:6] = dirs
    rays[:, 6] = 0.5
    return rays


N_UNUSABLE = 8
_cases = {}


def case(oracle, name):
    """Map `name` with its table, the points and states, the restatement's samples, the direction set (the sampled directions
    in front) and the restatement's evaluation of it: computed once, shared by both test files, never changed."""
    import env_restatement as ER
    if name not in _cases:
        rgb, imp = env_map(name)
        tab = ER.table(rgb, imp)
        pts, st = points_and_states()
        res = ER.sample(oracle, tab, pts, st)
        rays = directions(res["rays"][:, 3:6])
        _cases[name] = dict(rgb=rgb, imp=imp, tab=tab, pts=pts, st=st, res=res, dirs=rays, ev=ER.evaluate(tab, rays))
    return _cases[name]


# ---- the frame of the trace_environment tests: an open scene under a sky with a small sun ------------------------------------------
LAMB, METAL = 0.0, 1.0


def _sphere(c, r, mat=LAMB, albedo=(0.5, 0.5, 0.5), fuzz=0.0, ri=1.5):
    return [0.0, c[0], c[1], c[2], 0.0, 0.0, 0.0, 0.0, 0.0, r, mat, albedo[0], albedo[1], albedo[2], fuzz, ri]


def open_scene():
    """A ground sphere and one diffuse sphere, as flat (n, 16) records."""
    return np.array([_sphere((0.0, -100.5, -1.0), 100.0, LAMB, (0.6, 0.6, 0.5)), _sphere((0.0, 0.0, -1.0), 0.5, LAMB, (0.7, 0.4, 0.3))])


def sun_sky(dirs, sun=(0.4, 0.8, 0.45), cos_width=0.995, sun_rgb=(400.0, 360.0, 300.0)):
    """The reference's gradient (render.nim:41-44) plus a sun: rgb (..., 3) for unit directions (..., 3)."""
    dirs = np.asarray(dirs, dtype=np.float64)
    t = 0.5 * dirs[..., 1] + 1.0
    rgb = (1.0 - t)[..., None] * np.array([1.0, 1.0, 1.0]) + t[..., None] * np.array([0.5, 0.7, 1.0])
    s = np.asarray(sun) / np.sqrt((np.asarray(sun) ** 2).sum())
    inside = (dirs * s).sum(axis=-1) > cos_width
    return np.where(inside[..., None], np.array(sun_rgb), np.clip(rgb, 0.0, None))
