"""The synthetic inputs of tests/test_gpu_deposit.py, and what tests/test_deposit.py measures on them from the restatement alone.

N = 64 * 9 + 37 entries (nine full waves and a ragged one, three workgroups of 256) into NPIX = 50 pixels.  Colours are drawn in
[0, 1.5 * min(max_value, 1)): with max_value <= 1 a third of the channels clamp; with max_value = 128 only the value cases reach
the clamp, which keeps every pixel inside the exactness bound (8 accepted samples of 128 are all a pixel may hold; the restatement
asserts its own sums).  A quarter of the channels are exact ties (j + 0.5) * 2^-36."""
import numpy as np

N = 64 * 9 + 37
NPIX = 50
MAX_VALUES = (0.25, 1.0, 128.0)
RUN_LENGTHS = (1, 2, 63, 64, 65, 300)        # sorted runs: they cross the lane-64 and the workgroup-256 boundaries
CASES = ("runs", "abab", "aabb", "one", "uniform", "edges", "rejects", "values")
INT32_MIN = -2 ** 31
UNIT = 2.0 ** -36


def value_cases(max_value):
    """The hand-worked values of tests/test_deposit.py as (8, 3) colours: ties, -0.0, a denormal, the clamp's edge, a huge value."""
    mv = float(max_value)
    return np.array([[0.5 * UNIT, 1.5 * UNIT, 2.5 * UNIT],              # ties round to even: 0, 2, 2 units
                     [-0.0, 0.0, -0.0],
                     [5e-324, 2.0 ** -1030, 0.25 * UNIT],                 # denormals and a quarter unit: 0
                     [mv, np.nextafter(mv, np.inf), np.nextafter(mv, 0.0)],
                     [1e300, 0.0, mv * 0.5],
                     [3.5 * UNIT, 0.75 * UNIT, UNIT],
                     [mv * 0.999, mv * 1.001, 0.0],
                     [np.finfo(np.float64).max, mv, 0.125 * mv]], dtype=np.float64)


def colors_of(rng, n, max_value):
    top = 1.5 * min(float(max_value), 1.0)
    c = rng.uniform(0.0, top, size=(n, 3))
    tie = rng.random((n, 3)) < 0.25
    j = np.floor(rng.uniform(0.0, top, size=(n, 3)) * 2.0 ** 36)
    return np.where(tie, (j + 0.5) * UNIT, c)


def reject_colors(c, rows, rng):
    """Make the listed rows rejects: NaN, +inf, -inf, a negative denormal, -1 in one channel each, the other channels kept."""
    kinds = (np.nan, np.inf, -np.inf, -5e-324, -1.0)
    for m, r in enumerate(rows):
        c[r, int(rng.integers(3))] = kinds[m % len(kinds)]
    return c


def case(name, max_value, seed=5):
    """(colors (N, 3) float64, pixels (N,) int32) of one input case."""
    rng = np.random.default_rng([seed, CASES.index(name), int(max_value * 4)])
    c = colors_of(rng, N, max_value)
    if name == "runs":
        p = rng.integers(0, NPIX, size=N)
        at = 0
        for m, ln in enumerate(RUN_LENGTHS):
            p[at:at + ln] = m * 7 + 3            # neighbouring runs hold different pixels
            at += ln
    elif name == "abab":                         # A B A B ...: every lane a run of its own, two pixels
        p = np.where(np.arange(N) % 2 == 0, 7, 11)
    elif name == "aabb":                         # A A B B A A B B ...: runs of two on two pixels
        p = np.where((np.arange(N) // 2) % 2 == 0, 7, 11)
    elif name == "one":
        p = np.full(N, 13)
    elif name == "uniform":
        p = rng.integers(0, NPIX, size=N)
    elif name == "edges":                        # pixels outside the film among runs of four: they break the runs
        p = (np.arange(N) // 4) % NPIX
        out = rng.random(N) < 0.2
        p = np.where(out, rng.choice([-1, NPIX, INT32_MIN, NPIX + 7, 2 ** 31 - 1], size=N), p)
    elif name == "rejects":
        # runs of 24 on one pixel; by turns the head, the middle, the tail of a run is rejected, and a whole run of 8 between two
        # runs of the same pixel
        p = (np.arange(N) // 24) % NPIX
        rows = []
        for g in range(N // 24):
            b = 24 * g
            rows += [[b], [b + 11, b + 12], [b + 23], list(range(b + 8, b + 16))][g % 4]
        c = reject_colors(c, rows, rng)
    elif name == "values":                       # every value case five times, one pixel each; the rest ordinary
        p = rng.integers(0, NPIX, size=N)
        v = value_cases(max_value)
        for rep in range(5):
            at = 70 * rep + 60                   # (they straddle lanes 60 .. 67 of the first waves)
            c[at:at + len(v)] = v
            p[at:at + len(v)] = (np.arange(len(v)) + 8 * rep) % NPIX
    else:
        raise KeyError(name)
    return np.ascontiguousarray(c), np.ascontiguousarray(p, dtype=np.int32)


def list_cases(seed=9):
    """{name: index list (int32)} over N entries: a subset, duplicates, entries out of range, an empty list, gaps inside a wave."""
    rng = np.random.default_rng(seed)
    sub = np.sort(rng.choice(N, size=N // 3, replace=False))
    gaps = np.arange(N, dtype=np.int64)
    gaps[rng.random(N) < 0.3] = N + 5           # dead lanes between live ones: they split the runs of a sorted input
    return {"subset": sub, "shuffled subset": rng.permutation(sub), "duplicates": np.concatenate([sub[:64], sub[:64], np.repeat(sub[5], 70)]),
            "out of range": np.concatenate([[-1, N, INT32_MIN, 2 ** 31 - 1], sub[:40], [N + 1, -7], sub[40:90]]),
            "empty": np.zeros(0, dtype=np.int64), "gaps": gaps}


def shares(max_value=1.0):
    """What the cases exercise, over all of them, by the definition alone: the share of deposited lanes that sit in a run longer
    than 1 (adjacent accepted lanes of one wave with one pixel), of rejected samples, of pixels outside the film, of tied channels."""
    in_run = dep = rej = out = tie = chan = total = 0
    for name in CASES:
        c, p = case(name, max_value)
        inside = (p >= 0) & (p < NPIX)
        with np.errstate(invalid="ignore"):
            bad = (np.isnan(c) | np.isinf(c) | (c < 0.0)).any(axis=1)
        live = inside & ~bad
        same = live[1:] & live[:-1] & (p[1:] == p[:-1]) & ((np.arange(1, N) % 64) != 0)   # lane i continues lane i - 1's run
        member = np.zeros(N, dtype=bool)
        member[1:] |= same
        member[:-1] |= same
        in_run += int(member.sum())
        dep += int(live.sum())
        rej += int((inside & bad).sum())
        out += int((~inside).sum())
        cl = np.minimum(c[live], max_value) * 2.0 ** 36
        tie += int((cl - np.floor(cl) == 0.5).sum())
        chan += cl.size
        total += N
    return {"in_run": in_run / dep, "rejected": rej / total, "outside": out / total, "ties": tie / chan}
