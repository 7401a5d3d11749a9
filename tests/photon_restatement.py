"""The definition of the photon-map queries (include/tor_photons.h), restated in numpy from the header's text -- what
tests/test_gpu_photon_query.py compares the kernels with, bit for bit, and what tests/test_photon_query.py holds to hand-worked cases.

  store()        the map a build keeps: the valid listed photons with their cells and buckets, the dropped count, the bucket count
  gather()       float64: brute force over ALL stored photons, the quantiser as (x + 98304.0) - 98304.0
  gather_int()   integers: rint(min(power * w, max_value) * 2^36) summed as int64, scaled back by 2^-36 -- no float64 sum at all
  walk()         the 27-cell walk of the grid, as the header describes it, for the coverage statistics of tests/photon_inputs.py

Neither gather knows of cells or buckets: the grid is an acceleration and has no say in the answer.  Both assert the exactness bound
count * max_value < 2^17, so inputs that pass are inside it by the reference statement alone; agree() asserts equal bits."""
import numpy as np

BIAS = 98304.0          # 1.5 * 2^16: ulp(x + BIAS) = 2^-36 for 0 <= x < 2^15
UNIT = 2.0 ** -36
SUM_BOUND = 2.0 ** 17
MAX_VALUE = 128.0
CELL_MAX = 2 ** 30
KERNELS = {"constant": 0, "epanechnikov": 1}


def quantize36(x):
    x = np.asarray(x, dtype=np.float64)
    return (x + BIAS) - BIAS


def cell_size(radius):
    r = np.float64(radius)
    return r + r * np.float64(2.0 ** -20)       # two roundings


def cells(points, h):
    """floor(p / h) per axis, as float64 (out of range, infinite and NaN values stay what they are)."""
    with np.errstate(all="ignore"):
        return np.floor(np.asarray(points, dtype=np.float64).reshape(-1, 3) / np.float64(h))


def n_buckets(n_list):
    want, nb = 2 * max(int(n_list), 1), 16
    while nb < want and nb < 2 ** 26:
        nb *= 2
    return nb


def bucket(cell, nb):
    """The documented hash of int cells (m, 3), in wrapping 32-bit arithmetic."""
    c = np.asarray(cell, dtype=np.int64).reshape(-1, 3) & 0xFFFFFFFF
    m = 0xFFFFFFFF
    hx, hy, hz = (c[:, 0] * 73856093) & m, (c[:, 1] * 19349663) & m, (c[:, 2] * 83492791) & m
    return (hx ^ hy ^ hz) & (nb - 1)


def _entries(n, index):
    if index is None:
        return np.arange(n, dtype=np.int64)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    return index[(index >= 0) & (index < n)]      # a listed entry outside [0, n) is skipped; a repeated one stays


def store(positions, powers, directions, radius, index=None):
    """The map of a build: {"position", "power", "direction" (None without), "cell" int64, "bucket", "dropped", "n_buckets",
    "largest", "R", "h"} -- the stored photons in list order (the library's order inside a bucket is not defined)."""
    R = np.float64(radius)
    h = cell_size(R)
    assert np.isfinite(R) and R > 0 and np.isfinite(h)
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    pw = np.asarray(powers, dtype=np.float64).reshape(-1, 3)
    dr = None if directions is None else np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    n_list = len(pos) if index is None else int(np.asarray(index).size)
    e = _entries(len(pos), index)
    pos, pw = pos[e], pw[e]
    dr = None if dr is None else dr[e]
    c = cells(pos, h)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(pos).all(axis=1) & np.isfinite(pw).all(axis=1) & (pw >= 0.0).all(axis=1)      # (-0.0 >= 0.0: passes)
        if dr is not None:
            ok &= np.isfinite(dr).all(axis=1)
        ok &= (np.abs(c) <= CELL_MAX).all(axis=1)                                                      # (NaN fails)
    nb = n_buckets(n_list)
    cell = c[ok].astype(np.int64)
    b = bucket(cell, nb)
    return {"position": pos[ok], "power": pw[ok], "direction": None if dr is None else dr[ok], "cell": cell, "bucket": b,
            "dropped": int((~ok).sum()), "n_buckets": nb, "largest": int(np.bincount(b, minlength=1).max()) if len(b) else 0,
            "R": R, "h": h}


def info(m):
    return {"stored": len(m["position"]), "dropped": m["dropped"], "n_buckets": m["n_buckets"], "largest_bucket": m["largest"]}


def _radius2(m, n, radius):
    """(usable, r2) per point: r = radius or R; !(r >= 0) accepts nothing; r = min(r, R); r2 = r * r."""
    r = np.full(n, m["R"]) if radius is None else np.broadcast_to(np.asarray(radius, dtype=np.float64), (n,)).copy()
    with np.errstate(invalid="ignore"):
        usable = r >= 0.0
        r = np.where(r < m["R"], r, m["R"])
    return usable, r * r


def _pairs(m, points, normals, radius, kernel, max_value, chunk=128):
    """Per chunk of points: (rows, accepted (rows, stored) bool, clamped weighted powers (rows, stored, 3))."""
    assert 0.0 < max_value <= MAX_VALUE
    k = KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
    assert k in (0, 1)
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    nrm = None if normals is None else np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    assert nrm is None or m["direction"] is not None, "normals need a map with directions"
    usable, r2 = _radius2(m, len(x), radius)
    p, pw, dr = m["position"], m["power"], m["direction"]
    for lo in range(0, len(x), chunk):
        rows = np.arange(lo, min(lo + chunk, len(x)))
        with np.errstate(all="ignore"):
            e = p[None, :, :] - x[rows, None, :]
            d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            acc = (d2 < r2[rows, None]) & usable[rows, None]
            if nrm is not None:
                dn = (dr[None, :, 0] * nrm[rows, None, 0] + dr[None, :, 1] * nrm[rows, None, 1]) + dr[None, :, 2] * nrm[rows, None, 2]
                acc &= dn < 0.0
            w = 1.0 - d2 / r2[rows, None] if k == 1 else np.ones_like(d2)
            a = pw[None, :, :] * w[..., None]
            a = np.where(a < max_value, a, max_value)
        yield rows, acc, a, d2, r2[rows]


def _start(into, n, index):
    sums = np.zeros((n, 3)) if into is None else np.array(into["sums"], dtype=np.float64).reshape(n, 3)
    count = np.zeros(n, dtype=np.int32) if into is None else np.array(into["count"], dtype=np.int32).reshape(n)
    listed = np.zeros(n, dtype=bool)
    listed[_entries(n, index)] = True             # points that are not listed keep what `into` holds
    return sums, count, listed


def gather(m, points, normals=None, radius=None, kernel="epanechnikov", max_value=1.0, index=None, into=None):
    """{"sums" (n, 3), "count" (n,) int32}: brute force in float64."""
    n = len(np.asarray(points).reshape(-1, 3))
    sums, count, listed = _start(into, n, index)
    for rows, acc, a, _, _ in _pairs(m, points, normals, radius, kernel, max_value):
        q = np.where(acc[..., None], quantize36(a), 0.0)
        s, c = np.zeros((len(rows), 3)), acc.sum(axis=1).astype(np.int32)
        for j in range(q.shape[1]):               # sequentially, in stored order: a float64 sum as a lane forms it
            s += q[:, j, :]
        assert (c * max_value < SUM_BOUND).all(), "the inputs exceed the exactness bound"
        sums[rows] = np.where(listed[rows, None], s, sums[rows])
        count[rows] = np.where(listed[rows], c, count[rows])
    return {"sums": sums, "count": count}


def gather_int(m, points, normals=None, radius=None, kernel="epanechnikov", max_value=1.0, index=None, into=None):
    """gather() in integers: multiples of 2^-36 as int64, summed as int64, scaled back at the end."""
    n = len(np.asarray(points).reshape(-1, 3))
    sums, count, listed = _start(into, n, index)
    for rows, acc, a, _, _ in _pairs(m, points, normals, radius, kernel, max_value):
        with np.errstate(invalid="ignore"):
            qi = np.where(acc[..., None], np.rint(np.where(acc[..., None], a, 0.0) * 2.0 ** 36), 0.0).astype(np.int64)
        si, c = qi.sum(axis=1), acc.sum(axis=1).astype(np.int32)
        assert si.max(initial=0) < 2 ** 53 and (c * max_value < SUM_BOUND).all(), "the inputs exceed the exactness bound"
        sums[rows] = np.where(listed[rows, None], si.astype(np.float64) * UNIT, sums[rows])
        count[rows] = np.where(listed[rows], c, count[rows])
    return {"sums": sums, "count": count}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def mismatches(got, want):
    """The fields of two gathers that differ in any bit (sums compared as int64 words: -0.0 is not 0.0)."""
    bad = []
    if not np.array_equal(bits(got["sums"]).reshape(-1), bits(want["sums"]).reshape(-1)):
        bad.append("sums")
    if not np.array_equal(np.asarray(got["count"]).reshape(-1), np.asarray(want["count"]).reshape(-1)):
        bad.append("count")
    return bad


def agree(m, points, normals=None, radius=None, kernel="epanechnikov", max_value=1.0, index=None, into=None):
    """gather(), after asserting that gather_int() gives the same bits."""
    a = gather(m, points, normals, radius, kernel, max_value, index, into)
    b = gather_int(m, points, normals, radius, kernel, max_value, index, into)
    assert not mismatches(a, b), f"the two statements of the gather disagree: {mismatches(a, b)}"
    return a


def query_cells(points, h):
    """Per point the (27, 3) cells the grid visits and which of them exist: floor(x / h) + {-1, 0, 1}^3, clipped to the range; a
    point with a quotient at or beyond 2^30 + 3 (NaN, infinite) visits none."""
    q = cells(points, h)
    with np.errstate(invalid="ignore"):
        alive = (np.abs(np.asarray(points, dtype=np.float64).reshape(-1, 3) / np.float64(h)) < CELL_MAX + 3).all(axis=1)
    base = np.where(alive[:, None], q, 0.0).astype(np.int64)
    off = np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], dtype=np.int64)
    c = base[:, None, :] + off[None, :, :]
    exists = (np.abs(c) <= CELL_MAX).all(axis=2) & alive[:, None]
    return c, exists


def walk(m, points, normals=None, radius=None, kernel="epanechnikov", max_value=1.0):
    """The grid's walk, restated: per visited cell its bucket's photons, of those the ones stored under that very cell, then the
    brute-force test.  Returns (the gather, statistics): per point `shared` (two distinct visited cells in one bucket),
    `strangers` (photons met in a walked bucket whose cell is not the one asked for and is none of the visited cells, within
    4 R of the point), `twice` (accepted photons whose bucket is walked for more than one cell: a walk that did not compare
    cells would count them again)."""
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n, nb = len(x), m["n_buckets"]
    c, exists = query_cells(x, m["h"])
    out = {"sums": np.zeros((n, 3)), "count": np.zeros(n, dtype=np.int32)}
    shared, strangers, twice = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    by_bucket = {}
    for j, b in enumerate(m["bucket"]):
        by_bucket.setdefault(int(b), []).append(j)
    pieces = list(_pairs(m, x, normals, radius, kernel, max_value, chunk=max(n, 1))) if n else []
    acc, a = (pieces[0][1], pieces[0][2]) if pieces else (None, None)
    for i in range(n):
        visited = [tuple(int(v) for v in c[i, k]) for k in range(27) if exists[i, k]]
        bks = [int(bucket(np.array([v]), nb)[0]) for v in visited]
        shared[i] = len(bks) - len(set(bks))
        vset = set(visited)
        for v, b in zip(visited, bks):
            for j in by_bucket.get(b, ()):
                cj = tuple(int(t) for t in m["cell"][j])
                if cj != v:
                    if cj not in vset:
                        d = m["position"][j] - x[i]
                        strangers[i] += bool(np.sqrt((d * d).sum()) < 4.0 * m["R"])
                    elif acc[i, j]:
                        twice[i] += 1
                    continue
                if acc[i, j]:
                    out["sums"][i] += quantize36(a[i, j])
                    out["count"][i] += 1
    return out, {"shared": shared, "strangers": strangers, "twice": twice}
