"""An independent numpy restatement of the direct-light sampling queries (tor_light_sample_device, tor_light_pdf_device), written
from the text of include/tor_lights.h, not from the kernels: per light one pass of elementwise float64 operations over all points,
the (n, L) matrices of importances and running sums kept, the pick read off them as the header words it ("the first j with
I_j > 0 whose running sum is > x; if rounding leaves none, the last j with I_j > 0").  numpy's elementwise float64 operations are
single IEEE roundings and never fuse, its sqrt and `/` are correctly rounded, and every expression keeps the header's operation
order.  The draws come from the CPU oracle's exported generator (oracle_rng_uniform01), the sin / cos from its portable routine
(oracle_port_sincos), the centres from nearest_restatement.  It reads the flat (n, 16) records of Scene.to_records."""
import ctypes as C

import numpy as np

import nearest_restatement as N
import radiance_restatement as RR

BY_WEIGHT, BY_SOLID_ANGLE = 0, 1
_DP = C.POINTER(C.c_double)


def _listed(index, n):
    if index is None:
        return np.arange(n)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    return index[(index >= 0) & (index < n)]        # entries outside [0, n) are skipped


def _sincos(L, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    s, c = np.empty_like(a), np.empty_like(a)
    if a.size:
        L.oracle_port_sincos(a.ctypes.data_as(_DP), s.ctypes.data_as(_DP), c.ctypes.data_as(_DP), a.size)
    return s, c


def geometry(recs, lights, points):
    """Per (point, light): dict of (n, L) arrays wx, wy, wz, d2, inside, m and the (L,) R2 -- the header's "per light" block."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    px, py, pz, time = (points[:, k].copy() for k in range(4))
    n, nl = points.shape[0], len(lights)
    g = {k: np.empty((n, nl)) for k in ("wx", "wy", "wz", "d2", "m")}
    g["inside"] = np.empty((n, nl), dtype=bool)
    g["R2"] = np.empty(nl)
    with np.errstate(all="ignore"):
        for j, obj in enumerate(lights):
            rec = recs[int(obj)]
            cx, cy, cz = N._centre(rec, time)
            R = abs(rec[9])
            R2 = R * R
            wx, wy, wz = cx - px, cy - py, cz - pz
            d2 = wx * wx + wy * wy + wz * wz
            inside = ~(d2 > R2)
            s2 = R2 / d2
            m = np.where(inside, 2.0, s2 / (1.0 + np.sqrt(1.0 - s2)))
            g["wx"][:, j], g["wy"][:, j], g["wz"][:, j], g["d2"][:, j], g["m"][:, j] = wx, wy, wz, d2, m
            g["inside"][:, j], g["R2"][j] = inside, R2
    return g


def importances(g, weights, strategy):
    """I (n, L), the running sums (n, L) and the total T (n,): added sequentially in table order, from 0.0."""
    w = np.asarray(weights, dtype=np.float64)
    with np.errstate(all="ignore"):
        imp = np.broadcast_to(w, g["m"].shape).copy() if strategy == BY_WEIGHT else w[None, :] * g["m"]
        runs = np.empty_like(imp)
        total = np.zeros(imp.shape[0])
        for j in range(imp.shape[1]):
            total = total + imp[:, j]
            runs[:, j] = total
    return imp, runs, total


def _weights(lights, weights):
    return np.ones(len(lights)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(len(lights))


def cone(L, wx, wy, wz, d2, R2, m, inside, u1, u2):
    """The header's "cone" block for arrays of picked lights: (the three components of dir, t)."""
    with np.errstate(all="ignore"):
        k = u1 * m
        cos_t = 1.0 - k
        sin2 = k * (2.0 - k)
        sin_t = np.sqrt(sin2)
        s, c = _sincos(L, u2 * RR.TWO_PI)
        sd = np.sqrt(d2)
        inv = 1.0 / sd
        zero = d2 == 0
        ax, ay, az = np.where(zero, 0.0, wx * inv), np.where(zero, 0.0, wy * inv), np.where(zero, 1.0, wz * inv)
        sg = np.copysign(1.0, az)
        aa = -1.0 / (sg + az)
        bb = ax * ay * aa
        b1 = (1.0 + sg * ax * ax * aa, sg * bb, (-sg) * ax)
        b2 = (bb, sg + ay * ay * aa, -ay)
        e1, e2 = sin_t * c, sin_t * s
        dirs = [b1[q] * e1 + b2[q] * e2 + a * cos_t for q, a in enumerate((ax, ay, az))]
        h = R2 - d2 * sin2
        h = np.where(h > 0, h, 0.0)
        t = np.where(inside, sd * cos_t + np.sqrt(h), sd * cos_t - np.sqrt(h))
    return dirs, t


def sample(oracle, recs, lights, weights, points, states, index=None, strategy=BY_SOLID_ANGLE, out=None):
    """tor_light_sample_device for the listed points: a dict of rays (n, 7), pdf (n,), light (n,) int32, dist (n,), states (n, 4)
    uint64 and, for the tests, P (n,) the picked share and pick (n,) the picked light's TABLE index; points that are not listed
    keep what `out` (an earlier result) holds, else light = -1 and the rest 0, and their states."""
    L = oracle.lib()
    lights = np.asarray(lights, dtype=np.int64).reshape(-1)
    weights = _weights(lights, weights)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    n = points.shape[0]
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    res = out if out is not None else dict(rays=np.zeros((n, 7)), pdf=np.zeros(n), light=np.full(n, -1, dtype=np.int32), dist=np.zeros(n),
                                           P=np.zeros(n), pick=np.full(n, -1, dtype=np.int64))
    ids = _listed(index, n)
    u = np.empty((ids.size, 3))
    for e, i in enumerate(ids):                                           # exactly three draws, always, in this order
        for k in range(3):
            u[e, k] = L.oracle_rng_uniform01(RR._ptr(st, i))
    res["states"] = st
    if ids.size == 0:
        return res
    pts = points[ids]
    g = geometry(recs, lights, pts)
    imp, runs, T = importances(g, weights, strategy)
    with np.errstate(all="ignore"):
        usable = (T > 0) & np.isfinite(T)
        x = u[:, 0] * T
        pos = imp > 0
        above = pos & (runs > x[:, None])
        first = np.argmax(above, axis=1)                                  # the first j with I_j > 0 whose running sum is > x
        last = imp.shape[1] - 1 - np.argmax(pos[:, ::-1], axis=1)         # the last j with I_j > 0
        pick = np.where(above.any(axis=1), first, last)
        usable &= pos.any(axis=1)
        rows = np.arange(ids.size)
        wx, wy, wz, d2, m, inside = (g[k][rows, pick] for k in ("wx", "wy", "wz", "d2", "m", "inside"))
        R2 = g["R2"][pick]
        P = imp[rows, pick] / T
        dirs, t = cone(L, wx, wy, wz, d2, R2, m, inside, u[:, 1], u[:, 2])
        pdf = P / (RR.TWO_PI * m)
    rays = np.zeros((ids.size, 7))
    rays[:, 0:3], rays[:, 6] = pts[:, 0:3], pts[:, 3]
    for q in range(3):
        with np.errstate(all="ignore"):
            rays[:, 3 + q] = dirs[q] * t
    none = ~usable
    rays[none] = 0.0
    res["rays"][ids] = rays
    res["pdf"][ids] = np.where(none, 0.0, pdf)
    res["light"][ids] = np.where(none, -1, lights[pick]).astype(np.int32)
    res["dist"][ids] = np.where(none, 0.0, t)
    res["P"][ids] = np.where(none, 0.0, P)
    res["pick"][ids] = np.where(none, -1, pick)
    return res


def pdf(recs, lights, weights, points, objects, index=None, strategy=BY_SOLID_ANGLE, out=None):
    """tor_light_pdf_device: (n,) float64; points that are not listed keep what `out` holds, else 0."""
    lights = np.asarray(lights, dtype=np.int64).reshape(-1)
    weights = _weights(lights, weights)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    objects = np.asarray(objects, dtype=np.int64).reshape(-1)
    n = points.shape[0]
    res = np.zeros(n) if out is None else out
    ids = _listed(index, n)
    if ids.size == 0:
        return res
    g = geometry(recs, lights, points[ids])
    imp, _, T = importances(g, weights, strategy)
    is_light = objects[ids][:, None] == lights[None, :]
    found = is_light.any(axis=1)
    j = np.argmax(is_light, axis=1)
    rows = np.arange(ids.size)
    with np.errstate(all="ignore"):
        I = imp[rows, j]
        value = (I / T) / (RR.TWO_PI * g["m"][rows, j])
        ok = found & (T > 0) & np.isfinite(T) & (I > 0)
    res[ids] = np.where(ok, value, 0.0)
    return res


def same_bits(got, want):
    """Elementwise: equal in every bit, or NaN on both sides (a NaN's sign and payload are not defined, tor_lights.h)."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
