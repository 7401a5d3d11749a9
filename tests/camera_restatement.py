"""An independent numpy restatement of the light-tracing queries (tor_camera_connect_device, tor_light_emit_device), written from
the text of include/tor_camera.h, not from the kernels: elementwise float64 operations over all points or paths, in the header's
order.  numpy's elementwise float64 operations are single IEEE roundings and never fuse, its sqrt and `/` are correctly rounded.
The draws come from the CPU oracle's exported generator (oracle_rng_uniform01, oracle_rng_uniform_range), the sin / cos from its
portable routine (oracle_port_sincos), the centres from nearest_restatement.  The pick is read off np.searchsorted(...,
side="right") on the running sums plus the fallback, not walked.  Cameras are the 24 float64 of Camera.as_array(): origin,
lower_left_corner, horizontal, vertical, u, v, w, lens_radius, shutter_open, shutter_close; scenes the flat (n, 16) records."""
import numpy as np

import light_restatement as LR
import nearest_restatement as N
import radiance_restatement as RR

PI = 3.141592653589793
same_bits = LR.same_bits


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def camera_constants(cam24, nrows, ncols):
    """The header's "per camera and frame": dict of origin, llc, H, V, u, v, w (3-vectors), lens, fd, HH, VV, K."""
    cam = np.asarray(cam24, dtype=np.float64).reshape(24)
    origin, llc, H, V, u, v, w = (cam[3 * k:3 * k + 3].copy() for k in range(7))
    with np.errstate(all="ignore"):
        fd = _dot(origin - llc, w)
        HH, VV = _dot(H, H), _dot(V, V)
        K = fd * fd * float(ncols - 1) * float(nrows - 1) / (np.sqrt(HH) * np.sqrt(VV))
    return dict(origin=origin, llc=llc, H=H, V=V, u=u, v=v, w=w, lens=cam[21], fd=fd, HH=HH, VV=VV, K=K)


def _draws(L, st, ids, k):
    u = np.empty((ids.size, k))
    for e, i in enumerate(ids):
        for q in range(k):
            u[e, q] = L.oracle_rng_uniform01(RR._ptr(st, i))
    return u


def connect_points(L, c, nrows, ncols, pts, u0, u1):
    """The header's lens / geometry / valid / outputs blocks for arrays of points (m, 4) and their two draws: a dict of rays
    (m, 7), pixel (m,) int32, factor (m,), lens (m, 2) and, for the tests, s, t, z."""
    y = [pts[:, 0], pts[:, 1], pts[:, 2]]
    with np.errstate(all="ignore"):
        r = np.sqrt(u0)
        sn, cs = LR._sincos(L, u1 * RR.TWO_PI)
        lr = c["lens"] * r
        rdx, rdy = lr * cs, lr * sn
        x = [c["origin"][k] + c["u"][k] * rdx + c["v"][k] * rdy for k in range(3)]
        e = [y[k] - x[k] for k in range(3)]
        z = -_dot(e, c["w"])
        kk = c["fd"] / z
        q = [(x[k] + e[k] * kk) - c["llc"][k] for k in range(3)]
        s = _dot(q, c["H"]) / c["HH"]
        t = _dot(q, c["V"]) / c["VV"]
        a, b = s * float(ncols - 1), t * float(nrows - 1)
        ln = np.sqrt(_dot(e, e))
        z3 = z * z * z
        f = c["K"] * ln / z3
        valid = (z > 0) & (a >= 0) & (a < float(ncols)) & (b >= 0) & (b < float(nrows)) & (z3 < np.inf) & (f >= 0) & (f < np.inf)
        col = np.floor(np.where(valid, a, 0.0)).astype(np.int64)
        row = np.floor(np.where(valid, b, 0.0)).astype(np.int64)
        rays = np.zeros((pts.shape[0], 7))
        for k in range(3):
            rays[:, k], rays[:, 3 + k] = y[k], x[k] - y[k]
        rays[:, 6] = pts[:, 3]
    rays[~valid] = 0.0
    return dict(rays=rays, pixel=np.where(valid, row * ncols + col, -1).astype(np.int32), factor=np.where(valid, f, 0.0),
                lens=np.stack([rdx, rdy], axis=1), s=s, t=t, z=z)


def connect(oracle, cam24, nrows, ncols, points, states, index=None, out=None):
    """tor_camera_connect_device for the listed points: a dict of rays (n, 7), pixel (n,) int32, factor (n,), lens (n, 2), states
    (n, 4) uint64; points that are not listed keep what `out` (an earlier result) holds, else pixel = -1 and the rest 0, and
    their states."""
    L = oracle.lib()
    points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    n = points.shape[0]
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    res = out if out is not None else dict(rays=np.zeros((n, 7)), pixel=np.full(n, -1, dtype=np.int32), factor=np.zeros(n),
                                           lens=np.zeros((n, 2)))
    ids = LR._listed(index, n)
    u = _draws(L, st, ids, 2)                                              # exactly two draws, always
    res["states"] = st
    if ids.size == 0:
        return res
    got = connect_points(L, camera_constants(cam24, nrows, ncols), nrows, ncols, points[ids], u[:, 0], u[:, 1])
    for k in ("rays", "pixel", "factor", "lens"):
        res[k][ids] = got[k]
    return res


def pick(runs, weights, x):
    """The header's pick for arrays x: the first light whose running sum is > x; if none, the last light of weight > 0."""
    runs, weights = np.asarray(runs, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    j = np.searchsorted(runs, x, side="right")
    last = int(np.nonzero(weights > 0)[0][-1])
    return np.where(j >= runs.size, last, j)


def running_sums(weights):
    """Added sequentially in table order, from 0.0 (tor_scene_lights)."""
    runs, total = np.empty(len(weights)), 0.0
    for j, w in enumerate(weights):
        total = total + float(w)
        runs[j] = total
    return runs


def emit(oracle, recs, lights, weights, states, time_lo=0.0, time_hi=0.0, index=None, out=None):
    """tor_light_emit_device for the listed paths: a dict of rays (n, 7), normal (n, 3), light (n,) int32, pdf (n, 2), states
    (n, 4) uint64 and, for the tests, pick (n,) the TABLE index, cos_t (n,) and u (n, 5); paths that are not listed keep what
    `out` holds, else light = -1 and the rest 0, and their states."""
    L = oracle.lib()
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    lights = np.asarray(lights, dtype=np.int64).reshape(-1)
    weights = LR._weights(lights, weights)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    n = st.shape[0]
    res = out if out is not None else dict(rays=np.zeros((n, 7)), normal=np.zeros((n, 3)), light=np.full(n, -1, dtype=np.int32),
                                           pdf=np.zeros((n, 2)), pick=np.full(n, -1, dtype=np.int64), cos_t=np.zeros(n), u=np.zeros((n, 5)))
    ids = LR._listed(index, n)
    time = np.empty(ids.size)
    u = np.empty((ids.size, 5))
    for e, i in enumerate(ids):                                           # exactly six draws, in this order
        time[e] = L.oracle_rng_uniform_range(RR._ptr(st, i), float(time_lo), float(time_hi))
        for q in range(5):
            u[e, q] = L.oracle_rng_uniform01(RR._ptr(st, i))
    res["states"] = st
    if ids.size == 0:
        return res
    runs = running_sums(weights)
    T = runs[-1]
    with np.errstate(all="ignore"):
        j = pick(runs, weights, u[:, 0] * T)
        P = weights[j] / T
        c = np.empty((ids.size, 3))
        for e in range(ids.size):
            c[e] = N._centre(recs[int(lights[j[e]])], time[e])
        R = np.abs(recs[lights[j], 9])
        R2 = R * R
        u1, u3 = u[:, 1], u[:, 3]
        zc = 1.0 - 2.0 * u1
        rr = np.sqrt(4.0 * u1 * (1.0 - u1))
        sn, cs = LR._sincos(L, u[:, 2] * RR.TWO_PI)
        nrm = [rr * cs, rr * sn, zc]
        sin_t, cos_t = np.sqrt(u3), np.sqrt(1.0 - u3)
        s4, c4 = LR._sincos(L, u[:, 4] * RR.TWO_PI)
        sg = np.copysign(1.0, nrm[2])
        aa = -1.0 / (sg + nrm[2])
        bb = nrm[0] * nrm[1] * aa
        b1 = (1.0 + sg * nrm[0] * nrm[0] * aa, sg * bb, (-sg) * nrm[0])
        b2 = (bb, sg + nrm[1] * nrm[1] * aa, -nrm[1])
        e1, e2 = sin_t * c4, sin_t * s4
        rays = np.empty((ids.size, 7))
        for k in range(3):
            rays[:, k] = c[:, k] + nrm[k] * R
            rays[:, 3 + k] = b1[k] * e1 + b2[k] * e2 + nrm[k] * cos_t
        rays[:, 6] = time
        pdf = np.stack([P / ((4.0 * PI) * R2), cos_t / PI], axis=1)
    res["rays"][ids], res["normal"][ids], res["pdf"][ids] = rays, np.stack(nrm, axis=1), pdf
    res["light"][ids], res["pick"][ids], res["cos_t"][ids], res["u"][ids] = lights[j].astype(np.int32), j, cos_t, u
    return res
