"""An independent numpy restatement of the environment-light queries (tor_scene_environment's tables, tor_env_sample_device,
tor_env_eval_device), written from the text of include/tor_env.h, not from the kernels: elementwise float64 operations over all
points in the header's order, the running sums added sequentially, the picks read off np.searchsorted(..., side="right") -- "the
first index whose running sum is > x" -- plus the header's fallbacks, not walked.  numpy's elementwise float64 operations are single
IEEE roundings and never fuse, its sqrt and `/` are correctly rounded.  The draws come from the CPU oracle's exported generator
(oracle_rng_uniform01)."""
import numpy as np

import radiance_restatement as RR


def _listed(index, n):
    if index is None:
        return np.arange(n)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    return index[(index >= 0) & (index < n)]        # entries outside [0, n) are skipped


def decode(s, t):
    """The header's decode for arrays: (dx, dy, dz, len)."""
    with np.errstate(all="ignore"):
        py = (1.0 - np.abs(s)) - np.abs(t)
        up = py >= 0
        px = np.where(up, s, np.copysign(1.0 - np.abs(t), s))
        pz = np.where(up, t, np.copysign(1.0 - np.abs(s), t))
        ln = np.sqrt(px * px + py * py + pz * pz)
        inv = 1.0 / ln
        return px * inv, py * inv, pz * inv, ln


def position(n, row, col, a, b):
    """(s, t) of the position (a, b) inside texel (row, col)."""
    h = 2.0 / float(n)
    return (col.astype(np.float64) + a) * h - 1.0, (row.astype(np.float64) + b) * h - 1.0


def encode(n, dx, dy, dz):
    """The header's encode for arrays: (usable, row, col, len); row = col = -1 and len = 0 where the direction is unusable."""
    with np.errstate(all="ignore"):
        L1 = np.abs(dx) + np.abs(dy) + np.abs(dz)
        usable = (L1 > 0) & np.isfinite(L1)
        L1 = np.where(usable, L1, 1.0)
        qx, qy, qz = dx / L1, dy / L1, dz / L1
        up = dy >= 0
        s = np.where(up, qx, np.copysign(1.0 - np.abs(qz), qx))
        t = np.where(up, qz, np.copysign(1.0 - np.abs(qx), qz))
        half = 0.5 * float(n)
        s, t = np.where(usable, s, 0.0), np.where(usable, t, 0.0)
        col = np.clip(np.floor((s + 1.0) * half).astype(np.int64), 0, n - 1)
        row = np.clip(np.floor((t + 1.0) * half).astype(np.int64), 0, n - 1)
        ln = np.sqrt(qx * qx + qy * qy + qz * qz)
    return usable, np.where(usable, row, -1), np.where(usable, col, -1), np.where(usable, ln, 0.0)


def table(rgb, importance=None):
    """The header's table: dict of n, rgb (n, n, 3), I (n, n), cum (n, n), S (n,), M (n,), T."""
    rgb = np.asarray(rgb, dtype=np.float64)
    n = rgb.shape[0]
    assert rgb.shape == (n, n, 3)
    if importance is None:
        R, G, B = rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2]
        lum = (0.2126 * R + 0.7152 * G) + 0.0722 * B
        idx = np.arange(n)
        s, t = position(n, idx[:, None] * np.ones((1, n), dtype=np.int64), idx[None, :] * np.ones((n, 1), dtype=np.int64), 0.5, 0.5)
        ln = decode(s, t)[3]
        imp = lum * (1.0 / ((ln * ln) * ln))
    else:
        imp = np.asarray(importance, dtype=np.float64).reshape(n, n).copy()
    cum = np.empty((n, n))
    run = np.zeros(n)
    for c in range(n):                                                    # sequential in ascending c
        run = run + imp[:, c]
        cum[:, c] = run
    S = cum[:, n - 1].copy()
    M = np.empty(n)
    tot = 0.0
    for r in range(n):                                                    # sequential in ascending r
        tot = tot + S[r]
        M[r] = tot
    return dict(n=n, rgb=rgb, I=imp, cum=cum, S=S, M=M, T=M[n - 1])


def density(tab, imp, ln):
    n = float(tab["n"])
    with np.errstate(all="ignore"):
        P = imp / tab["T"]
        A = (n * n) * 0.25
        return (P * A) * ((ln * ln) * ln)


def pick(tab, u0, u1):
    """The header's row and column for arrays of the first two draws."""
    n = tab["n"]
    x = u0 * tab["T"]
    row = np.searchsorted(tab["M"], x, side="right")                      # the first r with M_r > x
    last_row = int(np.nonzero(tab["S"] > 0)[0][-1])
    row = np.where(row >= n, last_row, row)
    y = u1 * tab["S"][row]
    col = np.empty_like(row)
    for e in range(row.size):
        r = int(row[e])
        c = int(np.searchsorted(tab["cum"][r], y[e], side="right"))       # the first c with cum[row][c] > y
        col[e] = c if c < n else int(np.nonzero(tab["I"][r] > 0)[0][-1])
    return row, col


def draws(oracle, states, ids, count=4):
    L = oracle.lib()
    u = np.empty((len(ids), count))
    for e, i in enumerate(ids):
        for k in range(count):
            u[e, k] = L.oracle_rng_uniform01(RR._ptr(states, i))
    return u


def sample(oracle, tab, points, states, index=None, out=None):
    """tor_env_sample_device for the listed points: a dict of rays (n, 7), pdf (n,), texel (n,) int32, color (n, 3), states (n, 4)
    uint64 and, for the tests, u (n, 4) the draws and len (n,); points that are not listed keep what `out` (an earlier result)
    holds, else texel = -1 and the rest 0, and their states."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    m, n = points.shape[0], tab["n"]
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    res = out if out is not None else dict(rays=np.zeros((m, 7)), pdf=np.zeros(m), texel=np.full(m, -1, dtype=np.int32),
                                           color=np.zeros((m, 3)), u=np.zeros((m, 4)), len=np.zeros(m))
    ids = _listed(index, m)
    u = draws(oracle, st, ids)                                            # exactly four draws, always, in this order
    res["states"] = st
    if ids.size == 0:
        return res
    row, col = pick(tab, u[:, 0], u[:, 1])
    s, t = position(n, row, col, u[:, 2], u[:, 3])
    dx, dy, dz, ln = decode(s, t)
    rays = np.empty((ids.size, 7))
    rays[:, 0:3], rays[:, 6] = points[ids, 0:3], points[ids, 3]
    rays[:, 3], rays[:, 4], rays[:, 5] = dx, dy, dz
    res["rays"][ids] = rays
    res["pdf"][ids] = density(tab, tab["I"][row, col], ln)
    res["texel"][ids] = (row * n + col).astype(np.int32)
    res["color"][ids] = tab["rgb"][row, col]
    res["u"][ids], res["len"][ids] = u, ln
    return res


def evaluate(tab, rays, index=None, out=None):
    """tor_env_eval_device for the listed rays: a dict of color (n, 3), pdf (n,), texel (n,) int32 and len (n,); rays that are not
    listed keep what `out` holds, else texel = -1 and the rest 0."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    m, n = rays.shape[0], tab["n"]
    res = out if out is not None else dict(color=np.zeros((m, 3)), pdf=np.zeros(m), texel=np.full(m, -1, dtype=np.int32), len=np.zeros(m))
    ids = _listed(index, m)
    if ids.size == 0:
        return res
    usable, row, col, ln = encode(n, rays[ids, 3], rays[ids, 4], rays[ids, 5])
    r, c = np.maximum(row, 0), np.maximum(col, 0)
    res["color"][ids] = np.where(usable[:, None], tab["rgb"][r, c], 0.0)
    res["pdf"][ids] = np.where(usable, density(tab, tab["I"][r, c], ln), 0.0)
    res["texel"][ids] = np.where(usable, r * n + c, -1).astype(np.int32)
    res["len"][ids] = ln
    return res


def same_bits(got, want):
    """Elementwise: equal in every bit, or NaN on both sides."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
