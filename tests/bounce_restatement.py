"""An independent numpy restatement of ONE iteration of the reference's radiance() loop (render.nim:26-38) -- world.hit(ray, 0.001,
+inf, rec), then rec.material.scatter(ray, rec, rng, attenuation, scattered) (materials.nim:21-96) -- for listed rays and
xoshiro256+ states, of the scatter alone for given hit records, of the sky (render.nim:41-44), and of the wavefront loop built
from them (what Context.trace runs).

The hit is hit_restatement.world_hit; the vector helpers are radiance_restatement's; the draws come from the CPU oracle's exported
generator (oracle_rng_uniform01, oracle_rng_uniform_range), its portable sin/cos (oracle_port_sincos) and pow5 (oracle_port_pow5).
Every ray is scattered on its own, in the reference's operation and draw order; numpy's float64 operations are single IEEE roundings
and never fuse.  It shares no code with the library.  test_bounce_query.py anchors it: chained max_depth times it equals
radiance_restatement.radiance, which test_radiance_query.py ties to the oracle's sample sums and the reference's PNG."""
import ctypes as C

import numpy as np

import hit_restatement as H
import radiance_restatement as RR

MISS, SCATTERED, ABSORBED = 0, 1, 2
_DP = C.POINTER(C.c_double)


def _sincos(L, a):
    a, s, c = np.array([a], dtype=np.float64), np.empty(1), np.empty(1)
    L.oracle_port_sincos(a.ctypes.data_as(_DP), s.ctypes.data_as(_DP), c.ctypes.data_as(_DP), 1)
    return s[0], c[0]


def _pow5(L, x):
    x, p = np.array([x], dtype=np.float64), np.empty(1)
    L.oracle_port_pow5(x.ctypes.data_as(_DP), p.ctypes.data_as(_DP), 1)
    return p[0]


def _listed(index, n):
    if index is None:
        return np.arange(n)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    return index[(index >= 0) & (index < n)]        # entries outside [0, n) are skipped


def sky(rays, index=None, out=None):
    """render.nim:41-44 without the attenuation: (1 - t) * white + t * (0.5, 0.7, 1.0), t = 0.5 * unit(direction).y + 1.0 (sic)."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    out = np.zeros((rays.shape[0], 3)) if out is None else out
    ids = _listed(index, rays.shape[0])
    with np.errstate(all="ignore"):
        t = 0.5 * RR._unit(rays[ids, 3:6])[:, 1] + 1.0
        out[ids] = np.stack([1.0 * (1.0 - t) + 0.5 * t, 1.0 * (1.0 - t) + 0.7 * t, 1.0 * (1.0 - t) + 1.0 * t], axis=1)
    return out


def scatter(oracle, recs, rays, raw, states, index=None, out=None):
    """rec.material.scatter for the records `raw` ((n, 8), as hit_restatement.world_hit writes them): the material of `object`, and
    p, normal, front_face as given.  Returns a dict: rays (scattered for a hit), states (after the scatter's last draw), attenuation
    (n, 3), status (n,) int32; rays that are not listed keep what `out` (an earlier result) holds, else 0.  An object outside the
    list counts as a miss (status MISS, attenuation 0, ray and state untouched, nothing drawn)."""
    L = oracle.lib()
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.array(rays, dtype=np.float64).reshape(-1, 7)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    n = rays.shape[0]
    rec = H.fields(np.asarray(raw, dtype=np.float64).reshape(n, 8))
    att = np.zeros((n, 3)) if out is None else out["attenuation"]
    status = np.zeros(n, dtype=np.int32) if out is None else out["status"]
    with np.errstate(all="ignore"):
        for i in _listed(index, n):
            obj = int(rec["object"][i])
            if obj < 0 or obj >= recs.shape[0]:
                att[i], status[i] = 0.0, MISS
                continue
            o = recs[obj]
            g = RR._ptr(st, i)
            p, nrm, front = rec["p"][i:i + 1], rec["normal"][i:i + 1], bool(rec["front_face"][i])
            d = rays[i:i + 1, 3:6].copy()
            mat = int(o[10])
            if mat == RR.MAT_LAMBERTIAN:                                  # materials.nim:24-30: keeps r_in.time
                a = L.oracle_rng_uniform01(g) * RR.TWO_PI                 # sampling.nim:51-55
                z = L.oracle_rng_uniform_range(g, -1.0, 1.0)
                r = np.sqrt(1.0 - z * z)
                s, c = _sincos(L, a)
                new = nrm + np.array([[r * c, r * s, z]])
                att[i], status[i] = o[11:14], SCATTERED
            elif mat == RR.MAT_METAL:                                     # materials.nim:39-47
                while True:                                               # sampling.nim:45-49
                    x = L.oracle_rng_uniform_range(g, -1.0, 1.0)
                    y = L.oracle_rng_uniform_range(g, -1.0, 1.0)
                    w = L.oracle_rng_uniform_range(g, -1.0, 1.0)
                    if x * x + y * y + w * w < 1.0:
                        break
                new = RR._reflect(RR._unit(d), nrm) + np.array([[x, y, w]]) * o[14]
                rays[i, 6] = 0.0                                          # rays.nim:19
                if RR._dot(new, nrm)[0] > 0:
                    att[i], status[i] = o[11:14], SCATTERED
                else:
                    att[i], status[i] = 0.0, ABSORBED                     # (`scattered` is written all the same: materials.nim:41)
            else:                                                         # materials.nim:62-86
                ri = o[15]
                eta = np.array([1.0 / ri if front else ri])
                ud = RR._unit(d)
                dd = RR._dot(-ud, nrm)[0]
                cos_t = dd if dd <= 1.0 else 1.0
                sin_t = np.sqrt(1.0 - cos_t * cos_t)
                if eta[0] * sin_t > 1.0:
                    new = RR._reflect(ud, nrm)                            # total internal reflection: no draw
                else:
                    r0 = (1.0 - eta[0]) / (1.0 + eta[0])                  # materials.nim:55-60
                    r0 = r0 * r0
                    prob = r0 + (1.0 - r0) * _pow5(L, 1.0 - cos_t)
                    new = RR._reflect(ud, nrm) if L.oracle_rng_uniform01(g) < prob else RR._refract(ud, nrm, eta)
                rays[i, 6] = 0.0
                att[i], status[i] = 1.0, SCATTERED
            rays[i, 0:3] = p[0]
            rays[i, 3:6] = new[0]
    return {"rays": rays, "states": st, "attenuation": att, "status": status}


def step(oracle, recs, rays, states, index=None, out=None):
    """One iteration of render.nim:26-38 for the listed rays: scatter()'s dict plus raw ((n, 8) hit records: world.hit(r, 0.001,
    +inf, rec) for the listed rays; others keep what `out` holds, else a miss record)."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    if out is None:
        raw = np.zeros((n, 8))
        raw.view(np.int32)[:, 14] = -1
    else:
        raw = out["raw"]
    ids = _listed(index, n)
    if ids.size:
        raw[ids] = H.world_hit(recs, rays[ids])
    res = scatter(oracle, recs, rays, raw, states, ids, out)
    res["raw"] = raw
    return res


def trace(oracle, recs, rays, states, max_depth, sky_fn=None, emission=None, on_bounce=None):
    """The wavefront loop of Context.trace on step(): (color (n, 3), states (n, 4) uint64).  sky_fn(rays, index) -> (len(index), 3);
    emission (n_objects, 3); on_bounce(step, index, result)."""
    rays = np.array(rays, dtype=np.float64).reshape(-1, 7)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    n = rays.shape[0]
    color, att = np.zeros((n, 3)), np.ones((n, 3))
    live = np.arange(n)
    res = None
    with np.errstate(all="ignore"):
        for k in range(max_depth):
            if live.size == 0:
                break
            res = step(oracle, recs, rays, st, live, res)
            rays, st = res["rays"], res["states"]
            status = res["status"][live]
            miss = live[status == MISS]
            if miss.size:
                color[miss] = (sky(rays, miss)[miss] if sky_fn is None else np.asarray(sky_fn(rays, miss), dtype=np.float64)) * att[miss]
            if emission is not None:
                hit = live[status != MISS]
                color[hit] = color[hit] + att[hit] * np.asarray(emission, dtype=np.float64)[H.fields(res["raw"])["object"][hit]]
            if on_bounce is not None:
                on_bounce(k, live, res)
            live = live[status == SCATTERED]
            att[live] = att[live] * res["attenuation"][live]
    return color, st
