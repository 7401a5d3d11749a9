"""An independent restatement of the participating-media queries (include/tor_media.h): the optical-depth march, the isotropic
scatter, the uniforms, and the wavefront loop built from them (what Context.trace_media runs).

The roots of every (ray, medium) pair are computed once in numpy float64 -- elementwise operations are single IEEE roundings and
never fuse, every expression keeps the header's order -- and the march then runs ray by ray in scalar float64, line by line as the
header writes it, over ALL media of the table (no touch word, no union: what the kernel skips must not matter).  The draws come
from the CPU oracle's exported generator (oracle_rng_uniform01, oracle_rng_uniform_range) and its portable sin / cos
(oracle_port_sincos), as bounce_restatement.py takes them.  It shares no code with the library, only the record layout: the
flat (n, 16) records {kind, c0 xyz, c1 xyz, t0, t1, radius, material, albedo rgb, fuzz, ri} of Scene.to_records / the oracle."""
import ctypes as C

import numpy as np

import bounce_restatement as BR
import hit_restatement as H
import radiance_restatement as RR

REFUSED, ESCAPED, COLLIDED = -1, 0, 1
MEDIA_MAX = 64
_F = np.float64


def _listed(index, n):
    if index is None:
        return np.arange(n)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    return index[(index >= 0) & (index < n)]        # entries outside [0, n) are skipped


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def roots(recs, objects, rays):
    """(has (n, M) bool, s0 (n, M), s1 (n, M)): per ray and medium m (object objects[m]) the two unclipped roots of the reference's
    sphere test (spheres.nim:29-48, moving_spheres.nim:39-66), disc > 0 strict; 0 where has is false."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n, M = rays.shape[0], len(objects)
    ox, oy, oz, dx, dy, dz, time = (rays[:, k].copy() for k in range(7))
    has, s0, s1 = np.zeros((n, M), dtype=bool), np.zeros((n, M)), np.zeros((n, M))
    with np.errstate(all="ignore"):
        a = dx * dx + dy * dy + dz * dz
        for m, j in enumerate(objects):
            rec = recs[int(j)]
            cx, cy, cz = rec[1], rec[2], rec[3]
            if int(rec[0]) != 0:
                f = (time - rec[7]) / (rec[8] - rec[7])
                cx, cy, cz = cx + (rec[4] - rec[1]) * f, cy + (rec[5] - rec[2]) * f, cz + (rec[6] - rec[3]) * f
            ocx, ocy, ocz = ox - cx, oy - cy, oz - cz
            half_b = ocx * dx + ocy * dy + ocz * dz
            cc = (ocx * ocx + ocy * ocy + ocz * ocz) - rec[9] * rec[9]
            disc = half_b * half_b - a * cc
            pos = disc > 0
            root = np.sqrt(np.where(pos, disc, 0.0))
            has[:, m] = pos
            s0[:, m] = np.where(pos, (-half_b - root) / a, 0.0)
            s1[:, m] = np.where(pos, (-half_b + root) / a, 0.0)
    return has, s0, s1


def march(recs, objects, sigma, rays, tau, t_range=None, index=None, into=None, steps=None, variant=None):
    """tor_media_march_device for the listed rays: a dict of status (n,) int32, t, depth, rho (n,) float64, active (n,) uint64; rays
    that are not listed keep what `into` (an earlier result) holds, else 0.  steps: an (n,) int array that receives the number of
    iterations each listed ray ran.  variant: None, or the name of a deliberately wrong march (the mutants of
    profiles/media_mutants.txt, restated, so that the CPU suite can show which inputs tell them apart)."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n, M = rays.shape[0], len(objects)
    assert M <= MEDIA_MAX
    sigma = [float(s) for s in np.asarray(sigma, dtype=np.float64).reshape(-1)]
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,))
    if t_range is None:
        t_lo, t_hi = np.zeros(n), np.full(n, np.inf)
    else:
        t_range = np.asarray(t_range, dtype=np.float64).reshape(n, 2)
        t_lo, t_hi = t_range[:, 0], t_range[:, 1]
    if into is None:
        out = {"status": np.zeros(n, dtype=np.int32), "t": np.zeros(n), "depth": np.zeros(n), "rho": np.zeros(n),
               "active": np.zeros(n, dtype=np.uint64)}
    else:
        out = {k: np.array(v) for k, v in into.items()}
    has, s0, s1 = roots(recs, objects, rays)
    d = rays[:, 3:6]
    with np.errstate(all="ignore"):
        length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        for i in _listed(index, n):
            t_min, t_max, budget, ln = _F(t_lo[i]), _F(t_hi[i]), _F(tau[i]), _F(length[i])
            if not (budget >= 0) or not (t_min < t_max):
                out["status"][i], out["t"][i], out["depth"][i], out["rho"][i], out["active"][i] = REFUSED, t_min, 0.0, 0.0, 0
                continue
            hs, a0, a1 = has[i].tolist(), [_F(v) for v in s0[i]], [_F(v) for v in s1[i]]
            t, D = t_min, _F(0.0)
            answer = None
            count = 0
            for _ in range(2 * M + 1):
                count += 1
                rho, A = _F(0.0), 0
                order = range(M - 1, -1, -1) if variant == "rho_descending" else range(M)
                for m in order:
                    inside = (a0[m] < t if variant == "s0_strict" else a0[m] <= t) and t < a1[m]
                    if hs[m] and inside:
                        rho = rho + _F(sigma[m])
                        A |= (1 << (m % 32)) if variant == "shift32" else (1 << m)
                t_next = t_max
                for m in range(M):
                    if not hs[m]:
                        continue
                    if a0[m] > t and a0[m] < t_next:
                        t_next = a0[m]
                    if variant != "skip_s1" and a1[m] > t and a1[m] < t_next:
                        t_next = a1[m]
                if variant == "no_rho_guard":
                    step = rho * ((t_next - t) * ln)
                else:
                    step = rho * ((t_next - t) * ln) if rho > 0 else _F(0.0)
                rem = budget - D
                if rho > 0 and (rem <= step if variant == "rem_le" else rem < step):
                    t_c = t + (rem / rho) / ln
                    if variant != "no_clamp" and t_next < t_c:
                        t_c = t_next
                    answer = (COLLIDED, t_c, budget, rho, A)
                    break
                D = D + step
                if not (t_next < t_max):
                    break
                t = t_next
            if answer is None:
                answer = (ESCAPED, t_max, D, _F(0.0), 0)
            out["status"][i], out["t"][i], out["depth"][i], out["rho"][i] = answer[:4]
            out["active"][i] = np.uint64(answer[4])
            if steps is not None:
                steps[i] = count
    return out


VARIANTS = ("s0_strict", "rem_le", "rho_descending", "shift32", "no_rho_guard", "skip_s1", "no_clamp")


def _sincos(L, a):
    dp = C.POINTER(C.c_double)
    a, s, c = np.array([a], dtype=np.float64), np.empty(1), np.empty(1)
    L.oracle_port_sincos(a.ctypes.data_as(dp), s.ctypes.data_as(dp), c.ctypes.data_as(dp), 1)
    return s[0], c[0]


def scatter(oracle, sigma, albedo, rays, t, active, states, index=None, into=None):
    """tor_media_scatter_device for the listed rays: a dict of rays (n, 7), attenuation (n, 3) and states (n, 4) uint64; rays that
    are not listed keep what `into` holds (else 0) and their state."""
    L = oracle.lib()
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    M = sigma.size
    albedo = np.ones((M, 3)) if albedo is None else np.asarray(albedo, dtype=np.float64).reshape(M, 3)
    t = np.asarray(t, dtype=np.float64).reshape(n)
    active = np.asarray(active).reshape(n).view(np.uint64) if np.asarray(active).dtype.itemsize == 8 else np.asarray(active, dtype=np.uint64)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    new = np.zeros((n, 7)) if into is None else np.array(into["rays"])
    att = np.zeros((n, 3)) if into is None else np.array(into["attenuation"])
    with np.errstate(all="ignore"):
        for i in _listed(index, n):
            g = RR._ptr(st, i)
            a = L.oracle_rng_uniform01(g) * RR.TWO_PI                     # sampling.nim:51-55: exactly two outputs, always
            z = L.oracle_rng_uniform_range(g, -1.0, 1.0)
            r = np.sqrt(_F(1.0) - _F(z) * _F(z))
            s, c = _sincos(L, a)
            A = int(active[i])
            rho, num = _F(0.0), [_F(0.0)] * 3
            for m in range(M):
                if (A >> m) & 1:
                    rho = rho + sigma[m]
                    num = [num[k] + sigma[m] * albedo[m, k] for k in range(3)]
            if A == 0 or (A >> M) != 0 or not (rho > 0):
                new[i], att[i] = 0.0, 0.0
                continue
            new[i, 0:3] = rays[i, 0:3] + t[i] * rays[i, 3:6]
            new[i, 3:6] = [r * c, r * s, z]
            new[i, 6] = rays[i, 6]
            att[i] = [num[k] / rho for k in range(3)]
    return {"rays": new, "attenuation": att, "states": st}


def uniforms(oracle, states, n_draws, index=None, into=None):
    """tor_rng_uniform_device: (u (n, n_draws), states (n, 4) uint64 after the draws)."""
    L = oracle.lib()
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    u = np.zeros((st.shape[0], n_draws)) if into is None else np.array(into)
    for i in _listed(index, st.shape[0]):
        for k in range(n_draws):
            u[i, k] = L.oracle_rng_uniform01(RR._ptr(st, i))
    return u, st


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def march_mismatches(got, want, rows=slice(None)):
    """What differs between two march results, bit for bit (a NaN on both sides counts as equal: its sign and payload are not
    defined); `got` may hold active as int64."""
    bad = []
    for k in ("t", "depth", "rho"):
        same = same_bits(np.asarray(got[k])[rows], want[k][rows])
        if not same.all():
            bad.append(f"{k}: {int((~same).sum())} rays")
    if not np.array_equal(np.asarray(got["status"])[rows], want["status"][rows]):
        bad.append(f"status: {int((np.asarray(got['status'])[rows] != want['status'][rows]).sum())} rays")
    ga = np.ascontiguousarray(got["active"]).view(np.uint64)[rows]
    if not np.array_equal(ga, want["active"][rows]):
        bad.append(f"active: {int((ga != want['active'][rows]).sum())} rays")
    return bad


def trace(oracle, recs, objects, sigma, albedo, rays, states, max_depth, free_flight, sky_fn=None):
    """The wavefront loop of Context.trace_media with the media's boundaries hidden from the surface hits: per iteration and live
    ray the closest hit on the other objects, one uniform01, tau = free_flight(u), the march up to the hit, then the medium's or the
    material's scatter, or the sky.  Returns (color (n, 3), states (n, 4) uint64)."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.array(rays, dtype=np.float64).reshape(-1, 7)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    n = rays.shape[0]
    surf = np.array([j for j in range(len(recs)) if j not in set(int(o) for o in objects)], dtype=np.int64)
    color, att = np.zeros((n, 3)), np.ones((n, 3))
    live = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(max_depth):
            if live.size == 0:
                break
            raw = np.zeros((n, 8))
            raw.view(np.int32)[:, 14] = -1
            if surf.size:
                sub = H.world_hit(recs[surf], rays[live])
                w = sub.view(np.int32)
                w[:, 14] = np.where(w[:, 14] >= 0, surf[np.maximum(w[:, 14], 0)], -1)
                raw[live] = sub
            hit = H.fields(raw)
            u, st = uniforms(oracle, st, 1, live)
            tau = np.asarray(free_flight(u[:, 0]), dtype=np.float64)
            tr = np.zeros((n, 2))
            tr[:, 1] = np.where(hit["object"] >= 0, hit["t"], np.inf)
            m = march(recs, objects, sigma, rays, tau, tr, live)
            status, obj = m["status"][live], hit["object"][live]
            collided = live[status == COLLIDED]
            surface = live[(status == ESCAPED) & (obj >= 0)]
            missed = live[(status == ESCAPED) & (obj < 0)]
            alive = np.zeros(n, dtype=bool)
            if missed.size:
                sk = BR.sky(rays, missed)[missed] if sky_fn is None else np.asarray(sky_fn(rays, missed), dtype=np.float64)
                color[missed] = sk * att[missed]
            if surface.size:
                res = BR.scatter(oracle, recs, rays, raw, st, surface)
                rays, st = res["rays"], res["states"]
                sc = surface[res["status"][surface] == BR.SCATTERED]
                att[sc] = att[sc] * res["attenuation"][sc]
                alive[sc] = True
            if collided.size:
                res = scatter(oracle, sigma, albedo, rays, m["t"], m["active"], st, collided)
                st = res["states"]
                rays[collided] = res["rays"][collided]
                att[collided] = att[collided] * res["attenuation"][collided]
                alive[collided] = True
            live = np.nonzero(alive)[0]
    return color, st
