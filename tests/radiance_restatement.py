"""An independent numpy restatement of the reference's radiance(ray, world, max_depth, rng) (render.nim:21-47) for arbitrary rays and
xoshiro256+ states, and of the camera's rays (render.nim:63-65 + cameras.nim:47-57) with the state they leave.

Every bounce is hit_restatement.world_hit (world.hit(r, 0.001, +inf, rec)); the scatter follows the CPU oracle's `scatter`
(oracle/tor_oracle.c, materials.nim:24-96) in its draw order, with the oracle's exported generator (oracle_rng_uniform01,
oracle_rng_uniform_range), its portable sin/cos (oracle_port_sincos) and pow5 (oracle_port_pow5).  numpy's float64 operations are
single IEEE roundings and never fuse; every expression keeps the reference's operation order.  It shares no code with the library.
Records are the flat (n, 16) {kind, c0 xyz, c1 xyz, t0, t1, radius, material, albedo rgb, fuzz, ri} of Scene.to_records / the oracle."""
import ctypes as C

import numpy as np

import hit_restatement as H

TWO_PI = 2.0 * 3.141592653589793  # sampling.nim:52: Nim's 2 * PI
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2


def _ptr(states, i):
    return states[i].ctypes.data_as(C.POINTER(C.c_uint64))


def quantize36(x):
    """Round to the nearest multiple of 2^-36 (ties to even), as oracle_quantize36: (x + 1.5 * 2^16) - 1.5 * 2^16."""
    return (np.asarray(x, dtype=np.float64) + 98304.0) - 98304.0


def _unit(d):
    """vec3s.nim:106-107 unit_vector: d / length, `/ s` as `* (1.0 / s)` (vec3s.nim:93-94)."""
    inv = 1.0 / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return d * inv[:, None]


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _reflect(u, n):
    """rays.nim:27-28: u - n * (2 * dot(u, n))."""
    return u - n * (2.0 * _dot(u, n))[:, None]


def _refract(uv, n, eta):
    """rays.nim:30-37."""
    cos_theta = _dot(-uv, n)
    par = (uv + n * cos_theta[:, None]) * eta[:, None]
    perp = n * (-np.sqrt(1.0 - _dot(par, par)))[:, None]
    return par + perp


def radiance(oracle, recs, rays, states, max_depth):
    """(color (n, 3), states (n, 4) uint64 after the path's last draw) of radiance(rays[i], world, max_depth, states[i])."""
    L = oracle.lib()
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.array(rays, dtype=np.float64).reshape(-1, 7)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    n = rays.shape[0]
    color = np.zeros((n, 3), dtype=np.float64)
    att = np.ones((n, 3), dtype=np.float64)
    active = np.arange(n) if max_depth > 0 else np.arange(0)
    depth = 0
    with np.errstate(all="ignore"):
        while active.size and depth < max_depth:                          # render.nim:25
            rec = H.fields(H.world_hit(recs, rays[active]))               # render.nim:28
            obj = rec["object"]
            miss = obj < 0
            # render.nim:41-45: the sky (sic: 0.5 * y + 1.0)
            mi = active[miss]
            t = 0.5 * _unit(rays[mi, 3:6])[:, 1] + 1.0
            sky = np.stack([1.0 * (1.0 - t) + 0.5 * t, 1.0 * (1.0 - t) + 0.7 * t, 1.0 * (1.0 - t) + 1.0 * t], axis=1)
            color[mi] = sky * att[mi]
            keep = np.zeros(active.size, dtype=bool)
            hit = np.nonzero(~miss)[0]
            o = recs[obj[hit]]
            mat = o[:, 10].astype(int)
            p, nrm, front = rec["p"][hit], rec["normal"][hit], rec["front_face"][hit] != 0
            ids = active[hit]
            new_dir = np.zeros((hit.size, 3))
            new_time = rays[ids, 6].copy()
            # Lambertian (materials.nim:24-30): normal + random_unit_vector (sampling.nim:51-55); keeps r_in.time
            lam = np.nonzero(mat == MAT_LAMBERTIAN)[0]
            a, z = np.empty(lam.size), np.empty(lam.size)
            for j, k in enumerate(lam):
                a[j] = L.oracle_rng_uniform01(_ptr(st, ids[k])) * TWO_PI
                z[j] = L.oracle_rng_uniform_range(_ptr(st, ids[k]), -1.0, 1.0)
            s, c = np.empty(lam.size), np.empty(lam.size)
            if lam.size:
                a = np.ascontiguousarray(a)
                L.oracle_port_sincos(a.ctypes.data_as(C.POINTER(C.c_double)), s.ctypes.data_as(C.POINTER(C.c_double)),
                                     c.ctypes.data_as(C.POINTER(C.c_double)), lam.size)
            r = np.sqrt(1.0 - z * z)
            new_dir[lam] = nrm[lam] + np.stack([r * c, r * s, z], axis=1)
            att[ids[lam]] = att[ids[lam]] * o[lam, 11:14]
            keep[hit[lam]] = True
            # Metal (materials.nim:39-47): reflect(unit(d), n) + fuzz * random_in_unit_sphere; time 0; absorbed unless dot > 0
            met = np.nonzero(mat == MAT_METAL)[0]
            ris = np.empty((met.size, 3))
            for j, k in enumerate(met):
                while True:                                               # sampling.nim:45-49
                    x = L.oracle_rng_uniform_range(_ptr(st, ids[k]), -1.0, 1.0)
                    y = L.oracle_rng_uniform_range(_ptr(st, ids[k]), -1.0, 1.0)
                    w = L.oracle_rng_uniform_range(_ptr(st, ids[k]), -1.0, 1.0)
                    if x * x + y * y + w * w < 1.0:
                        break
                ris[j] = (x, y, w)
            md = _reflect(_unit(rays[ids[met], 3:6]), nrm[met]) + ris * o[met, 14:15]
            new_dir[met] = md
            new_time[met] = 0.0
            ok = _dot(md, nrm[met]) > 0
            att[ids[met[ok]]] = att[ids[met[ok]]] * o[met[ok], 11:14]
            keep[hit[met[ok]]] = True                                     # (the others: black, render.nim:38)
            # Dielectric (materials.nim:62-86)
            die = np.nonzero(mat == MAT_DIELECTRIC)[0]
            ri = o[die, 15]
            eta = np.where(front[die], 1.0 / ri, ri)
            ud = _unit(rays[ids[die], 3:6])
            nd = nrm[die]
            dd = _dot(-ud, nd)
            cos_t = np.where(dd <= 1.0, dd, 1.0)
            sin_t = np.sqrt(1.0 - cos_t * cos_t)
            tir = eta * sin_t > 1.0
            r0 = (1.0 - eta) / (1.0 + eta)                                # materials.nim:55-60
            r0 = r0 * r0
            x5 = np.ascontiguousarray(1.0 - cos_t)
            p5 = np.empty(die.size)
            if die.size:
                L.oracle_port_pow5(x5.ctypes.data_as(C.POINTER(C.c_double)), p5.ctypes.data_as(C.POINTER(C.c_double)), die.size)
            prob = r0 + (1.0 - r0) * p5
            refl = tir.copy()
            for j, k in enumerate(die):
                if not tir[j]:
                    refl[j] = L.oracle_rng_uniform01(_ptr(st, ids[k])) < prob[j]
            new_dir[die] = np.where(refl[:, None], _reflect(ud, nd), _refract(ud, nd, eta))
            new_time[die] = 0.0
            keep[hit[die]] = True
            rays[ids, 0:3] = p
            rays[ids, 3:6] = new_dir
            rays[ids, 6] = new_time
            active = active[keep]
            depth += 1
    return color, st                                                      # (still active: depth exhausted, black)


def camera_rays(oracle, cam24, nrows, ncols, pixels=None, first_sample=0, n_samples=1, states=None):
    """The camera rays of render.nim:63-65 + cameras.nim:47-57 (the oracle's pixel_sample draw order) and the states after the
    camera's draws: (rays (m, 7), states (m, 4) uint64).  pixels: flat indices row * ncols + col (None: every pixel, row-major).
    states None: TOR_SEED_SAMPLE, seed3(row, col, s) for s in [first_sample, first_sample + n_samples), entry e and sample s at
    e * n_samples + (s - first_sample); else (one sample) the per-pixel states to draw from, as TOR_SEED_PIXEL chains them."""
    L = oracle.lib()
    cam = np.asarray(cam24, dtype=np.float64)
    origin, llc, horiz, vert, u, v = (cam[3 * k:3 * k + 3] for k in range(6))
    lens, t_open, t_close = cam[21], cam[22], cam[23]
    pix = np.arange(nrows * ncols) if pixels is None else np.asarray(pixels, dtype=np.int64).reshape(-1)
    if states is not None:
        assert n_samples == 1
        st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    else:
        st = np.zeros((pix.size * n_samples, 4), dtype=np.uint64)
    out = np.empty((pix.size * n_samples, 7), dtype=np.float64)
    for e, flat in enumerate(pix):
        row, col = int(flat) // ncols, int(flat) % ncols
        for k in range(n_samples):
            i = e * n_samples + k
            g = _ptr(st, i)
            if states is None:
                L.oracle_rng_seed3(row, col, first_sample + k, g)
            s = (float(col) + L.oracle_rng_uniform01(g)) / float(ncols - 1)
            t = (float(row) + L.oracle_rng_uniform01(g)) / float(nrows - 1)
            while True:                                                   # random_in_unit_disk
                x = L.oracle_rng_uniform_range(g, -1.0, 1.0)
                y = L.oracle_rng_uniform_range(g, -1.0, 1.0)
                if x * x + y * y + 0.0 * 0.0 < 1.0:
                    break
            rx, ry = x * lens, y * lens
            off = [u[j] * rx + v[j] * ry for j in range(3)]
            o = [origin[j] + off[j] for j in range(3)]
            d = [(((llc[j] + horiz[j] * s) + vert[j] * t) - origin[j]) - off[j] for j in range(3)]
            out[i] = (*o, *d, L.oracle_rng_uniform_range(g, t_open, t_close))
    return out, st


def sums_and_moments(color, n_pix, n_samples):
    """Per pixel the sum of q = quantize36(color) and of quantize36(q * q) over its n_samples consecutive entries: what
    oracle.accumulate returns (exact in any order)."""
    q = quantize36(np.asarray(color, dtype=np.float64).reshape(n_pix, n_samples, 3))
    return q.sum(axis=1), quantize36(q * q).sum(axis=1)


def three_material_scene():
    """A small scene with all three materials on both sides of glass, a fuzzy and a sharp metal, a mover and a ground sphere."""
    return np.asarray([
        [0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0],
        [0, 0, 1, 0, 0, 1, 0, 0, 1, 1.0, 2, 0, 0, 0, 0, 1.5],
        [0, 0, 1, 0, 0, 1, 0, 0, 1, -0.9, 2, 0, 0, 0, 0, 1.5],
        [0, -4, 1, 0, -4, 1, 0, 0, 1, 1.0, 0, .4, .2, .1, 0, 0],
        [0, 4, 1, 0, 4, 1, 0, 0, 1, 1.0, 1, .7, .6, .5, 0.0, 0],
        [0, 2, 0.3, 2, 2, 0.3, 2, 0, 1, 0.3, 1, .8, .8, .8, 0.4, 0],
        [1, -2, 0.25, 2, -2, 0.6, 2, 0, 1, 0.25, 0, .2, .8, .3, 0, 0],
        [0, 1, 0.2, 3, 1, 0.2, 3, 0, 1, 0.2, 2, 0, 0, 0, 0, 2.4],
    ], dtype=np.float64)
