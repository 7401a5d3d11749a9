"""An independent numpy restatement of the reference's closest-hit query, HittableList.hit (hittables_lists.nim:48-55) over
Sphere.hit (spheres.nim:28-49) and MovingSphere.hit (moving_spheres.nim:39-67), and the generators the closest-hit tests share.

The restatement walks the list in order with the reference's `closest_so_far`, one object at a time over all rays at once.  numpy's
elementwise float64 operations are single IEEE roundings and never fuse, and every expression keeps the reference's operation order,
so its records are the reference's bits.  It does not share code with the library: it reads the flat (n, 16) records of
Scene.to_records / the oracle {kind, c0 xyz, c1 xyz, t0, t1, radius, material, albedo rgb, fuzz, ri}."""
import ctypes as C

import numpy as np


def _centre(rec, time):
    """moving_spheres.nim:39-44: center0 + (time - time0) / (time1 - time0) * (center1 - center0); a sphere's centre."""
    c0 = [np.full_like(time, rec[1 + k]) for k in range(3)]
    if int(rec[0]) == 0:
        return c0
    f = (time - rec[7]) / (rec[8] - rec[7])
    return [c0[k] + (rec[4 + k] - rec[1 + k]) * f for k in range(3)]


def world_hit(recs, rays, t_range=None):
    """For every ray {origin xyz, direction xyz, time} the record of world.hit(r, t_min, t_max, rec): a dict of t, p (n, 3),
    normal (n, 3), object (int32, -1 = miss) and front_face (int32).  t_range: None = (0.001, +inf), else (n, 2) {t_min, t_max}.
    A miss has every field 0 but object = -1 (the library's convention: the reference leaves rec untouched)."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    ox, oy, oz, dx, dy, dz, time = (rays[:, k].copy() for k in range(7))
    if t_range is None:
        t_min, t_max = np.full(n, 0.001), np.full(n, np.inf)
    else:
        t_range = np.asarray(t_range, dtype=np.float64).reshape(n, 2)
        t_min, t_max = t_range[:, 0].copy(), t_range[:, 1].copy()
    obj = np.full(n, -1, dtype=np.int32)
    closest = t_max.copy()
    with np.errstate(all="ignore"):
        a = dx * dx + dy * dy + dz * dz                                   # spheres.nim:30
        for i, rec in enumerate(recs):                                    # hittables_lists.nim:51-55
            cx, cy, cz = _centre(rec, time)
            ocx, ocy, ocz = ox - cx, oy - cy, oz - cz                     # :29
            half_b = ocx * dx + ocy * dy + ocz * dz                       # :31
            c = (ocx * ocx + ocy * ocy + ocz * ocz) - rec[9] * rec[9]      # :32
            disc = half_b * half_b - a * c                                # :33
            pos = disc > 0
            root = np.sqrt(np.where(pos, disc, 0.0))
            s1 = (-half_b - root) / a                                     # :47
            ok1 = pos & (t_min < s1) & (s1 < closest)
            s2 = (-half_b + root) / a                                     # :48
            ok2 = pos & ~ok1 & (t_min < s2) & (s2 < closest)
            hit = ok1 | ok2
            closest = np.where(ok1, s1, np.where(ok2, s2, closest))
            obj = np.where(hit, np.int32(i), obj)
        out = np.zeros((n, 8), dtype=np.float64)
        words = out.view(np.int32)
        words[:, 14] = -1
        for i in np.unique(obj[obj >= 0]):
            sel = obj == i
            t = closest[sel]
            cx, cy, cz = _centre(recs[i], time[sel])
            px, py, pz = ox[sel] + dx[sel] * t, oy[sel] + dy[sel] * t, oz[sel] + dz[sel] * t   # rays.nim:24-25
            inv = 1.0 / recs[i, 9]                                        # vec3s.nim:93-94
            nx, ny, nz = (px - cx) * inv, (py - cy) * inv, (pz - cz) * inv
            front = (dx[sel] * nx + dy[sel] * ny + dz[sel] * nz) < 0      # core.nim:47-49
            out[sel, 0], out[sel, 1], out[sel, 2] = px, py, pz
            out[sel, 3] = np.where(front, nx, -nx)
            out[sel, 4] = np.where(front, ny, -ny)
            out[sel, 5] = np.where(front, nz, -nz)
            out[sel, 6] = t
            words[sel, 14] = i
            words[sel, 15] = front.astype(np.int32)
    return out


def fields(raw):
    """The fields of an (n, 8) record array (world_hit's, or HitResult.raw)."""
    raw = np.asarray(raw, dtype=np.float64)
    w = raw.view(np.int32)
    return {"p": raw[:, 0:3], "normal": raw[:, 3:6], "t": raw[:, 6], "object": w[:, 14], "front_face": w[:, 15]}


def mismatches(got, want):
    """Field names whose bits differ (NaN against NaN counts as equal: a NaN's sign and payload are not part of IEEE results)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    same[:, 7] = got.view(np.uint64)[:, 7] == want.view(np.uint64)[:, 7]
    bad = []
    for name, cols in (("p", [0, 1, 2]), ("normal", [3, 4, 5]), ("t", [6]), ("object/front_face", [7])):
        if not same[:, cols].all():
            bad.append(f"{name}: {int((~same[:, cols].all(axis=1)).sum())} rays")
    return bad


def camera_rays(oracle, cam24, nrows, ncols, sample=0):
    """The camera ray of sample `sample` of every pixel on the oracle's per-sample streams (TOR_SEED_SAMPLE): pixel_sample's draw
    order (oracle/tor_oracle.c pixel_sample, camera_ray; render.nim:62-66, cameras.nim:47-57) through the oracle's exported RNG.
    Returns (nrows * ncols, 7), row-major, row 0 = bottom."""
    L = oracle.lib()
    cam = np.asarray(cam24, dtype=np.float64)
    origin, llc, horiz, vert, u, v = (cam[3 * k:3 * k + 3] for k in range(6))
    lens, t_open, t_close = cam[21], cam[22], cam[23]
    st = (C.c_uint64 * 4)()
    out = np.empty((nrows * ncols, 7), dtype=np.float64)
    for row in range(nrows):
        for col in range(ncols):
            L.oracle_rng_seed3(row, col, sample, st)
            s = (float(col) + L.oracle_rng_uniform01(st)) / float(ncols - 1)
            t = (float(row) + L.oracle_rng_uniform01(st)) / float(nrows - 1)
            while True:                                                   # random_in_unit_disk
                x = L.oracle_rng_uniform_range(st, -1.0, 1.0)
                y = L.oracle_rng_uniform_range(st, -1.0, 1.0)
                if x * x + y * y + 0.0 * 0.0 < 1.0:
                    break
            rx, ry = x * lens, y * lens
            off = [u[k] * rx + v[k] * ry for k in range(3)]
            o = [origin[k] + off[k] for k in range(3)]
            d = [(((llc[k] + horiz[k] * s) + vert[k] * t) - origin[k]) - off[k] for k in range(3)]
            out[row * ncols + col] = (*o, *d, L.oracle_rng_uniform_range(st, t_open, t_close))
    return out


def incoherent_rays(recs, n, seed, time_range=(0.0, 1.0)):
    """n rays with seeded origins in the scene's box (centres +- radius) and uniform directions."""
    rng = np.random.default_rng(seed)
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    r = np.abs(recs[:, 9:10])
    lo = np.minimum(recs[:, 1:4], recs[:, 4:7]) - r
    hi = np.maximum(recs[:, 1:4], recs[:, 4:7]) + r
    # (the ground sphere of random_scene is 1000 units across: its top is what matters)
    lo, hi = np.percentile(lo, 2, axis=0), np.percentile(hi, 98, axis=0)
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = rng.uniform(time_range[0], time_range[1], n)
    return np.concatenate([o, d, t[:, None]], axis=1)


def far_grazing_rays(recs, seed, distances=(1e4, 1e5, 3e5, 1e6), offsets=(0.0, 2e-7, 1e-6, 2e-6, 4e-6, 8e-6, 3e-5)):
    """Horizontal rays from far away that pass just over the top of every small static sphere (y = top + offset): at a distance D the
    reference's discriminant rounds with an absolute error ~ eps D^2, so it accepts some of them although they pass outside the
    sphere -- farther out than a culling box's margin once D is large."""
    rng = np.random.default_rng(seed)
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    out = []
    for rec in recs:
        if int(rec[0]) != 0 or abs(rec[9]) > 0.5:
            continue
        for dist in distances:
            for off in offsets:
                a = rng.uniform(0, 2 * np.pi)
                u = np.array([np.cos(a), 0.0, np.sin(a)])
                p = rec[1:4] + np.array([0.0, abs(rec[9]) + off, 0.0])
                out.append([*(p - dist * u), *u, 0.0])
    return np.asarray(out, dtype=np.float64)


def group_scene(seed, n=700):
    """A scene of several time groups with movers in general position and along y, spheres at common heights, a ground sphere and a
    few negative radii (after tools/fuzz_accel.py's generator)."""
    rng = np.random.default_rng(seed)
    groups = [(0.0, 1.0), (-0.5, 0.5), (0.25, 2.0), (1.0, 0.0)]
    levels = rng.uniform(0, 3, 3)
    recs = [[0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0]]
    while len(recs) < n:
        c = np.array([rng.uniform(-12, 12), rng.uniform(0, 4), rng.uniform(-12, 12)])
        if rng.random() < 0.5:
            c[1] = levels[int(rng.integers(0, 3))]
        r = float(rng.choice([0.15, 0.2, 0.3, 0.45])) * (1 if rng.random() > 0.03 else -1)
        mat, alb = int(rng.integers(0, 3)), rng.uniform(0.1, 0.9, 3)
        if rng.random() < 0.4:
            recs.append([0, *c, *c, 0, 1, r, mat, *alb, 0.2, 1.5])
        else:
            t0, t1 = groups[int(rng.integers(0, len(groups)))]
            d = rng.uniform(-0.6, 0.6, 3) if rng.random() < 0.5 else np.array([0.0, rng.uniform(0, 0.6), 0.0])
            recs.append([1, *c, *(c + d), t0, t1, r, mat, *alb, 0.2, 1.5])
    return np.asarray(recs, dtype=np.float64)
