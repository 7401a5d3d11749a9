"""An independent restatement of the heterogeneous-media queries (include/tor_grid.h): the optical-depth march through the density
grid of one medium by regular tracking, the density lookup, the homogeneous march on a table some of whose media have grids, and
the wavefront loops built from them (what Context.trace_media and Context.trace_media_direct run with grids).

Everything runs ray by ray in scalar numpy float64 -- every operation a single IEEE rounding, never fused --, one operation per
line of the header.  It shares no code with the library, only the record layout of media_restatement.py: the flat (n, 16) records
{kind, c0 xyz, c1 xyz, t0, t1, radius, ...}.  A grid is a dict(medium, n (3 ints), lo (3), hi (3), density (flat, C order)); make_grid
builds one, with the sphere's bounding cube as the default box."""
import numpy as np

import media_restatement as MR

REFUSED, ESCAPED, COLLIDED = -1, 0, 1
GRID_MAX_DIM, GRID_MAX_CELLS = 1024, 1 << 24
_F = np.float64
INF = _F(np.inf)

VARIANTS = ("tie_high_axis", "no_guard", "x_fastest", "no_entry_clamp", "incremental_planes", "rem_le_step", "no_collision_clamp",
            "box_in_world")


def make_grid(recs, objects, medium, density, box=None):
    density = np.asarray(density, dtype=np.float64)
    assert density.ndim == 3
    rec = np.asarray(recs, dtype=np.float64).reshape(-1, 16)[int(objects[medium])]
    if box is None:
        R = np.sqrt(_F(rec[9]) * _F(rec[9]))
        lo, hi = [-R] * 3, [R] * 3
    else:
        lo, hi = [_F(v) for v in box[:3]], [_F(v) for v in box[3:]]
    return dict(medium=int(medium), n=tuple(int(v) for v in density.shape), lo=[_F(v) for v in lo], hi=[_F(v) for v in hi],
                density=np.ascontiguousarray(density).reshape(-1).copy())


def _centre(rec, time):
    c = [_F(rec[1]), _F(rec[2]), _F(rec[3])]
    if int(rec[0]) != 0:
        f = (_F(time) - _F(rec[7])) / (_F(rec[8]) - _F(rec[7]))
        c = [c[k] + (_F(rec[4 + k]) - _F(rec[1 + k])) * f for k in range(3)]
    return c


def _index(q, lo, h, n, clamp=True):
    f = np.floor((q - lo) / h)
    if clamp:
        if not (f >= 0):
            f = _F(0.0)
        if f > n - 1:
            f = _F(n - 1)
        return int(f)
    return int(f) if np.isfinite(f) else 0


def _plane(i, dr, lo, h, oc, d):
    return ((lo + _F(i + (1 if dr > 0 else 0)) * h) - oc) / d


def march_one(rec, sigma_m, grid, ray, tau, t_min, t_max, variant=None, trail=None):
    """One ray: (status, t, depth, active, rho, cell, iterations).  trail: a dict that receives what the walk met (guard: times tn < t
    held; clamped: the entry clamp changed an index)."""
    o = [_F(ray[0]), _F(ray[1]), _F(ray[2])]
    d = [_F(ray[3]), _F(ray[4]), _F(ray[5])]
    tau, t_min, t_max = _F(tau), _F(t_min), _F(t_max)
    m = grid["medium"]
    n, lo, hi, dens = grid["n"], grid["lo"], grid["hi"], grid["density"]
    h = [(hi[k] - lo[k]) / _F(n[k]) for k in range(3)]
    a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    ln = np.sqrt(a)
    c = _centre(rec, ray[6])
    oc = [o[k] - c[k] for k in range(3)]
    half_b = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2]
    cc = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - _F(rec[9]) * _F(rec[9])
    disc = half_b * half_b - a * cc
    if not (tau >= 0) or not (t_min < t_max):
        return REFUSED, t_min, _F(0.0), 0, _F(0.0), -1, 0
    empty = (ESCAPED, t_max, _F(0.0), 0, _F(0.0), -1, 0)
    if not (disc > 0):
        return empty
    root = np.sqrt(disc)
    s0 = (-half_b - root) / a
    s1 = (-half_b + root) / a
    t0, t1 = t_min, t_max
    if s0 > t0:
        t0 = s0
    if s1 < t1:
        t1 = s1
    ob = o if variant == "box_in_world" else oc            # the mutant takes the box in world coordinates
    for k in range(3):
        if d[k] == 0:
            if not (ob[k] >= lo[k] and ob[k] < hi[k]):
                return empty
        else:
            ta = (lo[k] - ob[k]) / d[k]
            tb = (hi[k] - ob[k]) / d[k]
            near, far = (ta, tb) if d[k] > 0 else (tb, ta)
            if near > t0:
                t0 = near
            if far < t1:
                t1 = far
    if not (t0 < t1):
        return empty
    i, dr, tk = [0] * 3, [0] * 3, [INF] * 3
    for k in range(3):
        p = ob[k] + t0 * d[k]
        i[k] = _index(p, lo[k], h[k], n[k], clamp=variant != "no_entry_clamp")
        if trail is not None and _index(p, lo[k], h[k], n[k], clamp=False) != i[k]:
            trail["clamped"] = trail.get("clamped", 0) + 1
        dr[k] = 1 if d[k] > 0 else (-1 if d[k] < 0 else 0)
        tk[k] = INF if dr[k] == 0 else _plane(i[k], dr[k], lo[k], h[k], ob[k], d[k])
    t, D = t0, _F(0.0)
    count = 0
    cells = n[0] * n[1] * n[2]
    for _ in range(n[0] + n[1] + n[2]):
        count += 1
        ks, tn = 0, tk[0]
        if variant == "tie_high_axis":
            if tk[1] <= tn:
                ks, tn = 1, tk[1]
            if tk[2] <= tn:
                ks, tn = 2, tk[2]
        else:
            if tk[1] < tn:
                ks, tn = 1, tk[1]
            if tk[2] < tn:
                ks, tn = 2, tk[2]
        last = not (tn < t1)
        if last:
            tn = t1
        if tn < t:
            if trail is not None:
                trail["guard"] = trail.get("guard", 0) + 1
            if variant != "no_guard":
                tn = t
        cell = (i[2] * n[1] + i[1]) * n[0] + i[0] if variant == "x_fastest" else (i[0] * n[1] + i[1]) * n[2] + i[2]
        rho = _F(sigma_m) * _F(dens[cell] if 0 <= cell < cells else 0.0)   # (out of range only for no_entry_clamp: a fault there)
        step = rho * ((tn - t) * ln) if rho > 0 else _F(0.0)
        rem = tau - D
        if rho > 0 and (rem <= step if variant == "rem_le_step" else rem < step):
            t_c = t + (rem / rho) / ln
            if variant != "no_collision_clamp" and tn < t_c:
                t_c = tn
            return COLLIDED, t_c, tau, 1 << m, rho, cell, count
        D = D + step
        if last:
            break
        i[ks] += dr[ks]
        if i[ks] < 0 or i[ks] >= n[ks]:
            break
        if variant == "incremental_planes":
            tk[ks] = tk[ks] + h[ks] / abs(d[ks])
        else:
            tk[ks] = _plane(i[ks], dr[ks], lo[ks], h[ks], ob[ks], d[ks])
        t = tn
    return ESCAPED, t_max, D, 0, _F(0.0), -1, count


def _ranges(t_range, n):
    if t_range is None:
        return np.zeros(n), np.full(n, np.inf)
    t_range = np.asarray(t_range, dtype=np.float64).reshape(n, 2)
    return t_range[:, 0], t_range[:, 1]


def march(recs, objects, sigma, grid, rays, tau, t_range=None, index=None, into=None, steps=None, variant=None, trails=None):
    """tor_media_grid_march_device for the listed rays: a dict of status, cell (n,) int32, t, depth, rho (n,) float64, active (n,)
    uint64; rays that are not listed keep what `into` holds, else 0 (cell -1).  steps: receives the iterations per listed ray;
    trails: a dict ray -> what march_one's trail recorded."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,))
    t_lo, t_hi = _ranges(t_range, n)
    if into is None:
        out = {"status": np.zeros(n, dtype=np.int32), "t": np.zeros(n), "depth": np.zeros(n), "rho": np.zeros(n),
               "active": np.zeros(n, dtype=np.uint64), "cell": np.full(n, -1, dtype=np.int32)}
    else:
        out = {k: np.array(v) for k, v in into.items()}
    m = grid["medium"]
    rec, sg = recs[int(objects[m])], np.asarray(sigma, dtype=np.float64).reshape(-1)[m]
    with np.errstate(all="ignore"):
        for i in MR._listed(index, n):
            trail = {} if trails is not None else None
            st, t, dep, act, rho, cell, count = march_one(rec, sg, grid, rays[i], tau[i], t_lo[i], t_hi[i], variant, trail)
            out["status"][i], out["t"][i], out["depth"][i], out["rho"][i], out["cell"][i] = st, t, dep, rho, cell
            out["active"][i] = np.uint64(act)
            if steps is not None:
                steps[i] = count
            if trails is not None:
                trails[int(i)] = trail
    return out


def density(recs, objects, grid, points, index=None, into=None):
    """tor_media_grid_density_device: (cell (n,) int32, density (n,) float64)."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    n = points.shape[0]
    cell, value = (np.full(n, -1, dtype=np.int32), np.zeros(n)) if into is None else (np.array(into[0]), np.array(into[1]))
    rec = recs[int(objects[grid["medium"]])]
    nn, lo, hi = grid["n"], grid["lo"], grid["hi"]
    h = [(hi[k] - lo[k]) / _F(nn[k]) for k in range(3)]
    with np.errstate(all="ignore"):
        for i in MR._listed(index, n):
            c = _centre(rec, points[i, 3])
            q = [_F(points[i, k]) - c[k] for k in range(3)]
            inside = (q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) - _F(rec[9]) * _F(rec[9]) < 0
            inside = inside and all(q[k] >= lo[k] and q[k] < hi[k] for k in range(3))
            if not inside:
                cell[i], value[i] = -1, 0.0
                continue
            ix, iy, iz = (_index(q[k], lo[k], h[k], nn[k]) for k in range(3))
            cell[i] = (ix * nn[1] + iy) * nn[2] + iz
            value[i] = grid["density"][cell[i]]
    return cell, value


def march_with_grids(recs, objects, sigma, grid_media, rays, tau, t_range=None, index=None, into=None):
    """tor_media_march_device on a table whose media `grid_media` have grids: media_restatement's march on the table with those
    media REMOVED, the active bits mapped back to the full table's."""
    keep = [m for m in range(len(objects)) if m not in set(int(g) for g in grid_media)]
    sub = MR.march(recs, [objects[m] for m in keep], [np.asarray(sigma, dtype=np.float64).reshape(-1)[m] for m in keep], rays, tau,
                   t_range, index, None)
    full = np.zeros(len(sub["active"]), dtype=np.uint64)
    for b, m in enumerate(keep):
        full |= ((sub["active"] >> np.uint64(b)) & np.uint64(1)) << np.uint64(m)
    sub["active"] = full
    if into is not None:
        rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
        listed = np.zeros(rays.shape[0], dtype=bool)
        listed[MR._listed(index, rays.shape[0])] = True
        sub = {k: np.where(listed, v, np.asarray(into[k])).astype(v.dtype) for k, v in sub.items()}
    return sub


def mismatches(got, want, rows=slice(None)):
    """media_restatement.march_mismatches, and the cell."""
    bad = MR.march_mismatches(got, want, rows)
    if not np.array_equal(np.asarray(got["cell"])[rows], want["cell"][rows]):
        bad.append(f"cell: {int((np.asarray(got['cell'])[rows] != want['cell'][rows]).sum())} rays")
    return bad


def depth_through(recs, objects, sigma, grids, rays, t_range):
    """The optical depth of segments through the table and its grids, as Context.transmittance adds it: the homogeneous depth, then
    each grid medium's, in ascending medium order."""
    grids = sorted(grids, key=lambda g: g["medium"])
    depth = march_with_grids(recs, objects, sigma, [g["medium"] for g in grids], rays, np.inf, t_range)["depth"]
    for g in grids:
        depth = depth + march(recs, objects, sigma, g, rays, np.inf, t_range)["depth"]
    return depth


def trace(oracle, recs, objects, sigma, albedo, g_phase, grids, rays, states, max_depth, free_flight, phase=False, direct=None):
    """The wavefront loop of Context.trace_media (phase False / True) and, with direct = dict(emission, light_states, light_sample,
    occluded, transmit) as phase_restatement.trace takes it, of Context.trace_media_direct, on a table with density grids: per iteration and live ray the closest hit on the
    objects that are not boundaries, 1 + K uniforms in one call, the homogeneous march up to the hit, then each grid march in
    ascending medium order up to the earliest collision so far; the winner scatters.  Returns (color (n, 3), states (n, 4) uint64)."""
    import bounce_restatement as BR
    import hit_restatement as H
    import phase_restatement as PR
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.array(rays, dtype=np.float64).reshape(-1, 7)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    n = rays.shape[0]
    grids = sorted(grids, key=lambda g: g["medium"])
    gm = [g["medium"] for g in grids]
    K = len(grids)
    surf = np.array([j for j in range(len(recs)) if j not in set(int(o) for o in objects)], dtype=np.int64)
    color, att = np.zeros((n, 3)), np.ones((n, 3))
    live = np.arange(n)
    if direct is not None:
        assert phase
        emission = np.asarray(direct["emission"], dtype=np.float64).reshape(-1, 3)
        lst = direct["light_states"]
        after_collision = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for step in range(max_depth):
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
            u, st = MR.uniforms(oracle, st, 1 + K, live)
            tr = np.zeros((n, 2))
            tr[:, 1] = np.where(hit["object"] >= 0, hit["t"], np.inf)
            m = march_with_grids(recs, objects, sigma, gm, rays, np.asarray(free_flight(u[:, 0]), dtype=np.float64), tr, live)
            status, t, active = m["status"].copy(), m["t"].copy(), m["active"].copy()
            for j, g in enumerate(grids):
                gr = np.zeros((n, 2))
                gr[:, 1] = np.where(status == COLLIDED, t, tr[:, 1])
                a = march(recs, objects, sigma, g, rays, np.asarray(free_flight(u[:, 1 + j]), dtype=np.float64), gr, live)
                won = np.zeros(n, dtype=bool)
                won[live] = a["status"][live] == COLLIDED
                status, t, active = np.where(won, COLLIDED, status), np.where(won, a["t"], t), np.where(won, a["active"], active)
            obj = hit["object"][live]
            collided = live[status[live] == COLLIDED]
            surface = live[(status[live] == ESCAPED) & (obj >= 0)]
            missed = live[(status[live] == ESCAPED) & (obj < 0)]
            alive = np.zeros(n, dtype=bool)
            if missed.size:
                sk = BR.sky(rays, missed)[missed] * att[missed]
                color[missed] = sk if direct is None else color[missed] + sk
            if surface.size:
                if direct is not None:
                    found = att[surface] * emission[hit["object"][surface]]
                    color[surface] = color[surface] + np.where(after_collision[surface][:, None], 0.0, found)
                res = BR.scatter(oracle, recs, rays, raw, st, surface)
                rays, st = res["rays"], res["states"]
                sc = surface[res["status"][surface] == BR.SCATTERED]
                att[sc] = att[sc] * res["attenuation"][sc]
                alive[sc] = True
                if direct is not None:
                    after_collision[sc] = False
            if collided.size:
                if phase:
                    res = PR.sample(oracle, sigma, albedo, g_phase, rays, t, active, st, collided)
                else:
                    res = MR.scatter(oracle, sigma, albedo, rays, t, active, st, collided)
                st = res["states"]
                if direct is not None:
                    after_collision[collided] = True
                    if step != max_depth - 1:
                        points = np.zeros((n, 4))
                        points[collided, 0:3], points[collided, 3] = res["rays"][collided, 0:3], res["rays"][collided, 6]
                        ls = direct["light_sample"](points, lst, collided)
                        lst = ls["states"]
                        sr = np.zeros((n, 2))
                        sr[:, 0], sr[:, 1] = 0.001, 1.0
                        blocked = direct["occluded"](ls["rays"], sr, collided)
                        zr = np.zeros((n, 2))
                        zr[:, 1] = 1.0
                        depth = march_with_grids(recs, objects, sigma, gm, ls["rays"], np.inf, zr, collided)["depth"][collided]
                        for g in grids:                      # the depths of a shadow segment add, ascending
                            depth = depth + march(recs, objects, sigma, g, ls["rays"], np.inf, zr, collided)["depth"][collided]
                        T = np.asarray(direct["transmit"](depth), dtype=np.float64)
                        ev = PR.evaluate(sigma, albedo, g_phase, rays, active, ls["rays"], collided)
                        pdf, lamp = ls["pdf"][collided], ls["light"][collided].astype(np.int64)
                        ok = (~blocked[collided]) & (lamp >= 0) & (pdf > 0) & np.isfinite(pdf)
                        add = att[collided] * ev["value"][collided] * emission[np.maximum(lamp, 0)] * (T / pdf)[:, None]
                        color[collided] = color[collided] + np.where(ok[:, None], add, 0.0)
                rays[collided] = res["rays"][collided]
                att[collided] = att[collided] * res["attenuation"][collided]
                alive[collided] = True
            live = np.nonzero(alive)[0]
    return color, st
