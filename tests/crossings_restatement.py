"""An independent numpy restatement of the ordered multi-hit query (tor_crossings_device): every surface a ray crosses, in order.

Per object both roots of the reference's sphere test (spheres.nim:29-48, moving_spheres.nim:39-66) for all rays at once, each kept
when t_min < t < t_max (both strict); then one stable sort per ray by t over columns laid out as object * 2 + which, so equal t goes
to the lower object and then to which 0 before 1.  numpy's elementwise float64 operations are single IEEE roundings and never fuse,
and every expression keeps the reference's operation order, so the roots are the reference's bits.  It shares no code with the
library (and none with hit_restatement.py but the record layout): it reads the flat (n, 16) records of Scene.to_records / the oracle
{kind, c0 xyz, c1 xyz, t0, t1, radius, material, albedo rgb, fuzz, ri}."""
import numpy as np

ALL = 0xFFFFFFFF


def _centre(rec, time):
    """moving_spheres.nim:39-44: center0 + (time - time0) / (time1 - time0) * (center1 - center0); a sphere's centre."""
    if int(rec[0]) == 0:
        return rec[1], rec[2], rec[3]
    f = (time - rec[7]) / (rec[8] - rec[7])
    return tuple(rec[1 + k] + (rec[4 + k] - rec[1 + k]) * f for k in range(3))


def _ranges(n, t_range):
    if t_range is None:
        return np.full(n, 0.001), np.full(n, np.inf)
    t_range = np.asarray(t_range, dtype=np.float64).reshape(n, 2)
    return t_range[:, 0].copy(), t_range[:, 1].copy()


def all_roots(recs, rays, t_range=None):
    """(n, 2 m) float64: column 2 j + w holds root w of object j where it is a crossing, +inf where it is not."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n, m = rays.shape[0], recs.shape[0]
    ox, oy, oz, dx, dy, dz, time = (rays[:, k].copy() for k in range(7))
    t_min, t_max = _ranges(n, t_range)
    out = np.full((n, 2 * m), np.inf)
    with np.errstate(all="ignore"):
        a = dx * dx + dy * dy + dz * dz                                   # spheres.nim:30
        for j, rec in enumerate(recs):
            cx, cy, cz = _centre(rec, time)
            ocx, ocy, ocz = ox - cx, oy - cy, oz - cz                     # :29
            half_b = ocx * dx + ocy * dy + ocz * dz                       # :31
            c = (ocx * ocx + ocy * ocy + ocz * ocz) - rec[9] * rec[9]      # :32
            disc = half_b * half_b - a * c                                # :33
            pos = disc > 0
            root = np.sqrt(np.where(pos, disc, 0.0))
            for w, s in ((0, (-half_b - root) / a), (1, (-half_b + root) / a)):   # :47, :48
                ok = pos & (t_min < s) & (s < t_max)
                out[:, 2 * j + w] = np.where(ok, s, np.inf)
    return out


def crossings(recs, rays, k, t_range=None):
    """The first k crossings of every ray: a dict of t (n, k) float64, object (n, k) int32, which (n, k) int32, count (n,) int32 =
    min(total, k), total (n,) and tied (n,) bool: two of the first k + 1 crossings share one t.  Unused entries: t = 0, object =
    -1, which = 0."""
    roots = all_roots(recs, rays, t_range)
    n = roots.shape[0]
    t = np.zeros((n, k))
    obj = np.full((n, k), -1, dtype=np.int32)
    which = np.zeros((n, k), dtype=np.int32)
    total = np.isfinite(roots).sum(axis=1).astype(np.int64)
    tied = np.zeros(n, dtype=bool)
    if roots.shape[1]:
        order = np.argsort(roots, axis=1, kind="stable")[:, :k + 1]       # stable: equal t keeps the column order (object, which)
        st = np.take_along_axis(roots, order, axis=1)
        has = np.isfinite(st)
        tied = ((st[:, 1:] == st[:, :-1]) & has[:, 1:]).any(axis=1)
        kk = min(k, order.shape[1])
        t[:, :kk] = np.where(has[:, :kk], st[:, :kk], 0.0)
        obj[:, :kk] = np.where(has[:, :kk], order[:, :kk] // 2, -1)
        which[:, :kk] = np.where(has[:, :kk], order[:, :kk] % 2, 0)
    return {"t": t, "object": obj, "which": which, "count": np.minimum(total, k).astype(np.int32), "total": total, "tied": tied}


def tied_rays(recs, rays, k, t_range=None, chunk=8192):
    """crossings(recs, rays, k, t_range)["tied"] -- two of the first k + 1 crossings share one t -- for many rays: the same roots
    (all_roots), chunk by chunk so that the (chunk, 2 m) array stays small, and the k + 1 smallest of each ray by a partition in
    place of the full sort (equal t values are equal wherever a partition puts them)."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    t_range = None if t_range is None else np.asarray(t_range, dtype=np.float64).reshape(-1, 2)
    n = rays.shape[0]
    out = np.zeros(n, dtype=bool)
    for lo in range(0, n, chunk):
        roots = all_roots(recs, rays[lo:lo + chunk], None if t_range is None else t_range[lo:lo + chunk])
        if roots.shape[1] < 2:
            continue
        kk = min(k + 1, roots.shape[1])
        st = np.sort(np.partition(roots, kk - 1, axis=1)[:, :kk], axis=1)
        out[lo:lo + chunk] = ((st[:, 1:] == st[:, :-1]) & np.isfinite(st[:, 1:])).any(axis=1)
    return out


def masked_crossings(recs, groups, rays, mask, k, t_range=None):
    """crossings() on the sub-list of the objects a ray sees -- object j for ray i iff groups[j] & mask[i] != 0 -- per distinct
    mask value, with `object` mapped back to the full list's numbering."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    g = np.full(len(recs), ALL, dtype=np.uint32) if groups is None else (np.asarray(groups).astype(np.int64) & ALL).astype(np.uint32)
    m = np.full(n, int(mask) & ALL, dtype=np.uint32) if np.ndim(mask) == 0 else (np.asarray(mask).astype(np.int64) & ALL).astype(np.uint32)
    assert g.shape == (len(recs),) and m.shape == (n,)
    out = crossings(recs[:0], rays, k)                                    # every entry unused
    for value in np.unique(m):
        sel = np.nonzero(m == value)[0]
        seen = np.nonzero((g & value) != 0)[0]                            # the sub-list, in list order
        if seen.size == 0:
            continue
        sub = crossings(recs[seen], rays[sel], k, None if t_range is None else np.asarray(t_range, dtype=np.float64)[sel])
        sub["object"] = np.where(sub["object"] >= 0, seen[np.maximum(sub["object"], 0)], -1).astype(np.int32)
        for name in out:
            out[name][sel] = sub[name]
    return out


def records(recs, rays, cr):
    """(n, k, 8) raw TorHit records of the crossings `cr`: p = origin + direction * t (rays.nim:24-25), normal = outward = (p -
    centre(time)) * (1.0 / radius) (vec3s.nim:93-94), negated when front_face = 0, front_face = dot(direction, outward) < 0
    (core.nim:47-49); t; object and front_face as the two int32 halves of word 7.  Unused entries: the miss record."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n, k = cr["t"].shape
    out = np.zeros((n, k, 8))
    words = out.view(np.int32)
    words[:, :, 14] = -1
    with np.errstate(all="ignore"):
        for e in range(k):
            obj, t = cr["object"][:, e], cr["t"][:, e]
            for j in np.unique(obj[obj >= 0]):
                sel = np.nonzero(obj == j)[0]
                o, d, ts = rays[sel, 0:3], rays[sel, 3:6], t[sel]
                cx, cy, cz = _centre(recs[j], rays[sel, 6])
                p = [o[:, a] + d[:, a] * ts for a in range(3)]
                inv = 1.0 / recs[j, 9]
                nrm = [(p[0] - cx) * inv, (p[1] - cy) * inv, (p[2] - cz) * inv]
                front = (d[:, 0] * nrm[0] + d[:, 1] * nrm[1] + d[:, 2] * nrm[2]) < 0
                for a in range(3):
                    out[sel, e, a] = p[a]
                    out[sel, e, 3 + a] = np.where(front, nrm[a], -nrm[a])
                out[sel, e, 6] = ts
                words[sel, e, 14] = j
                words[sel, e, 15] = front.astype(np.int32)
    return out


def mismatches(got, want, hits=None, want_hits=None):
    """What differs between a library result (fields t, object, which, count as arrays) and the restatement's, bit for bit.  In the
    records' float words a NaN on both sides counts as equal, as in hit_restatement.mismatches: IEEE 754 leaves a NaN result's sign
    and payload open, so those bits are not the reference's to fix; a NaN against a number, and every other bit, differs.  t, object,
    which, count and the records' word 7 are compared by their bits without exception."""
    bad = []
    if not np.array_equal(np.asarray(got["count"]), want["count"]):
        bad.append(f"count: {int((np.asarray(got['count']) != want['count']).sum())} rays")
    gt, wt = np.ascontiguousarray(got["t"], dtype=np.float64), np.ascontiguousarray(want["t"], dtype=np.float64)
    if not np.array_equal(gt.view(np.uint64), wt.view(np.uint64)):
        bad.append(f"t: {int((gt.view(np.uint64) != wt.view(np.uint64)).any(axis=1).sum())} rays")
    for name in ("object", "which"):
        if not np.array_equal(np.asarray(got[name]), want[name]):
            bad.append(f"{name}: {int((np.asarray(got[name]) != want[name]).any(axis=1).sum())} rays")
    if want_hits is not None:
        g, w = np.ascontiguousarray(hits, dtype=np.float64).view(np.uint64), want_hits.view(np.uint64)
        same = (g == w) | (np.isnan(np.asarray(hits)) & np.isnan(want_hits))
        same[:, :, 7] = g[:, :, 7] == w[:, :, 7]
        if not same.all():
            bad.append(f"records: {int((~same.all(axis=(1, 2))).sum())} rays")
    return bad
