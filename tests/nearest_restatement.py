"""An independent numpy restatement of the nearest-surface point query (tor_nearest_device): the K objects closest to a point.

Per object, in list order, the signed distance of every point to its surface
    c  = the sphere's centre, or center0 + (time - time0) / (time1 - time0) * (center1 - center0)     (moving_spheres.nim:39-44)
    oc = p - c
    d  = sqrt(oc.x * oc.x + oc.y * oc.y + oc.z * oc.z) - abs(radius)                                  (vec3s.nim:23-27)
kept when d is finite and d < d_max (strict); then one stable sort per point by d over the columns in list order, so equal d goes to
the lower index.  numpy's elementwise float64 operations are single IEEE roundings and never fuse, its sqrt is correctly rounded,
and every expression keeps the definition's operation order, so the distances are the definition's bits.  It shares no code with
the library: it reads the flat (n, 16) records of Scene.to_records {kind, c0 xyz, c1 xyz, t0, t1, radius, material, ...}."""
import numpy as np

ALL = 0xFFFFFFFF


def _centre(rec, time):
    if int(rec[0]) == 0:
        return rec[1], rec[2], rec[3]
    f = (time - rec[7]) / (rec[8] - rec[7])
    return tuple(rec[1 + k] + (rec[4 + k] - rec[1 + k]) * f for k in range(3))


def _limits(n, d_max):
    if d_max is None:
        return np.full(n, np.inf)
    if np.ndim(d_max) == 0:
        return np.full(n, float(d_max))
    return np.asarray(d_max, dtype=np.float64).reshape(n).copy()


def distances(recs, points):
    """(n, m) float64: column j holds the signed distance of every point to object j's surface (NaN and +-inf as they come)."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    px, py, pz, time = (points[:, k].copy() for k in range(4))
    out = np.empty((points.shape[0], recs.shape[0]))
    with np.errstate(all="ignore"):
        for j, rec in enumerate(recs):
            cx, cy, cz = _centre(rec, time)
            ocx, ocy, ocz = px - cx, py - cy, pz - cz
            out[:, j] = np.sqrt(ocx * ocx + ocy * ocy + ocz * ocz) - abs(rec[9])
    return out


def nearest(recs, points, k, d_max=None):
    """The first k neighbours of every point: a dict of distance (n, k) float64, object (n, k) int32, inside (n, k) int32, count
    (n,) int32 = min(total, k), total (n,) and tied (n,) bool: two of the first k + 1 neighbours share one distance.  Unused
    entries: distance = 0, object = -1, inside = 0."""
    d = distances(recs, points)
    n = d.shape[0]
    lim = _limits(n, d_max)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d < lim[:, None])
    keyed = np.where(ok, d, np.inf)
    dist = np.zeros((n, k))
    obj = np.full((n, k), -1, dtype=np.int32)
    inside = np.zeros((n, k), dtype=np.int32)
    total = ok.sum(axis=1).astype(np.int64)
    tied = np.zeros(n, dtype=bool)
    if keyed.shape[1]:
        order = np.argsort(keyed, axis=1, kind="stable")[:, :k + 1]      # stable: equal d keeps the list order
        st = np.take_along_axis(keyed, order, axis=1)
        has = np.isfinite(st)
        tied = ((st[:, 1:] == st[:, :-1]) & has[:, 1:]).any(axis=1)
        kk = min(k, order.shape[1])
        dist[:, :kk] = np.where(has[:, :kk], st[:, :kk], 0.0)
        obj[:, :kk] = np.where(has[:, :kk], order[:, :kk], -1)
        inside[:, :kk] = (has[:, :kk] & (st[:, :kk] < 0)).astype(np.int32)
    return {"distance": dist, "object": obj, "inside": inside, "count": np.minimum(total, k).astype(np.int32), "total": total,
            "tied": tied}


def masked_nearest(recs, groups, points, mask, k, d_max=None):
    """nearest() on the sub-list of the objects a point sees -- object j for point i iff groups[j] & mask[i] != 0 -- per distinct
    mask value, with `object` mapped back to the full list's numbering."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    n = points.shape[0]
    lim = _limits(n, d_max)
    g = np.full(len(recs), ALL, dtype=np.uint32) if groups is None else (np.asarray(groups).astype(np.int64) & ALL).astype(np.uint32)
    m = np.full(n, int(mask) & ALL, dtype=np.uint32) if np.ndim(mask) == 0 else (np.asarray(mask).astype(np.int64) & ALL).astype(np.uint32)
    assert g.shape == (len(recs),) and m.shape == (n,)
    out = nearest(recs[:0], points, k)                                    # every entry unused
    for value in np.unique(m):
        sel = np.nonzero(m == value)[0]
        seen = np.nonzero((g & value) != 0)[0]                            # the sub-list, in list order
        if seen.size == 0:
            continue
        sub = nearest(recs[seen], points[sel], k, lim[sel])
        sub["object"] = np.where(sub["object"] >= 0, seen[np.maximum(sub["object"], 0)], -1).astype(np.int32)
        for name in out:
            out[name][sel] = sub[name]
    return out


def mismatches(got, want):
    """What differs between a library result (fields distance, object, inside, count as arrays) and the restatement's, bit for bit;
    in `distance` a NaN on both sides counts as equal (no neighbour has one: a NaN there is already a mismatch of `object`)."""
    bad = []
    if not np.array_equal(np.asarray(got["count"]), want["count"]):
        bad.append(f"count: {int((np.asarray(got['count']) != want['count']).sum())} points")
    gd = np.ascontiguousarray(got["distance"], dtype=np.float64)
    wd = np.ascontiguousarray(want["distance"], dtype=np.float64)
    same = (gd.view(np.uint64) == wd.view(np.uint64)) | (np.isnan(gd) & np.isnan(wd))
    if not same.all():
        bad.append(f"distance: {int((~same).any(axis=1).sum())} points")
    for name in ("object", "inside"):
        if not np.array_equal(np.asarray(got[name]), want[name]):
            bad.append(f"{name}: {int((np.asarray(got[name]) != want[name]).any(axis=1).sum())} points")
    return bad
