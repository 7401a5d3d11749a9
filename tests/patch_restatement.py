"""An independent numpy restatement of the planar patch queries, written from the text of include/tor_patches.h and not from the
kernel: Moeller-Trumbore per (ray, patch) with the header's operation order, the winner rule, the record, the merge into sphere
records, the any-hit bit and the wavefront loop of Context.trace_patches.

The table is walked in order, one patch at a time over all rays at once.  numpy's elementwise float64 operations are single IEEE
roundings and never fuse, so every value is the header's bits.  The spheres are hit_restatement.world_hit's and the scatter is
bounce_restatement.scatter's, by import.  VARIANTS are single wrong readings of the header; tests/test_patch_query.py shows that
each changes an output bit of a named case of tests/patch_inputs.py."""
import numpy as np

import bounce_restatement as B
import hit_restatement as H

QUAD, TRIANGLE = 0, 1
PATCH_MAX = 16384

VARIANTS = ["edges_exclusive", "tie_high_index", "range_inclusive", "merge_tie_to_patch", "one_sided", "triangle_as_quad",
            "triangle_sum_before_flip", "normal_not_flipped", "groups_ignored", "record_t_ignored", "default_range_zero"]


def quad(q, u, v, material=-1, groups=0xFFFFFFFF):
    return {"kind": QUAD, "material": int(material), "groups": int(groups) & 0xFFFFFFFF,
            "q": np.asarray(q, dtype=np.float64), "u": np.asarray(u, dtype=np.float64), "v": np.asarray(v, dtype=np.float64)}


def triangle(a, b, c, material=-1, groups=0xFFFFFFFF):
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    return dict(quad(a, b - a, c - a, material, groups), kind=TRIANGLE)


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def refusal(table, n_objects):
    """What tor_scene_patches says of the table (rule 5 of the header): None, or (index, reason)."""
    with np.errstate(all="ignore"):
        for j, p in enumerate(table):
            if p["kind"] not in (QUAD, TRIANGLE):
                return j, "kind"
            if not -1 <= p["material"] < n_objects:
                return j, "material"
            if not all(np.isfinite(p[k]).all() for k in ("q", "u", "v")):
                return j, "finite"
            n = np.array(cross(p["u"], p["v"]))
            if not np.isfinite(n).all():
                return j, "normal"
            nn = dot(n, n)
            if not nn > 0 or np.isinf(nn):
                return j, "area"
            if not np.isfinite(1.0 / np.sqrt(nn)):
                return j, "inverse"
    return None


def pair(p, o, d, variant=None):
    """THE TEST's values for patch p and the rays (o, d: three arrays each), before the range: (inside, t, an, bn, det)."""
    u, v, q = p["u"], p["v"], p["q"]
    pv = cross(d, v)
    det = dot(u, pv)
    usable = np.abs(det) > 0
    tv = (o[0] - q[0], o[1] - q[1], o[2] - q[2])
    an = dot(tv, pv)
    qv = cross(tv, u)
    bn = dot(d, qv)
    tn = dot(v, qv)
    neg = det < 0
    if variant == "one_sided":
        usable = usable & ~neg
    raw_sum_ok = (an + bn) <= det                                         # (triangle_sum_before_flip reads these)
    det, an, bn, tn = (np.where(neg, -x, x) for x in (det, an, bn, tn))
    if variant == "edges_exclusive":
        in_quad = (an > 0) & (an < det) & (bn > 0) & (bn < det)
        in_tri = (an > 0) & (bn > 0) & ((an + bn) < det)
    else:
        in_quad = (an >= 0) & (an <= det) & (bn >= 0) & (bn <= det)
        in_tri = (an >= 0) & (bn >= 0) & (raw_sum_ok if variant == "triangle_sum_before_flip" else ((an + bn) <= det))
    inside = in_tri if (p["kind"] == TRIANGLE and variant != "triangle_as_quad") else in_quad
    return usable & inside, tn / det, an, bn, det


def _operands(rays, t_range, mask, variant):
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    o, d = tuple(rays[:, k].copy() for k in range(3)), tuple(rays[:, 3 + k].copy() for k in range(3))
    if t_range is None:
        t_min, t_max = np.full(n, 0.0 if variant == "default_range_zero" else 0.001), np.full(n, np.inf)
    else:
        t_range = np.asarray(t_range, dtype=np.float64).reshape(n, 2)
        t_min, t_max = t_range[:, 0].copy(), t_range[:, 1].copy()
    if mask is None:
        mask = 0xFFFFFFFF
    words = np.broadcast_to(np.asarray(mask, dtype=np.int64) & 0xFFFFFFFF, (n,)).astype(np.int64)
    return n, o, d, t_min, t_max, words


def _listed(index, n):
    if index is None:
        return np.ones(n, dtype=bool)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    sel = np.zeros(n, dtype=bool)
    sel[index[(index >= 0) & (index < n)]] = True
    return sel


def _in_range(t, t_min, limit, variant, limit_is_record=None):
    if variant == "range_inclusive":
        return (t_min <= t) & (t <= limit)
    upper = t < limit
    if variant == "merge_tie_to_patch" and limit_is_record is not None:
        upper = np.where(limit_is_record, t <= limit, upper)
    return (t_min < t) & upper


def hit(table, rays, t_range=None, mask=None, merge=None, index=None, out=None, variant=None):
    """tor_patch_hit_device: {"raw": (n, 8) records, "patch": (n,) int32, "uv": (n, 2)}.  merge: None, or the (n, 8) sphere records
    the answer starts from.  index: the listed rays; the others keep what `out` (an earlier answer) holds, else raw = merge or a
    miss record, patch -1, uv 0."""
    n, o, d, t_min, t_max, words = _operands(rays, t_range, mask, variant)
    listed = _listed(index, n)
    if out is not None:
        raw, patch, uv = out["raw"], out["patch"], out["uv"]
    else:
        raw = np.zeros((n, 8)) if merge is None else np.array(merge, dtype=np.float64).reshape(n, 8)
        if merge is None:
            raw.view(np.int32)[:, 14] = -1
        patch, uv = np.full(n, -1, dtype=np.int32), np.zeros((n, 2))
    with np.errstate(all="ignore"):
        limit, from_record = t_max.copy(), np.zeros(n, dtype=bool)
        if merge is not None and variant != "record_t_ignored":
            f = H.fields(raw)
            from_record = (f["object"] >= 0) & (f["t"] < t_max)
            limit = np.where(from_record, f["t"], t_max)
        best_t, best_j = np.zeros(n), np.full(n, -1, dtype=np.int64)
        best_an, best_bn, best_det = np.zeros(n), np.zeros(n), np.ones(n)
        for j, p in enumerate(table):
            sees = np.ones(n, dtype=bool) if variant == "groups_ignored" else (p["groups"] & words) != 0
            inside, t, an, bn, det = pair(p, o, d, variant)
            ok = sees & inside & _in_range(t, t_min, limit, variant, from_record)
            better = ok & ((best_j < 0) | ((t <= best_t) if variant == "tie_high_index" else (t < best_t)))
            best_t, best_j = np.where(better, t, best_t), np.where(better, j, best_j)
            best_an, best_bn, best_det = np.where(better, an, best_an), np.where(better, bn, best_bn), np.where(better, det, best_det)
        w = raw.view(np.int32)
        none = listed & (best_j < 0)
        if merge is None:
            raw[none] = 0.0
            w[none, 14] = -1
        patch[none], uv[none] = -1, 0.0
        for j in np.unique(best_j[listed & (best_j >= 0)]):
            sel = listed & (best_j == j)
            p, t = table[j], best_t[sel]
            nrm = cross(p["u"], p["v"])
            inv = 1.0 / np.sqrt(dot(nrm, nrm))
            N = [np.float64(nrm[k] * inv) for k in range(3)]
            front = dot([d[k][sel] for k in range(3)], N) < 0
            for k in range(3):
                raw[sel, k] = o[k][sel] + d[k][sel] * t
                raw[sel, 3 + k] = N[k] if variant == "normal_not_flipped" else np.where(front, N[k], -N[k])
            raw[sel, 6] = t
            w[sel, 14], w[sel, 15] = p["material"], front.astype(np.int32)
            patch[sel] = j
            uv[sel, 0], uv[sel, 1] = best_an[sel] / best_det[sel], best_bn[sel] / best_det[sel]
    return {"raw": raw, "patch": patch, "uv": uv}


def occluded(table, rays, t_range=None, mask=None, merge=None, index=None, out=None, variant=None):
    """tor_patch_occluded_device: (n,) int32.  merge: None, or the (n,) bits the answer is OR-ed into."""
    n, o, d, t_min, t_max, words = _operands(rays, t_range, mask, variant)
    listed = _listed(index, n)
    if out is None:
        out = np.zeros(n, dtype=np.int32) if merge is None else np.array(merge, dtype=np.int32).reshape(n)
    any_hit = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for p in table:
            sees = np.ones(n, dtype=bool) if variant == "groups_ignored" else (p["groups"] & words) != 0
            inside, t, _, _, _ = pair(p, o, d, variant)
            any_hit |= sees & inside & _in_range(t, t_min, t_max, variant)
    if merge is None:
        out[listed] = any_hit[listed]
    else:
        out[listed & any_hit] = 1
    return out


def merge(recs, table, rays, t_range=None, mask=None, variant=None):
    """The closest of spheres and patches, spheres first: world_hit's records with hit(merge=) on top."""
    return hit(table, rays, t_range, mask, merge=H.world_hit(recs, rays, t_range), variant=variant)


def closest_of_both(recs, table, rays, t_range=None):
    """The same said differently: both answers computed alone, the patch taken where it exists and is strictly nearer than the
    sphere (or there is no sphere)."""
    s, p = H.world_hit(recs, rays, t_range), hit(table, rays, t_range)
    fs, fp = H.fields(s), H.fields(p["raw"])
    take = (p["patch"] >= 0) & ((fs["object"] < 0) | (fp["t"] < fs["t"]))
    raw = np.where(take[:, None], p["raw"].view(np.uint64), s.view(np.uint64)).view(np.float64)
    return {"raw": raw, "patch": np.where(take, p["patch"], -1).astype(np.int32), "uv": np.where(take[:, None], p["uv"], 0.0)}


def trace(oracle, recs, table, rays, states, max_depth, sky_fn=None, emission=None, patch_emission=None):
    """The wavefront loop of Context.trace_patches: (color (n, 3), states (n, 4) uint64)."""
    rays = np.array(rays, dtype=np.float64).reshape(-1, 7)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    n = rays.shape[0]
    color, att = np.zeros((n, 3)), np.ones((n, 3))
    live = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(max_depth):
            if live.size == 0:
                break
            r = rays[live]
            rec = merge(recs, table, r)
            obj, patch = H.fields(rec["raw"])["object"], rec["patch"]
            miss = (obj < 0) & (patch < 0)
            if miss.any():
                sky = B.sky(r)[miss] if sky_fn is None else np.asarray(sky_fn(rays, live[miss]), dtype=np.float64)
                color[live[miss]] = sky * att[live[miss]]
            if emission is not None:
                h = obj >= 0
                color[live[h]] = color[live[h]] + att[live[h]] * np.asarray(emission, dtype=np.float64)[obj[h]]
            if patch_emission is not None:
                h = patch >= 0
                color[live[h]] = color[live[h]] + att[live[h]] * np.asarray(patch_emission, dtype=np.float64)[patch[h]]
            res = B.scatter(oracle, recs, r, rec["raw"], st[live])
            rays[live], st[live] = res["rays"], res["states"]
            on = res["status"] == B.SCATTERED
            att[live[on]] = att[live[on]] * res["attenuation"][on]
            live = live[on]
    return color, st


def mismatches(got, want):
    """The outputs whose bits differ (NaN against NaN counts as equal): records field by field, patch, uv; or, for two int32 bit
    arrays, "occluded"."""
    if not isinstance(got, dict):
        bad = int((np.asarray(got, dtype=np.int32) != np.asarray(want, dtype=np.int32)).sum())
        return [f"occluded: {bad} rays"] if bad else []
    bad = list(H.mismatches(got["raw"], want["raw"]))
    if not np.array_equal(np.asarray(got["patch"], dtype=np.int32), np.asarray(want["patch"], dtype=np.int32)):
        bad.append(f"patch: {int((np.asarray(got['patch']) != np.asarray(want['patch'])).sum())} rays")
    g, w = np.asarray(got["uv"], dtype=np.float64), np.asarray(want["uv"], dtype=np.float64)
    same = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
    if not same.all():
        bad.append(f"uv: {int((~same.all(axis=1)).sum())} rays")
    return bad
