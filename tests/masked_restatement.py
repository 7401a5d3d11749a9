"""The masked queries restated on the restatements the unmasked tests use: a masked query is world.hit(r, t_min, t_max, rec)
(hittables_lists.nim:48-55) on the SUB-LIST of the objects a ray may see -- object j for ray i iff groups[j] & mask[i] != 0 -- in
list order, with `object` reported as the index in the full list.

Per distinct mask value the records are filtered, hit_restatement.world_hit (bounce_restatement.scatter for the steps) runs on the
sub-list for the rays that carry the value, and the winner's index is mapped back.  Nothing here knows about layouts, boxes or
group words per slot: it shares no code with the library."""
import numpy as np

import bounce_restatement as B
import hit_restatement as H

ALL = 0xFFFFFFFF


def _words(groups, n_objects):
    if groups is None:
        return np.full(n_objects, ALL, dtype=np.uint32)
    g = np.asarray(groups).astype(np.int64) & ALL
    assert g.shape == (n_objects,)
    return g.astype(np.uint32)


def ray_masks(mask, n):
    """The mask of every ray: an int for all of them, or one 32-bit word per ray (int32 words count by their bits)."""
    if np.ndim(mask) == 0:
        return np.full(n, int(mask) & ALL, dtype=np.uint32)
    m = (np.asarray(mask).astype(np.int64) & ALL).astype(np.uint32).reshape(-1)
    assert m.shape == (n,)
    return m


def world_hit(recs, groups, rays, mask, t_range=None):
    """(n, 8) records of the masked closest hit, as hit_restatement.world_hit writes them."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    g, m = _words(groups, recs.shape[0]), ray_masks(mask, n)
    out = np.zeros((n, 8), dtype=np.float64)
    out.view(np.int32)[:, 14] = -1                                        # (mask 0, or nothing visible: a miss)
    for value in np.unique(m):
        sel = np.nonzero(m == value)[0]
        seen = np.nonzero((g & value) != 0)[0]                            # the sub-list, in list order
        if seen.size == 0:
            continue
        sub = H.world_hit(recs[seen], rays[sel], None if t_range is None else np.asarray(t_range, dtype=np.float64)[sel])
        obj = sub.view(np.int32)[:, 14]
        sub.view(np.int32)[:, 14] = np.where(obj >= 0, seen[np.maximum(obj, 0)], -1).astype(np.int32)
        out[sel] = sub
    return out


def occluded(recs, groups, rays, mask, t_range=None):
    """world.hit's return value on the sub-list: one bool per ray."""
    return H.fields(world_hit(recs, groups, rays, mask, t_range))["object"] >= 0


def step(oracle, recs, groups, rays, states, mask, index=None, out=None):
    """bounce_restatement.step with the masked closest hit: the visible winner scatters with the reference's draws (the material
    is looked up by the full-list index, which is what the sub-list's record holds after the mapping)."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    if out is None:
        raw = np.zeros((n, 8))
        raw.view(np.int32)[:, 14] = -1
    else:
        raw = out["raw"]
    ids = B._listed(index, n)
    if ids.size:
        raw[ids] = world_hit(recs, groups, rays[ids], ray_masks(mask, n)[ids])
    res = B.scatter(oracle, recs, rays, raw, states, ids, out)
    res["raw"] = raw
    return res


def trace(oracle, recs, groups, rays, states, max_depth, mask_of_step):
    """bounce_restatement.trace's loop with step k seeing mask_of_step(k) (an int or one word per ray): (color, states)."""
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
            res = step(oracle, recs, groups, rays, st, mask_of_step(k), live, res)
            rays, st = res["rays"], res["states"]
            status = res["status"][live]
            miss = live[status == B.MISS]
            if miss.size:
                color[miss] = B.sky(rays, miss)[miss] * att[miss]
            live = live[status == B.SCATTERED]
            att[live] = att[live] * res["attenuation"][live]
    return color, st


def meaningful(recs, groups, rays, masks, t_range=None):
    """What every scene's test asserts before it compares: (share of rays whose masked answer differs from the unmasked one,
    share that keep a hit, every mask value shares a wave of 64 consecutive rays with another value)."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    m = ray_masks(masks, n)
    got = world_hit(recs, groups, rays, m, t_range)
    plain = H.world_hit(recs, rays, t_range)
    changed = (got.view(np.uint64) != plain.view(np.uint64)).any(axis=1)
    keeps = H.fields(got)["object"] >= 0
    mixed = set()
    for w0 in range(0, n, 64):
        vals = np.unique(m[w0:w0 + 64])
        if vals.size > 1:
            mixed.update(int(v) for v in vals)
    return float(changed.mean()), float(keeps.mean()), all(int(v) in mixed for v in np.unique(m))
