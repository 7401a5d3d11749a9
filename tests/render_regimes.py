"""Scene regimes, cameras and the expected kernel build for the render kernels' sweep (tests/test_render_regimes.py,
tests/test_gpu_render_regimes.py).

The scenes are tests/query_regimes.py's (scene(name, seed) there, unchanged), one derived regime that makes ties visible on the
canvas -- `dense_ties`: `dense` whose 24 trailing duplicates carry another material kind and another albedo than their originals,
so the canvas depends on WHICH of two coincident spheres wins -- and interleaved copies of five of the small regimes (`tiny_x5` ...),
because of query_regimes' scenes only dense2 has more than 96 blocks: without the copies the two-level kernels would meet the oracle on
one scene, and a two-level scene with several time groups on none.

Cameras per regime, from its `spread` and the 2..98 % box of its placeable records: `outside` and `inside` (thin lens, a shutter
that reaches outside every time group), `closeup` on the densest spot of the dense regimes (a quarter of its pixel-centre rays cross 64
or more spheres: what overflows the candidate queues and the pooled lists) `tele`, the outside direction from 1.0e6 (inside the
float32 filter's guard of 2^20), 1.1e6 (past it) and 1e9 units away, and `behind`, 1e9 units away with the world origin between the
camera and the scene.

expected_variant() restates, from tor_api.cpp's launch configuration and tor_scene.cpp's build_accel, which
integrate_kernel<SEEDING, ARITH, W, F32, BLOCKS> a lane launch must run for a scene; it never judges a pixel.  numpy only."""
import numpy as np

import query_regimes as Q

# name: (base regime, copies) -- copy k is shifted by k * TILE_STEP * spread: the copies interleave, the scene keeps its size
TILED = {"tiny_x5": ("tiny", 5), "far_x5": ("far", 5), "dense_x2": ("dense", 2), "huge_far_x3": ("huge_far", 3), "groups_x2": ("groups", 2),
         "noground_x12": ("noground", 12)}
TILE_STEP = np.array([0.27, 0.03, 0.08])               # (chosen so that no `inside` camera sits inside a sphere)
ISSUE_REGIMES = ("tiny", "far", "huge_far", "dense", "dense2", "groups", "noground", "odd_objects", "dense_ties")
REGIMES = ISSUE_REGIMES + tuple(TILED)
N_DUPLICATES = 24

H, W, SPP, DEPTH = 20, 34, 6, 12                       # 64 waves of samples: rays in different states share every wave
ASPECT = W / H
OUTSIDE, INSIDE = np.array([1.8, 0.7, 1.1]), np.array([0.11, 0.05, -0.07])
SHUTTER = (-0.25, 1.5)                                 # outside every one of query_regimes.TIME_GROUPS
TELE_DISTANCES = (1.0e6, 1.1e6, 1e9)                   # 2^20 = 1 048 576 lies between the first two
CLOSEUP_REGIMES, TELE_REGIMES = ("dense", "dense_ties", "dense2"), ("dense", "groups")
# `behind`: 1e9 units away on the far side of the WORLD origin, which then lies between the camera and the scene, on the axis: the
# layouts' padding records (centre 0, r^2 = -1) sit there, and from that far the reference's rounding "hits" such a sphere
BEHIND, BEHIND_REGIMES = "behind_1e+09", ("far", "dense2", "far_x5")   # (from there `dense` shows the underside of its ground alone)


def base_of(name):
    if name in TILED:
        return TILED[name][0]
    return name if name in Q.BASE else "dense"


def spread_of(name):
    return float(Q._SPECS[base_of(name)]["spread"])


def scene(name, seed=0):
    """(n, 16) float64 records."""
    if name == "dense_ties":
        recs = Q.scene("dense", seed)
        dup = recs[-N_DUPLICATES:]
        dup[:, 10] = (dup[:, 10] + 1) % 3              # another material kind
        dup[:, 11:14] = 1.05 - dup[:, 11:14]           # another albedo, still in 0.1 .. 0.95
        return recs
    if name in TILED:
        base, copies = TILED[name]
        one = Q.scene(base, seed)
        out = []
        for k in range(copies):
            c = one.copy()
            c[:, 1:4] += k * TILE_STEP * spread_of(name)
            c[:, 4:7] += k * TILE_STEP * spread_of(name)
            out.append(c)
        return np.concatenate(out)
    return Q.scene(name, seed)


def duplicate_pairs(recs):
    """[(duplicate, original)] of a dense / dense_ties list: the trailing records and the earlier record of the same geometry."""
    recs = np.asarray(recs)
    n = len(recs) - N_DUPLICATES
    pairs = []
    for j in range(n, len(recs)):
        same = np.flatnonzero((recs[:n, :10] == recs[j, :10]).all(axis=1))
        assert same.size == 1
        pairs.append((j, int(same[0])))
    return pairs


def swapped(recs):
    """The list with every duplicate and its original exchanged: the same spheres, the other one of each pair first."""
    out = np.array(recs, copy=True)
    for j, i in duplicate_pairs(recs):
        out[[i, j]] = out[[j, i]]
    return out


def camera_names(name):
    names = ["outside", "inside"]
    if name in CLOSEUP_REGIMES:
        names.append("closeup")
    if name in TELE_REGIMES:
        names += [f"tele_{d:g}" for d in TELE_DISTANCES]
    if name in BEHIND_REGIMES:
        names.append(BEHIND)
    return names


CASES = tuple((name, cam) for name in REGIMES for cam in camera_names(name))


def densest_spot(recs, radius):
    """The object centre with the most other centres within `radius`."""
    c = Q._placeable(recs)[:, 1:4]
    d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    return c[int(np.argmax((d2 <= radius * radius).sum(axis=1)))]


def camera(name, cam, recs=None, seed=0):
    """The keyword arguments of tor.camera() (oracle.camera() takes the same values under its own names, see oracle_camera())."""
    recs = scene(name, seed) if recs is None else recs
    spread = spread_of(name)
    rscale = spread / 12.0
    lo, hi = Q._box(Q._placeable(recs))
    centre = 0.5 * (lo + hi)
    unit = OUTSIDE / np.linalg.norm(OUTSIDE)
    if cam in ("outside", "inside"):
        look_from = centre + (OUTSIDE if cam == "outside" else INSIDE) * spread
        look_at, fov, aperture, shutter = centre, 40.0, 0.05 * rscale, SHUTTER
    elif cam == "closeup":
        look_at = densest_spot(recs, 0.25 * rscale)
        look_from = look_at + unit * 6.0 * rscale
        fov, aperture, shutter = float(np.degrees(2.0 * np.arctan(0.6 * rscale / (6.0 * rscale)))), 0.0, SHUTTER
    elif cam.startswith("tele_"):
        dist = float(cam[5:])
        look_at, look_from = centre, centre + unit * dist
        fov, aperture, shutter = float(np.degrees(2.0 * np.arctan(0.6 * spread / dist))), 0.0, SHUTTER
    elif cam == BEHIND:
        dist = 1e9
        look_at, look_from = centre, centre - centre / np.linalg.norm(centre) * dist
        fov, aperture, shutter = float(np.degrees(2.0 * np.arctan(0.6 * spread / dist))), 0.0, SHUTTER
    else:
        raise KeyError(cam)
    return dict(look_from=tuple(float(v) for v in look_from), look_at=tuple(float(v) for v in look_at), vertical_field_of_view=fov,
                aspect_ratio=ASPECT, aperture=float(aperture), focus_distance=float(np.linalg.norm(look_from - look_at)),
                shutter_open=shutter[0], shutter_close=shutter[1])


def oracle_camera(oracle, kw):
    return oracle.camera(look_from=kw["look_from"], look_at=kw["look_at"], vfov=kw["vertical_field_of_view"], aspect=kw["aspect_ratio"],
                         aperture=kw["aperture"], focus_dist=kw["focus_distance"], shutter_open=kw["shutter_open"],
                         shutter_close=kw["shutter_close"])


def pixel_centre_rays(kw, h=H, w=W):
    """(origin (3,), directions (h * w, 3)) of a pinhole camera through the pixel centres (cameras.nim's basis, no lens)."""
    o, at = np.array(kw["look_from"]), np.array(kw["look_at"])
    wv = (o - at) / np.linalg.norm(o - at)
    u = np.cross([0.0, 1.0, 0.0], wv)
    u /= np.linalg.norm(u)
    v = np.cross(wv, u)
    half_h = np.tan(np.radians(kw["vertical_field_of_view"]) / 2.0)
    half_w = kw["aspect_ratio"] * half_h
    s, t = np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h)
    d = -wv + ((2 * s - 1) * half_w)[..., None] * u + ((2 * t - 1) * half_h)[..., None] * v
    return o, d.reshape(-1, 3)


def spheres_crossed(recs, o, d, time=0.0):
    """Per ray, the spheres whose discriminant is > 0 in plain float64 (the line, not the half line), movers at `time`."""
    recs = Q._placeable(recs)
    dt = recs[:, 8] - recs[:, 7]
    moving = (recs[:, 0] == 1) & (dt != 0)
    with np.errstate(all="ignore"):
        f = np.where(moving, (time - recs[:, 7]) / np.where(dt != 0, dt, 1.0), 0.0)
    c = recs[:, 1:4] + f[:, None] * (recs[:, 4:7] - recs[:, 1:4])
    keep = (recs[:, 0] == 0) | moving                  # (a time0 == time1 mover has no finite fraction: never hit)
    c, r = c[keep], recs[keep, 9]
    oc = o[None, :] - c                                # (n, 3)
    a = (d * d).sum(axis=1)                            # (rays,)
    half_b = d @ oc.T                                  # (rays, n)
    cc = (oc * oc).sum(axis=1) - r * r
    return ((half_b * half_b - a[:, None] * cc[None, :]) > 0).sum(axis=1)


# ---- which integrate_kernel build a lane launch runs -----------------------------------------------------------------------------
F32_LIMIT = 2.0 ** 19                                  # tor_filter32.hpp: kF32Lim / 2 bounds |c0 - P| and |dc|; r^2 in 2^-40 .. 2^40


def _f32_eligible(recs):
    """Per object: may the float32 filter take it (tor_scene.cpp f32_options_for / build_layout, tor_filter32.hpp f32_eligible)?
    P is the per-axis median of the finite (start) centres, the limit 8 x the median distance from P."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    with np.errstate(all="ignore"):
        c0 = recs[:, 1:4]
        fin = np.isfinite(c0).all(axis=1)
        mid = int(fin.sum()) // 2
        origin = np.sort(c0[fin], axis=0)[mid]
        far_limit = 8.0 * np.sort(np.sqrt(((c0[fin] - origin) ** 2).sum(axis=1)))[mid]
        if not (far_limit > 0 and np.isfinite(far_limit)):
            far_limit = 0.0
        mc0 = np.sqrt(((c0 - origin) ** 2).sum(axis=1))
        moving = recs[:, 0] == 1
        dcn = np.where(moving, np.sqrt(((recs[:, 4:7] - c0) ** 2).sum(axis=1)), 0.0)
        dt = recs[:, 8] - recs[:, 7]
        r2 = recs[:, 9] ** 2
        ok = np.isfinite(mc0) & np.isfinite(dcn) & np.isfinite(r2) & (mc0 <= F32_LIMIT) & (dcn <= F32_LIMIT) & (r2 >= 2.0 ** -40) & (r2 <= 2.0 ** 40)
        ok &= mc0 <= far_limit
        ok &= ~moving | (np.isfinite(recs[:, 7]) & np.isfinite(dt) & (dt != 0))
    return ok


def time_groups_in_blocks(recs, layout):
    """The distinct (time0, time1) of the movers that the culling layout sorts into blocks."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    slots = np.asarray(layout[0]).reshape(-1)
    in_blocks = recs[slots[slots >= 0]]
    return {(float(a), float(b)) for a, b in in_blocks[in_blocks[:, 0] == 1][:, 7:9]}


def expected_variant(recs, layout, accel, seeding, screen=True):
    """(seeding, arith, f32, blocks) of tor_debug_last_variant (its W field left out) for a lane launch with the accel bits `accel`
    on a context whose FMA screen is `screen`; `layout` is tor.debug_accel_layout over the launch's ray-time range (not None here).
      * no accel bit: the brute force, behind the FMA screen (ARITH 2) unless the context has none
      * TOR_ACCEL_F32 alone: the float32 filter in front of the flat list (F32 1) when any object qualifies for it
      * TOR_ACCEL_BLOCKS alone: the float64 block expansion (BLOCKS 1), single or two-level alike
      * both: the cooperative resolve on float32 block records, BLOCKS 1 single-level and 2 two-level -- but those records hold ONE
        time group and only objects the filter may take: with several groups among the blocks' movers, or one object out of the
        filter's range, the whole launch stays on the float64 layout and runs the float64 block expansion (0, 0, 1) whatever the
        levels (tor_api.cpp configure_layout(): v32 = 0; DESIGN: "The float32 block records need ONE time group")."""
    assert layout is not None
    ok32 = _f32_eligible(recs)
    slots = np.asarray(layout[0]).reshape(-1)
    records32 = len(time_groups_in_blocks(recs, layout)) <= 1 and bool(ok32[slots[slots >= 0]].all())
    if accel == 0:
        return (seeding, 2 if screen else 0, 0, 0)
    if accel == 2:
        return (seeding, 0, 1, 0) if ok32.any() else (seeding, 2 if screen else 0, 0, 0)
    if accel == 1 or not records32:
        return (seeding, 0, 0, 1)
    return (seeding, 0, 1, 2 if layout[3] else 1)


def migrate_variant(seeding, f32, blocks):
    """tor_kernels.hip: the builds that carry the chain servers."""
    return seeding == 0 and f32 != 0 and blocks == 1


FAMILIES = ("screened brute force (2, 0, 0)", "unscreened brute force (0, 0, 0)", "float32 filter alone (0, 1, 0)",
            "float64 blocks (0, 0, 1), single-level", "float64 blocks (0, 0, 1), two-level", "cooperative resolve (0, 1, 1), single-level",
            "cooperative resolve (0, 1, 2), two-level", "two-level with several time groups, both accelerations")


def families_of(variant, accel, two_level, n_groups):
    """The names in FAMILIES a launch with tor_debug_last_variant `variant` counts for."""
    key = tuple(variant[k] for k in (1, 3, 4))
    out = []
    if key == (2, 0, 0):
        out.append(FAMILIES[0])
    if key == (0, 0, 0):
        out.append(FAMILIES[1])
    if key == (0, 1, 0):
        out.append(FAMILIES[2])
    if key == (0, 0, 1):
        out.append(FAMILIES[4 if two_level else 3])
    if key == (0, 1, 1) and not two_level:
        out.append(FAMILIES[5])
    if key == (0, 1, 2) and two_level:
        out.append(FAMILIES[6])
    if accel == 3 and two_level and n_groups > 1:
        out.append(FAMILIES[7])
    return out
