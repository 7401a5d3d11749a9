"""An independent numpy restatement of include/tor_texture.h: per hit record the colour and the texel of the texture bound to the
record's object -- a constant, a 3-D checker of p or of the outward normal, an octahedral image looked up by the outward normal
(nearest, or bilinear with the fold's seam rule) -- or the scatter's attenuation for an object without a texture; and of the
wavefront loop of Context.trace(textures=True) built on bounce_restatement.step.

One record at a time, on Python floats (IEEE float64, single roundings, never fused), in the header's operation order.  It shares
no code with the library.  `variant` switches ONE line of the definition to a plausible mistake; tests/test_texture_query.py shows
which named case of tests/texture_inputs.py tells each apart.  `loads` collects every (texture, row, col) the restatement reads,
so that a test can show they are all in range."""
import math

import numpy as np

import bounce_restatement as BR
import hit_restatement as H

CONSTANT, CHECKER, IMAGE = 0, 1, 2
WORLD, NORMAL = 0, 1
NEAREST, BILINEAR = 0, 1
TEXTURE_MAX, TEXTURE_MAX_SIDE, TEXTURE_MAX_TEXELS = 4096, 2048, 1 << 22
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2
BIG = 2.0 ** 52
INF = float("inf")
VARIANTS = ("clamp_seam", "shading_normal", "rows_from_s", "truncate", "no_half", "no_fold", "spaces_swapped", "offset_ignored",
            "lerp_rows_first", "dielectric_albedo")


def constant(rgb):
    return dict(kind=CONSTANT, option=0, a=tuple(map(float, rgb)), b=(0.0,) * 3, freq=(0.0,) * 3, rgb=None)


def checker(even, odd, freq, space=WORLD):
    f = tuple(float(x) for x in np.broadcast_to(np.asarray(freq, dtype=np.float64), (3,)))
    return dict(kind=CHECKER, option=space, a=tuple(map(float, even)), b=tuple(map(float, odd)), freq=f, rgb=None)


def image(rgb, filt=NEAREST):
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    assert rgb.ndim == 3 and rgb.shape[0] == rgb.shape[1] and rgb.shape[2] == 3
    return dict(kind=IMAGE, option=filt, a=(0.0,) * 3, b=(0.0,) * 3, freq=(0.0,) * 3, rgb=rgb)


def pack(textures):
    """(records with side and offset, the (n_texels, 3) atlas): the images one after the other in list order."""
    out, parts, at = [], [], 0
    for t in textures:
        t = dict(t, side=0, offset=0)
        if t["kind"] == IMAGE:
            t["side"], t["offset"] = int(t["rgb"].shape[0]), at
            parts.append(t["rgb"].reshape(-1, 3))
            at += t["side"] ** 2
        out.append(t)
    return out, (np.concatenate(parts) if parts else np.zeros((0, 3)))


def make_hits(p, normal, obj, front, t=1.0):
    """(n, 8) TorHit records: p, normal, t, then object and front_face as the halves of word 7."""
    p, normal = np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(normal, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    raw = np.zeros((n, 8))
    raw[:, 0:3], raw[:, 3:6], raw[:, 6] = p, normal, t
    w = raw.view(np.int32)
    w[:, 14], w[:, 15] = np.broadcast_to(np.asarray(obj, dtype=np.int64), (n,)).astype(np.int32), np.broadcast_to(np.asarray(front), (n,))
    return raw


def _floor(x):
    return float(np.floor(x))


def _clamp(v, n):
    return 0 if v < 0 else (n - 1 if v > n - 1 else v)


def encode(m, variant=None):
    """tor_env.h's encode of the direction m: (s, t), or None for an unusable direction."""
    mx, my, mz = m
    L1 = abs(mx) + abs(my) + abs(mz)
    if not (L1 > 0.0 and L1 < INF):
        return None
    qx, qz = mx / L1, mz / L1
    if my >= 0.0 or variant == "no_fold":
        return qx, qz
    return math.copysign(1.0 - abs(qz), qx), math.copysign(1.0 - abs(qx), qz)


def cell(w, n):
    f = _floor((w + 1.0) * (0.5 * float(n)))
    return int(f) if 0.0 < f < float(n - 1) else (n - 1 if f > 0.0 else 0)


def seam(n, r, c, variant=None):
    if variant == "clamp_seam":
        return _clamp(r, n), _clamp(c, n)
    if c < 0 or c > n - 1:
        r, c = (n - 1) - r, _clamp(c, n)
    if r < 0 or r > n - 1:
        c, r = (n - 1) - c, _clamp(r, n)
    return r, c


def bilinear_corners(s, t, n, variant=None):
    """((r, c) of T00, T01, T10, T11 after the seam rule, al, be)."""
    half = 0.0 if variant == "no_half" else 0.5
    u, v = (s + 1.0) * (0.5 * float(n)) - half, (t + 1.0) * (0.5 * float(n)) - half
    fc, fr = _floor(u), _floor(v)
    al, be = u - fc, v - fr

    def as_int(f):
        return -1 if not f >= -1.0 else (n - 1 if f > float(n - 1) else int(f))
    c0, r0 = as_int(fc), as_int(fr)
    return [seam(n, r, c, variant) for r, c in ((r0, c0), (r0, c0 + 1), (r0 + 1, c0), (r0 + 1, c0 + 1))], al, be


def eval_one(recs, table, atlas, binding, h, variant=None, loads=None):
    """(colour (3,), texel) of one 8-word record h."""
    obj, front = int(h.view(np.int32)[14]), int(h.view(np.int32)[15])
    if obj < 0 or obj >= len(recs):
        return (0.0, 0.0, 0.0), -1
    b = int(binding[obj])
    if b == -1:
        o = recs[obj]
        mat = int(o[10])
        if mat == MAT_DIELECTRIC:
            return ((float(o[15]), 0.0, 0.0) if variant == "dielectric_albedo" else (1.0, 1.0, 1.0)), -1
        return (float(o[11]), float(o[12]), float(o[13])), -1
    T = table[b]
    p = tuple(float(x) for x in h[0:3])
    nrm = tuple(float(x) for x in h[3:6])
    m = nrm if (front != 0 or variant == "shading_normal") else tuple(-x for x in nrm)
    if T["kind"] == CONSTANT:
        return T["a"], 0
    if T["kind"] == CHECKER:
        world = (T["option"] == WORLD) != (variant == "spaces_swapped")
        x = p if world else m
        rnd = (lambda z: float(np.trunc(z))) if variant == "truncate" else _floor
        f = [rnd(x[k] * T["freq"][k]) for k in range(3)]
        if any(not abs(fk) < BIG for fk in f):
            return T["a"], -1
        par = [fk - 2.0 * _floor(fk * 0.5) for fk in f]
        assert all(q in (0.0, 1.0) for q in par)
        odd = (int(par[0]) + int(par[1]) + int(par[2])) & 1
        return (T["b"] if odd else T["a"]), odd
    n, off = T["side"], (0 if variant == "offset_ignored" else T["offset"])
    st = encode(m, variant)
    if st is None:
        return (0.0, 0.0, 0.0), -1
    s, t = st
    if variant == "rows_from_s":
        s, t = t, s

    def load(r, c):
        if loads is not None:
            loads.append((b, n, r, c))
        return atlas[off + r * n + c]
    cn, rn = cell(s, n), cell(t, n)
    if T["option"] == NEAREST:
        return tuple(float(x) for x in load(rn, cn)), rn * n + cn
    corners, al, be = bilinear_corners(s, t, n, variant)
    t00, t01, t10, t11 = (load(r, c) for r, c in corners)
    if variant == "lerp_rows_first":
        col = tuple((((1.0 - be) * float(t00[k]) + be * float(t10[k])) * (1.0 - al)) + (((1.0 - be) * float(t01[k]) + be * float(t11[k])) * al)
                    for k in range(3))
    else:
        col = tuple((((1.0 - al) * float(t00[k]) + al * float(t01[k])) * (1.0 - be)) + (((1.0 - al) * float(t10[k]) + al * float(t11[k])) * be)
                    for k in range(3))
    return col, rn * n + cn


def evaluate(recs, textures, binding, hits, index=None, out=None, variant=None, loads=None):
    """{"color": (n, 3), "texel": (n,) int32} for the listed records; records that are not listed keep what `out` holds, else
    colour 0 and texel -1."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    hits = np.ascontiguousarray(hits, dtype=np.float64).reshape(-1, 8)
    table, atlas = pack(textures)
    n = hits.shape[0]
    color = np.zeros((n, 3)) if out is None else out["color"]
    texel = np.full(n, -1, dtype=np.int32) if out is None else out["texel"]
    ids = np.arange(n) if index is None else np.asarray(index, dtype=np.int64).reshape(-1)
    with np.errstate(all="ignore"):
        for i in ids[(ids >= 0) & (ids < n)]:
            color[i], texel[i] = eval_one(recs, table, atlas, binding, hits[i], variant, loads)
    return {"color": color, "texel": texel}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mismatches(got, want):
    """The fields whose bits differ (NaNs compare by their bits: the definition makes none from usable inputs)."""
    bad = []
    if not np.array_equal(bits(got["color"]), bits(want["color"])):
        rows = np.nonzero((bits(got["color"]) != bits(want["color"])).reshape(len(want["texel"]), 3).any(axis=1))[0]
        bad.append(("color", rows[:8].tolist(), len(rows)))
    if not np.array_equal(np.asarray(got["texel"]), want["texel"]):
        rows = np.nonzero(np.asarray(got["texel"]) != want["texel"])[0]
        bad.append(("texel", rows[:8].tolist(), len(rows)))
    return bad


def trace(oracle, recs, textures, binding, rays, states, max_depth, emission=None):
    """The wavefront loop of Context.trace(textures=True) on bounce_restatement.step: after each step the colours of the stepped
    records, and att *= colour for the rays that scattered.  (color (n, 3), states (n, 4) uint64)."""
    rays = np.array(rays, dtype=np.float64).reshape(-1, 7)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    n = rays.shape[0]
    color, att = np.zeros((n, 3)), np.ones((n, 3))
    live = np.arange(n)
    res, tex = None, None
    with np.errstate(all="ignore"):
        for _ in range(max_depth):
            if live.size == 0:
                break
            res = BR.step(oracle, recs, rays, st, live, res)
            rays, st = res["rays"], res["states"]
            status = res["status"][live]
            miss = live[status == BR.MISS]
            if miss.size:
                color[miss] = BR.sky(rays, miss)[miss] * att[miss]
            if emission is not None:
                hit = live[status != BR.MISS]
                color[hit] = color[hit] + att[hit] * np.asarray(emission, dtype=np.float64)[H.fields(res["raw"])["object"][hit]]
            tex = evaluate(recs, textures, binding, res["raw"], live, tex)
            live = live[status == BR.SCATTERED]
            att[live] = att[live] * tex["color"][live]
    return color, st
