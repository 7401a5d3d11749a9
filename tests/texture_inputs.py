"""The named inputs of the surface-texture tests (include/tor_texture.h): per case a scene (recs, (n, 16) records), a list of
textures (texture_restatement's dicts), a binding and about 250 hit records -- the smallest at which the kernel can go wrong.
assert_coverage() shows that each case does what its name says.  Used by tests/test_texture_query.py (CPU, on the restatement)
and tests/test_gpu_texture_query.py (on the MI355X)."""
import math

import numpy as np

import texture_restatement as R

ULP = 2.0 ** -52


def sphere(c, radius, mat=0, albedo=(0.5, 0.5, 0.5), fuzz=0.0, ri=1.5):
    r = np.zeros(16)
    r[0], r[1:4], r[4:7], r[7:10], r[10] = 0, c, c, (0.0, 1.0, radius), mat
    if mat == 2:
        r[15] = ri
    else:
        r[11:14], r[14] = albedo, (fuzz if mat == 1 else 0.0)
    return r


def moving_sphere(c0, c1, t0, t1, radius, albedo=(0.5, 0.5, 0.5)):
    r = np.zeros(16)
    r[0], r[1:4], r[4:7], r[7:10], r[10], r[11:14] = 1, c0, c1, (t0, t1, radius), 0, albedo
    return r


def ramp(n, base=1.0):
    """An (n, n, 3) image with a distinct exact value per texel and channel."""
    return base + np.arange(n * n * 3, dtype=np.float64).reshape(n, n, 3) / 16.0


def decode(s, t):
    """tor_env.h's decode: the unit direction of the square's point (s, t)."""
    py = (1.0 - abs(s)) - abs(t)
    px, pz = (s, t) if py >= 0 else (math.copysign(1.0 - abs(t), s), math.copysign(1.0 - abs(s), t))
    inv = 1.0 / math.sqrt(px * px + py * py + pz * pz)
    return (px * inv, py * inv, pz * inv)


def unit_dirs(n, seed):
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3))
    return d / np.sqrt((d * d).sum(1))[:, None]


def records(m, obj, front=1, centre=(0.0, 0.0, 0.0), radius=1.0):
    """Records of the outward normals m on a sphere: p = centre + radius * m; the stored normal is m, or -m where front == 0."""
    m = np.asarray(m, dtype=np.float64).reshape(-1, 3)
    front = np.broadcast_to(np.asarray(front, dtype=np.int32), (len(m),))
    p = np.asarray(centre, dtype=np.float64) + radius * m
    return R.make_hits(p, np.where(front[:, None] != 0, m, -m), obj, front)


def case(name, recs, textures, binding, hits):
    return dict(name=name, recs=np.asarray(recs, dtype=np.float64).reshape(-1, 16), textures=list(textures),
                binding=np.asarray(binding, dtype=np.int32), hits=np.ascontiguousarray(hits, dtype=np.float64).reshape(-1, 8))


def _two_spheres():
    return [sphere((0, 0, 0), 1.0), sphere((3, 0, 0), 1.0)]


def image_case(n, seed):
    """Side n: object 0 NEAREST, object 1 BILINEAR, on 250 random outward normals, a third of them seen from behind."""
    m = unit_dirs(250, seed)
    obj = np.arange(250) % 2
    front = (np.arange(250) % 3 != 0).astype(np.int32)
    img = ramp(n)
    return case(f"n{n}", _two_spheres(), [R.image(img, R.NEAREST), R.image(img, R.BILINEAR)], [0, 1], records(m, obj, front))


def two_images():
    m = unit_dirs(252, 21)
    obj = np.arange(252) % 3
    recs = _two_spheres() + [sphere((6, 0, 0), 1.0)]
    return case("two_images", recs, [R.image(ramp(4), R.BILINEAR), R.image(ramp(3, 100.0), R.NEAREST)], [0, 1, 0], records(m, obj))


SEAM_N = 8


def seam_normals():
    out = []
    tiny = (0.0, -0.0, 1e-17, -1e-17, 1e-16, -1e-16, 3e-16, -3e-16)
    for a in (0.6, -0.87):
        for z in tiny:                                       # |s| = 1 and |t| = 1 exactly and within a few ulps (lower hemisphere)
            out += [(a, -(1.0 - abs(a)), z), (z, -(1.0 - abs(a)), a)]
    for sx in (1.0, -1.0):                                   # the four corners: the pole -y and its neighbourhood
        for sz in (1.0, -1.0):
            for e in (0.0, 1e-17, 1e-3, 0.04):
                out.append((sx * e, -1.0, sz * e))
    g = np.random.default_rng(5)
    h = 2.0 / SEAM_N
    for _ in range(22):                                      # within half a texel of the square's edge
        e, w, sg = float(g.uniform(0, 0.5 * h)), float(g.uniform(-1, 1)), float(g.choice([-1.0, 1.0]))
        out += [decode(sg * (1.0 - e), w), decode(w, sg * (1.0 - e))]
    for _ in range(8):                                       # the crease |s| + |t| = 1, from both hemispheres
        s = float(g.uniform(-1, 1))
        t = float(g.choice([-1.0, 1.0])) * (1.0 - abs(s))
        for k in (-2, 0, 2):
            out.append(decode(s, t * (1.0 + k * ULP)))
        out += [(s, 1e-17, t), (s, -1e-17, t)]
    return np.asarray(out, dtype=np.float64)


def seam():
    m = seam_normals()
    m = np.concatenate([m, m])
    obj = np.repeat([0, 1], len(m) // 2)
    img = ramp(SEAM_N)
    return case("seam", _two_spheres(), [R.image(img, R.NEAREST), R.image(img, R.BILINEAR)], [0, 1], records(m, obj))


def axes():
    out = []
    for k in range(3):
        for sg in (1.0, -1.0):
            for z0 in (0.0, -0.0):
                for z1 in (0.0, -0.0):
                    v = [z0, z1]
                    v.insert(k, sg)
                    out.append(tuple(v))
    for x, z in ((0.3, 0.7), (-0.3, 0.7), (0.3, -0.7), (-0.5, -0.5), (1.0, 0.0), (0.0, -1.0)):
        out += [(x, -0.0, z), (x, 0.0, z)]                   # m.y == -0.0 is the upper half: no fold
    m = np.asarray(out, dtype=np.float64)
    m = np.concatenate([m, m])
    obj = np.repeat([0, 1], len(m) // 2)
    img = ramp(4)
    return case("axes", _two_spheres(), [R.image(img, R.NEAREST), R.image(img, R.BILINEAR)], [0, 1], records(m, obj))


def centres():
    out = []
    for n in (8, 3):
        h = 2.0 / n
        out += [decode((c + 0.5) * h - 1.0, (r + 0.5) * h - 1.0) for r in range(n) for c in range(n)]
    m = np.asarray(out, dtype=np.float64)
    obj = np.concatenate([np.zeros(64, dtype=int), np.full(9, 2)])
    m, obj = np.concatenate([m, m]), np.concatenate([obj, obj + 1])
    recs = _two_spheres() + [sphere((6, 0, 0), 1.0), sphere((9, 0, 0), 1.0)]
    tex = [R.image(ramp(8), R.NEAREST), R.image(ramp(8), R.BILINEAR), R.image(ramp(3), R.NEAREST), R.image(ramp(3), R.BILINEAR)]
    return case("centres", recs, tex, [0, 1, 2, 3], records(m, obj))


def unusable():
    nan, inf = float("nan"), float("inf")
    vs = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (nan, 0.0, 1.0), (0.0, nan, 0.0), (1.0, 1.0, nan), (inf, 0.0, 0.0), (0.0, -inf, 1.0),
          (1e308, 1e308, 1e308), (-1e308, 1e308, 0.0), (1e308, 0.0, 0.0), (0.0, -1e308, 0.0), (5e-324, 0.0, 0.0), (1e-310, -1e-310, 0.0),
          (0.3, 0.4, 0.5)]
    rows = []
    for obj in range(4):                                     # image nearest, image bilinear, checker world, checker normal
        for v in vs:
            for front in (1, 0):
                rows.append(R.make_hits([v], [v], obj, front))   # the point and the normal both hold the vector
    recs = _two_spheres() + [sphere((6, 0, 0), 1.0), sphere((9, 0, 0), 1.0)]
    tex = [R.image(ramp(4), R.NEAREST), R.image(ramp(4), R.BILINEAR), R.checker((0.9, 0.1, 0.1), (0.1, 0.1, 0.9), (2.0, 1e10, 1.0), R.WORLD),
           R.checker((0.9, 0.1, 0.1), (0.1, 0.1, 0.9), (3.0, 3.0, 3.0), R.NORMAL)]
    return case("unusable", recs, tex, [0, 1, 2, 3], np.concatenate(rows))


def _hit_record(rec, obj, origin, direction, root):
    """The record the library writes for the ray's root on a static sphere (tor_render.h: outward = (p - c) * (1 / radius), front
    = dot(d, outward) < 0, the normal negated when not front)."""
    c, radius = rec[1:4], rec[9]
    o, d = np.asarray(origin, dtype=np.float64), np.asarray(direction, dtype=np.float64)
    oc = o - c
    a, hb, cc = d @ d, oc @ d, oc @ oc - radius * radius
    sq = math.sqrt(hb * hb - a * cc)
    t = (-hb - sq) / a if root == 0 else (-hb + sq) / a
    p = o + d * t
    outward = (p - c) * (1.0 / radius)
    front = 1 if d @ outward < 0 else 0
    return R.make_hits([p], [outward if front else -outward], obj, front, t)


def back_face():
    recs = [sphere((0, 0, 0), 1.0), sphere((3, 0, 0), -1.0), sphere((6, 0, 0), 1.0, mat=2), sphere((9, 0, 0), -0.5)]
    tex = [R.image(ramp(8), R.BILINEAR), R.image(ramp(8), R.NEAREST), R.checker((1, 0, 0), (0, 1, 0), 2.0, R.NORMAL),
           R.checker((1, 0, 0), (0, 1, 0), 2.0, R.WORLD)]
    g = np.random.default_rng(9)
    rows = []
    for i in range(120):
        obj = i % 4
        c = recs[obj][1:4]
        d = unit_dirs(1, 100 + i)[0]
        o = c - 4.0 * d + g.uniform(-0.3, 0.3, size=3)
        rows.append(_hit_record(recs[obj], obj, o, d, 0))    # from outside: the first root
        rows.append(_hit_record(recs[obj], obj, o, d, 1))    # the far side: seen from inside
    return case("back_face", recs, tex, [0, 1, 2, 3], np.concatenate(rows))


MOVING_TIMES = (0.0, 0.4, 1.0)


def moving():
    c0, c1 = np.array([0.0, 0.0, 0.0]), np.array([1.3, 0.7, -0.4])
    recs = [moving_sphere(c0, c1, 0.0, 1.0, 0.5), moving_sphere(c0, c1, 0.0, 1.0, 0.5)]
    tex = [R.checker((1, 1, 1), (0, 0, 0), 3.0, R.NORMAL), R.checker((1, 1, 1), (0, 0, 0), 3.0, R.WORLD)]
    m = unit_dirs(42, 13)
    rows = []
    for obj in (0, 1):
        for time in MOVING_TIMES:
            centre = c0 + ((time - 0.0) / (1.0 - 0.0)) * (c1 - c0)
            rows.append(records(m, obj, 1, centre, 0.5))
    return case("moving", recs, tex, [0, 1], np.concatenate(rows))


def checker_edges():
    recs = [sphere((0, 0, 0), 1.0) for _ in range(4)]
    even, odd = (0.8, 0.8, 0.1), (0.1, 0.2, 0.7)
    tex = [R.checker(even, odd, (2.0, 0.5, 1.0), R.WORLD), R.checker(even, odd, (0.0, 0.0, 0.0), R.WORLD),
           R.checker(even, odd, (-1.0, -2.0, -0.5), R.WORLD), R.checker(even, odd, (1.0, 1.0, 1.0), R.WORLD)]
    pts = []
    for k in (-3, -2, -1, 0, 1, 2, 5):                       # x * freq exactly integral, and one ulp to either side
        x = k / 2.0
        for v in (x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)):
            pts += [(0, (v, 0.25, 0.25)), (0, (0.25, 2.0 * k + 0.0, v)), (2, (v, 0.1, 0.1)), (3, (v, v, v))]
    for v in (-0.25, -0.75, -1.5, -2.25, -1e-300, -5e-324):  # negative coordinates: floor, not truncation
        pts += [(0, (v, 0.25, 0.25)), (3, (0.5, v, 0.5)), (3, (v, v, v)), (2, (v, -v, v))]
    for v in (0.3, -7.7, 1e300, -1e300):                     # freq 0: every point is even
        pts.append((1, (v, -v, v)))
    big = 2.0 ** 52
    for v in (big, -big, big - 1.0, -(big - 1.0), big - 2.0, 2.0 ** 53, 1e300, 2.0 ** 51 + 0.5, -(2.0 ** 51) - 0.5):
        pts += [(3, (v, 0.5, 0.5)), (3, (0.5, 0.5, v)), (0, (v, 0.5, 0.5)), (2, (0.5, v, 0.5))]
    for p in ((1.5, 1.5, 1.5), (-0.5, 1.5, 3.5), (1.5, 0.5, 0.5), (1.5, 1.5, 0.5), (0.5, 0.5, 0.5), (-0.5, -0.5, -0.5)):
        pts.append((3, p))                                   # parity sums 3, 3, 1, 2, 0, 3
    g = np.random.default_rng(17)
    for i in range(60):
        pts.append((i % 4, tuple(g.uniform(-4, 4, size=3))))
    obj = np.array([o for o, _ in pts])
    p = np.array([q for _, q in pts], dtype=np.float64)
    return case("checker_edges", recs, tex, [0, 1, 2, 3], R.make_hits(p, unit_dirs(len(p), 3), obj, 1))


def untextured():
    recs = [sphere((0, 0, 0), 1.0, 0, (0.1, 0.2, 0.3)), sphere((3, 0, 0), 1.0, 1, (0.7, 0.6, 0.5), 0.0),
            sphere((6, 0, 0), 1.0, 1, (0.9, 0.8, 0.25), 0.3), sphere((9, 0, 0), 1.0, 2, ri=1.5), sphere((12, 0, 0), 1.0, 0, (0.4, 0.4, 0.4))]
    m = unit_dirs(250, 31)
    return case("untextured", recs, [R.constant((0.25, 0.5, 0.75))], [-1, -1, -1, -1, 0], records(m, np.arange(250) % 5, np.arange(250) % 2))


def no_object():
    recs = _two_spheres()
    m = unit_dirs(240, 41)
    obj = np.array([-1, 2, -2 ** 31, 0, 1, 3, 2 ** 31 - 1, -7])[np.arange(240) % 8]
    return case("no_object", recs, [R.image(ramp(2), R.BILINEAR), R.constant((0.5, 0.25, 0.125))], [0, 1], records(m, obj))


def wave16():
    recs = [sphere((3.0 * k, 0, 0), 1.0, mat, alb) for k, (mat, alb) in enumerate(
        [(0, (0.5, 0.5, 0.5))] * 5 + [(0, (0.2, 0.3, 0.4)), (2, (0, 0, 0))])]
    tex = [R.constant((0.3, 0.6, 0.9)), R.checker((1, 0.5, 0), (0, 0.5, 1), (1.5, 2.5, 3.5), R.WORLD),
           R.checker((1, 0.5, 0), (0, 0.5, 1), 4.0, R.NORMAL), R.image(ramp(5), R.NEAREST), R.image(ramp(5), R.BILINEAR)]
    m = unit_dirs(257, 51)
    obj = np.where(np.arange(257) % 8 == 7, -1, np.arange(257) % 8)
    centre = np.stack([3.0 * np.clip(obj, 0, 6), np.zeros(257), np.zeros(257)], axis=1)
    hits = R.make_hits(centre + m, np.where((np.arange(257) % 5 != 0)[:, None], m, -m), obj, (np.arange(257) % 5 != 0).astype(np.int32))
    return case("wave16", recs, tex, [0, 1, 2, 3, 4, -1, -1], hits)


def lists(n=257):
    """The lists of the wave16 tests by length: unique entries, some outside [0, n)."""
    g = np.random.default_rng(61)
    out = {}
    for length in (1, 63, 64, 65, 255):
        idx = g.permutation(n)[:length].astype(np.int64)
        if length > 1:
            idx[length // 2], idx[-1] = -1 - length, n + length
        out[length] = idx.astype(np.int32)
    return out


def _build():
    cs = [image_case(1, 1), image_case(2, 2), image_case(3, 3), image_case(8, 8), two_images(), seam(), axes(), centres(), unusable(),
          back_face(), moving(), checker_edges(), untextured(), no_object(), wave16()]
    return cs


CASES = _build()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
_answers = {}


def answer(name, variant=None):
    """The restatement's answer of a case: computed once, never changed."""
    key = (name, variant)
    if key not in _answers:
        c = BY_NAME[name]
        got = R.evaluate(c["recs"], c["textures"], c["binding"], c["hits"], variant=variant)
        got["color"].setflags(write=False)
        got["texel"].setflags(write=False)
        _answers[key] = got
    return _answers[key]


def _m(c):
    w = c["hits"].view(np.int32)
    return np.where((w[:, 15] != 0)[:, None], c["hits"][:, 3:6], -c["hits"][:, 3:6]), w[:, 14], w[:, 15]


def assert_coverage():
    """Each case does what its name says."""
    for name in ("n1", "n2", "n3", "n8"):
        c, a = BY_NAME[name], answer(name)
        n = int(name[1:])
        assert 240 <= len(c["hits"]) <= 260 and len(np.unique(c["textures"][0]["rgb"])) == n * n * 3
        assert set(np.unique(a["texel"])) == set(range(n * n)) if n < 8 else len(np.unique(a["texel"])) > 40
        assert (_m(c)[2] == 0).sum() > 60
    c = BY_NAME["two_images"]
    table, atlas = R.pack(c["textures"])
    assert [t["side"] for t in table] == [4, 3] and [t["offset"] for t in table] == [0, 16] and len(atlas) == 25 and len(c["recs"]) == 3
    assert sorted(c["binding"]) == [0, 0, 1]
    # seam: corners that the seam rule moves, on each edge, and a corner where both steps apply
    c = BY_NAME["seam"]
    m, obj, _ = _m(c)
    moved = {"left": 0, "right": 0, "bottom": 0, "top": 0, "both": 0}
    near_one, crease = 0, 0
    for v in m[obj == 1]:
        s, t = R.encode(tuple(float(x) for x in v))
        near_one += (abs(abs(s) - 1.0) <= 2 * ULP) + (abs(abs(t) - 1.0) <= 2 * ULP)
        crease += abs((abs(s) + abs(t)) - 1.0) <= 4 * ULP
        n = SEAM_N
        u, w = (s + 1.0) * (0.5 * n) - 0.5, (t + 1.0) * (0.5 * n) - 0.5
        c0, r0 = int(np.floor(u)), int(np.floor(w))
        moved["left"] += c0 < 0
        moved["right"] += c0 + 1 > n - 1
        moved["bottom"] += r0 < 0
        moved["top"] += r0 + 1 > n - 1
        moved["both"] += (c0 < 0 or c0 + 1 > n - 1) and (r0 < 0 or r0 + 1 > n - 1)
    assert min(moved.values()) >= 4 and near_one >= 40 and crease >= 20, (moved, near_one, crease)
    assert (m[:, 1] > 0).sum() >= 10 and (m[:, 1] < 0).sum() >= 100
    c = BY_NAME["axes"]
    m = _m(c)[0]
    assert sum(1 for v in m if sorted(np.abs(v)) == [0.0, 0.0, 1.0]) >= 48 and sum(1 for v in m if v[1] == 0 and np.signbit(v[1])) >= 12
    assert (np.signbit(m) & (m == 0)).any(axis=1).sum() >= 36
    # centres: al and be vanish up to rounding, so BILINEAR answers NEAREST's texel up to a few ulps
    c, a = BY_NAME["centres"], answer("centres")
    half = len(c["hits"]) // 2
    assert np.array_equal(a["texel"][:half], a["texel"][half:]) and np.array_equal(a["texel"][:64], np.arange(64))
    assert np.allclose(a["color"][:half], a["color"][half:], rtol=1e-12, atol=0)
    c, a = BY_NAME["unusable"], answer("unusable")
    assert (a["texel"] == -1).sum() >= 60 and (a["texel"] >= 0).sum() >= 16 and np.isnan(c["hits"][:, 0:6]).any() and np.isinf(c["hits"][:, 0:6]).any()
    assert (np.abs(c["hits"][:, 3:6]) == 1e308).any() and (c["hits"][:, 3:6] == 0).all(axis=1).any()
    c = BY_NAME["back_face"]
    _, obj, front = _m(c)
    for o in range(4):
        assert (front[obj == o] == 0).sum() >= 20 and (front[obj == o] == 1).sum() >= 20
    assert c["recs"][1][9] < 0 and c["recs"][3][9] < 0
    c, a = BY_NAME["moving"], answer("moving")
    k = 42
    nrm, wld = a["texel"][:3 * k].reshape(3, k), a["texel"][3 * k:].reshape(3, k)
    assert c["recs"][0][0] == 1 and (nrm[0] == nrm[1]).all() and (nrm[0] == nrm[2]).all() and (wld[0] != wld[1]).any() and (wld[0] != wld[2]).any()
    assert np.array_equal(c["hits"][:k, 3:6], c["hits"][k:2 * k, 3:6]) and not np.array_equal(c["hits"][:k, 0:3], c["hits"][k:2 * k, 0:3])
    c, a = BY_NAME["checker_edges"], answer("checker_edges")
    obj = _m(c)[1]
    assert set(np.unique(a["texel"])) == {-1, 0, 1} and (a["texel"] == -1).sum() >= 10 and (a["texel"][obj == 1] == 0).all()
    assert (c["hits"][:, 0:3] < 0).any() and any(f < 0 for f in c["textures"][2]["freq"]) and c["textures"][1]["freq"] == (0.0, 0.0, 0.0)
    p3 = c["hits"][obj == 3][:, 0:3]
    assert any((np.floor(q) % 2 == 1).all() for q in p3 if np.isfinite(q).all() and (np.abs(q) < 100).all())      # a parity sum of 3
    c, a = BY_NAME["untextured"], answer("untextured")
    assert [int(r[10]) for r in c["recs"][:4]] == [0, 1, 1, 2] and c["recs"][1][14] == 0 and c["recs"][2][14] != 0 and list(c["binding"][:4]) == [-1] * 4
    obj = _m(c)[1]
    assert (a["color"][obj == 3] == 1.0).all() and (a["color"][obj == 0] == c["recs"][0][11:14]).all() and (a["texel"][obj < 4] == -1).all()
    c, a = BY_NAME["no_object"], answer("no_object")
    obj = _m(c)[1]
    assert {-1, 2, -2 ** 31} <= set(obj.tolist()) and (a["texel"][(obj < 0) | (obj >= 2)] == -1).all() and (a["color"][(obj < 0) | (obj >= 2)] == 0).all()
    c, a = BY_NAME["wave16"], answer("wave16")
    assert len(c["hits"]) == 257 and sorted(lists()) == [1, 63, 64, 65, 255]
    obj = _m(c)[1]
    assert all((obj[i] != obj[i + 1]) for i in range(256)) and len({t["kind"] for t in c["textures"]}) == 3
    for length, idx in lists().items():
        assert len(idx) == length and len(np.unique(idx)) == length and (length == 1 or ((idx < 0).any() and (idx >= 257).any()))
    for c in CASES:
        assert 60 <= len(c["hits"]) <= 300, (c["name"], len(c["hits"]))


# ---- the frame of the integrator tests: a checkered ground, one image sphere, one tinted Dielectric, one lamp -------------------------

def frame_scene():
    """(recs, textures, binding, emission, lights): 12 spheres.  Object 0 is the ground (a WORLD checker), 1 the image sphere
    (BILINEAR, 8 x 8), 2 the tinted glass (a CONSTANT on a Dielectric), 3 the lamp, 4 a fuzzy Metal with a NORMAL checker, 5 a
    mirror with a NEAREST image; the other six are small untextured spheres of the three materials."""
    recs = [sphere((0, -1000, 0), 1000.0, 0, (0.5, 0.5, 0.5)), sphere((0, 1, 0), 1.0, 0, (0.6, 0.6, 0.6)), sphere((-2.2, 1, 0.4), 1.0, 2, ri=1.5),
            sphere((0.5, 4.5, 1.0), 0.8, 0, (0.0, 0.0, 0.0)), sphere((2.3, 1, -0.3), 1.0, 1, (0.8, 0.7, 0.6), 0.25),
            sphere((0.8, 0.4, 2.4), 0.4, 1, (0.9, 0.9, 0.9), 0.0)]
    small = [((-1.0, 0.3, 2.2), 0, (0.7, 0.2, 0.2)), ((2.0, 0.3, 1.8), 0, (0.2, 0.7, 0.3)), ((-3.0, 0.3, 2.0), 1, (0.6, 0.6, 0.9)),
             ((3.4, 0.3, 1.0), 2, (0, 0, 0)), ((-0.2, 0.25, 3.0), 0, (0.3, 0.3, 0.8)), ((1.5, 0.25, 3.2), 1, (0.8, 0.8, 0.3))]
    for k, (c, mat, alb) in enumerate(small):
        recs.append(sphere(c, c[1], mat, alb, 0.1 * (k % 2)))
    img = 0.2 + 0.6 * (ramp(8, 0.0) % 1.0)
    textures = [R.checker((0.9, 0.9, 0.9), (0.15, 0.2, 0.15), (1.0, 1.0, 1.0), R.WORLD), R.image(img, R.BILINEAR), R.constant((0.9, 0.6, 0.6)),
                R.checker((0.9, 0.8, 0.2), (0.2, 0.3, 0.9), 3.0, R.NORMAL), R.image(img[::-1].copy(), R.NEAREST)]
    binding = [0, 1, 2, -1, 3, 4] + [-1] * 6
    emission = np.zeros((12, 3))
    emission[3] = (12.0, 11.0, 9.0)
    return np.asarray(recs), textures, np.asarray(binding, dtype=np.int32), emission, [3]
