"""Shared inputs of the BSDF query tests (test_bsdf_query.py on the CPU, test_gpu_bsdf_query.py on the GPU): one scene as flat
(n, 16) records {kind, c0 xyz, c1 xyz, t0, t1, radius, material, albedo xyz, fuzz, ri} with every material case of
include/tor_bsdf.h, 300 items (incoming ray, hit record, outgoing ray) drawn from fixed seeds -- four full waves and a partial one
--, the named items that take each branch of the header, and the items whose outgoing ray is the restated scatter's own
(bounce_restatement.scatter over the oracle's generator) for the same incoming ray and record."""
import numpy as np

LAMB, METAL, GLASS = 0.0, 1.0, 2.0
N_RANDOM = 4 * 64 + 44
# the objects, by what they are there for
FLOOR, GLASS_BALL, MIRROR, DENORMAL, F1E100, F1E8, F005, F03, F09, F1, FNEG, F15, MOVER, RED = range(14)
FUZZ = {MIRROR: 0.0, DENORMAL: 5e-324, F1E100: 1e-100, F1E8: 1e-8, F005: 0.05, F03: 0.3, F09: 0.9, F1: 1.0, FNEG: -0.3, F15: 1.5,
        MOVER: 0.2}
# the lobes float64 resolves (tor_bsdf.h: below about 1e-16 the rounding of w x r is wider than the lobe): the round trip holds here
RESOLVED = (F1E8, F005, F03, F09, F1, FNEG, F15, MOVER)


def _sphere(c, r, mat=LAMB, albedo=(0.5, 0.5, 0.5), fuzz=0.0, ri=1.5):
    return [0.0, c[0], c[1], c[2], 0.0, 0.0, 0.0, 0.0, 0.0, r, mat, albedo[0], albedo[1], albedo[2], fuzz, ri]


def scene():
    """(14, 16) records.  -0.3 and 1.5 are fuzz values Scene.from_records carries although the reference's constructor clamps."""
    recs = [_sphere((0.0, -100.5, -1.0), 100.0, LAMB, (0.5, 0.6, 0.7)), _sphere((0.0, 0.0, -1.0), 0.5, GLASS)]
    for k in range(MIRROR, F15 + 1):
        recs.append(_sphere((float(k) - 6.0, 0.0, -2.0), 0.4, METAL, (0.8, 0.6 + 0.01 * k, 0.2), FUZZ[k]))
    recs.append([1.0, 2.0, 1.0, 0.0, 2.0, 1.5, 0.0, 0.0, 1.0, 0.3, METAL, 0.7, 0.7, 0.9, FUZZ[MOVER], 1.5])
    recs.append(_sphere((-2.0, 1.0, 0.0), 0.3, LAMB, (0.9, 0.1, 0.0)))
    recs = np.array(recs)
    assert recs.shape == (14, 16)
    return recs


def _unit(v):
    return v / np.sqrt((v * v).sum(axis=-1))[..., None]


def _reflect(d_in, nrm):
    """reflect(unit(d_in), nrm) with the header's operations (one item)."""
    ud = d_in * (1.0 / np.sqrt(d_in[0] * d_in[0] + d_in[1] * d_in[1] + d_in[2] * d_in[2]))
    return ud - nrm * (2.0 * (ud[0] * nrm[0] + ud[1] * nrm[1] + ud[2] * nrm[2]))


def pack(objects, normals, d_in, d_out):
    """(rays_in (n, 7), raw (n, 8), rays_out (n, 7)) of items given by object, normal and the two directions; the words the query
    does not read hold sentinels (origins, p, t, times: 7.0; front_face: 1)."""
    n = len(objects)
    rays_in, raw, rays_out = np.full((n, 7), 7.0), np.full((n, 8), 7.0), np.full((n, 7), 7.0)
    rays_in[:, 3:6], rays_out[:, 3:6], raw[:, 3:6] = d_in, d_out, normals
    words = raw.view(np.int32)
    words[:, 14], words[:, 15] = np.asarray(objects, dtype=np.int32), 1
    return rays_in, raw, rays_out


def random_items(recs, seed=0xB5DF):
    """N_RANDOM items: a random object, a random unit normal, an incoming direction of random length against the normal, and an
    outgoing one of random length -- for a Metal inside or just around its lobe (r + 1.2 f B), else anywhere, a quarter of them
    below the surface."""
    rs = np.random.RandomState(seed)
    n_obj = recs.shape[0]
    objects = rs.randint(n_obj, size=N_RANDOM)
    nrm = _unit(rs.normal(size=(N_RANDOM, 3)))
    d_in = _unit(rs.normal(size=(N_RANDOM, 3)))
    flip = (d_in * nrm).sum(axis=1) > 0
    d_in[flip] = -d_in[flip]
    d_in *= rs.uniform(0.1, 10.0, size=(N_RANDOM, 1))
    d_out = _unit(rs.normal(size=(N_RANDOM, 3)))
    up = rs.uniform(size=N_RANDOM) < 0.75
    below = (d_out * nrm).sum(axis=1) < 0
    d_out[up & below] = -d_out[up & below]
    ball = _unit(rs.normal(size=(N_RANDOM, 3))) * rs.uniform(size=(N_RANDOM, 1)) ** (1.0 / 3.0)
    for i in range(N_RANDOM):
        if recs[objects[i], 10] == METAL:
            d_out[i] = _reflect(d_in[i], nrm[i]) + ball[i] * (1.2 * abs(recs[objects[i], 14]))
    d_out *= rs.uniform(0.1, 10.0, size=(N_RANDOM, 1))
    return pack(objects, nrm, d_in, d_out)


def _rim(f, d_in, nrm):
    """Outgoing directions on the rim of the lobe of fuzz f: among the float64 neighbours of (f, 0, sqrt(1 - f f)) (normal
    incidence: r = +z) one whose s2 is the double just below f * f, one that gives exactly f * f, one just above -- or, where the
    neighbourhood holds none, the closest on that side.  Returns (the directions, their s2) by name."""
    r = _reflect(d_in, nrm)
    ff = f * f
    want = {"rim_inside": np.nextafter(ff, 0.0), "rim_exact": ff, "rim_outside": np.nextafter(ff, 1.0)}
    best = {}
    a0, c0 = f, np.sqrt(1.0 - ff)
    cand_a, cand_c = sorted(_steps(a0, 6)), sorted(_steps(c0, 6))
    cand_y = [0.0] + [float(np.sqrt(j * np.spacing(ff) / 4.0)) for j in range(1, 9)]   # (s2 grows by y * y: a fine adjustment)
    for a in cand_a:
        for c in cand_c:
            for y in cand_y:
                out = np.array([a, y, c])
                w = out * (1.0 / np.sqrt(out[0] * out[0] + out[1] * out[1] + out[2] * out[2]))
                x = np.array([w[1] * r[2] - w[2] * r[1], w[2] * r[0] - w[0] * r[2], w[0] * r[1] - w[1] * r[0]])
                s2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
                for name, target in want.items():
                    side_ok = (s2 < ff) if name == "rim_inside" else (s2 == ff) if name == "rim_exact" else (s2 > ff)
                    if side_ok and (name not in best or abs(s2 - target) < abs(best[name][0] - target)):
                        best[name] = (s2, out)
    return {name: best[name][1] for name in want if name in best}, {name: best[name][0] for name in want if name in best}


def _steps(x, k):
    """x and its k float64 neighbours on either side."""
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def named_items(recs):
    """(names, rays_in, raw, rays_out): the items that take each branch of include/tor_bsdf.h."""
    z = np.array([0.0, 0.0, 1.0])
    slant, down = np.array([0.6, 0.0, -0.8]), np.array([0.0, 0.0, -1.0])
    up = np.array([0.3, 0.2, 0.9])
    nan, inf = float("nan"), float("inf")
    rim, _ = _rim(0.3, down, z)
    items = [
        ("reflect", F03, z, slant, _reflect(slant, z)),                   # out exactly reflect(ud, n): the lobe's axis
        ("reflect_scaled", F005, z, slant * 3.0, _reflect(slant * 3.0, z) * 0.25),
        ("below_metal", F03, z, slant, np.array([0.6, 0.0, -0.8])),       # below the surface
        ("below_lambertian", FLOOR, z, slant, np.array([0.1, 0.2, -0.7])),
        ("tangent_zero", FLOOR, z, slant, np.array([1.0, 0.0, 0.0])),     # out . n == +0.0
        ("tangent_minus_zero", FLOOR, z, slant, np.array([-1.0, -1.0, -0.0])),   # out . n == -0.0
        ("tangent_metal", F09, z, slant, np.array([1.0, 0.0, 0.0])),
        ("tiny", F03, z, slant, _reflect(slant, z) * 1e-160),             # oo is denormal: > 0, w from a coarse sqrt
        ("tiny_lambertian", RED, z, slant, up * 1e-160),
        ("underflow", F03, z, slant, _reflect(slant, z) * 1e-170),        # oo underflows to 0
        ("overflow", F03, z, slant, _reflect(slant, z) * 1e160),          # oo overflows to +inf
        ("overflow_lambertian", FLOOR, z, slant, up * 1e160),
        ("zero_out", F03, z, slant, np.zeros(3)),
        ("nan_out", F03, z, slant, np.array([nan, 0.0, 1.0])),
        ("nan_out_lambertian", FLOOR, z, slant, np.array([0.0, nan, 1.0])),
        ("inf_out", F03, z, slant, np.array([inf, 0.0, 1.0])),
        ("inf_out_lambertian", FLOOR, z, slant, np.array([0.0, 1.0, inf])),
        ("nan_in", F03, z, np.array([nan, 0.0, -1.0]), _reflect(slant, z)),
        ("zero_in", F03, z, np.zeros(3), _reflect(slant, z)),
        ("grazing", F03, z, np.array([1.0, 0.0, -1e-9]), np.array([1.0, 0.05, 0.02])),
        ("grazing_wide", F09, z, np.array([1.0, 0.0, -1e-9]), np.array([0.5, 0.1, 0.4])),
        ("normal_incidence", F03, z, down, np.array([0.0, 0.0, 2.5])),
        ("normal_incidence_off", F03, z, down, np.array([0.1, -0.1, 1.0])),
        ("nonunit_normal", F09, z * 2.0, slant, np.array([-0.5, 0.1, 0.4])),     # r = ud - 4 (ud . z) z: not a unit vector
        ("nonunit_normal_lambertian", FLOOR, z * 2.0, slant, up),
        ("zero_normal", F03, np.zeros(3), slant, slant),                  # r = ud, but the gate sees out . 0
        ("zero_normal_lambertian", FLOOR, np.zeros(3), slant, up),
        ("nan_normal", F03, np.array([0.0, nan, 1.0]), slant, _reflect(slant, z)),
        ("object_minus_one", -1, z, slant, up),
        ("object_past_the_end", recs.shape[0], z, slant, up),
        ("object_int_min", -2 ** 31, z, slant, up),
        ("glass", GLASS_BALL, z, slant, _reflect(slant, z)),
        ("mirror", MIRROR, z, slant, _reflect(slant, z)),
        ("denormal_fuzz", DENORMAL, z, slant, _reflect(slant, z)),        # f * f == 0: DENSITY, and 0 everywhere
        ("fuzz_1e-100", F1E100, z, slant, _reflect(slant, z)),            # narrower than the rounding of w x r
        ("fuzz_1e-100_axis", F1E100, z, down, np.array([0.0, 0.0, 1.0])),  # w == r exactly, s2 == 0, f3 = 1e-300: about 4.8e199
        ("fuzz_1e-8", F1E8, z, slant, _reflect(slant, z)),
        ("negative_fuzz", FNEG, z, slant, _reflect(slant, z) + np.array([0.05, 0.1, -0.02])),
        ("holds_origin", F15, z, slant, np.array([-0.9, 0.1, 0.2])),      # the ball holds the origin: lo < 0 < hi
        ("holds_origin_axis", F15, z, slant, _reflect(slant, z)),
        ("touches_origin", F1, z, slant, np.array([-0.6, 0.0, 0.8])),     # f == |r|: the ball touches the origin, lo rounds about 0
        ("lo_zero", F1, z, down, np.array([20.0, 0.0, 21.0])),           # b - q == 0 exactly: the second closed form, whose bits differ
        ("gate_underflows", FLOOR, z * 1e-165, slant, up * 1e-160),       # out . n underflows to 0 although unit(out) . n > 0
        ("mover", MOVER, z, slant, _reflect(slant, z) + np.array([0.0, 0.1, 0.0])),
        ("red", RED, _unit(np.array([1.0, 2.0, 2.0])), slant, np.array([0.5, 1.0, 0.1])),
    ]
    for name in sorted(rim):                                              # the lobe's rim at normal incidence, fuzz 0.3
        items.append((name, F03, z, down, rim[name]))
    names = [it[0] for it in items]
    objects = [it[1] for it in items]
    rays_in, raw, rays_out = pack(objects, np.array([it[2] for it in items]), np.array([it[3] for it in items]),
                                  np.array([it[4] for it in items]))
    return names, rays_in, raw, rays_out


N_TRIP = 8 * 20


def scattered_items(oracle, recs, seed=0x7219):
    """N_TRIP items whose outgoing ray is bounce_restatement.scatter's for the same incoming ray and record, twenty per object of
    RESOLVED: (rays_in, raw, rays_out, status).  Normals are unit vectors, incidences from normal to grazing."""
    import bounce_restatement as BR
    import light_inputs as LI
    rs = np.random.RandomState(seed)
    objects = np.repeat(np.array(RESOLVED), N_TRIP // len(RESOLVED))
    nrm = _unit(rs.normal(size=(N_TRIP, 3)))
    d_in = _unit(rs.normal(size=(N_TRIP, 3)))
    flip = (d_in * nrm).sum(axis=1) > 0
    d_in[flip] = -d_in[flip]
    graze = np.arange(N_TRIP) % 4 == 3                                    # a quarter at grazing incidence: the absorbed ones
    tang = _unit(d_in - nrm * (d_in * nrm).sum(axis=1)[:, None])
    d_in[graze] = tang[graze] - nrm[graze] * 0.05
    d_in *= rs.uniform(0.5, 2.0, size=(N_TRIP, 1))
    rays_in, raw, _ = pack(objects, nrm, d_in, d_in)
    res = BR.scatter(oracle, recs, rays_in, raw, LI.states(N_TRIP, 0xB5DF))
    return rays_in, raw, res["rays"], res["status"]


# ---- the frame of the trace_direct(glossy=...) tests: a glossy floor that mirrors one small lamp ------------------------------------
G_FLOOR, G_BALL, G_LAMP = 0, 1, 2


def glossy_scene(enclosed=True):
    """(recs, emission): a floor sphere of Metal with fuzz 0.3, one Lambertian ball standing on it, one small black-body lamp above
    and behind the camera (no camera ray sees the lamp itself, whose partial coverage of a pixel would add the same noise to
    every estimator).  enclosed: the floor is the INSIDE of a sphere of radius 6 that holds the camera, the ball and the lamp, so no path
    reaches the sky -- Context.trace ends a path that misses with sky * att alone, the emission it had gathered included, so
    only an enclosed scene compares estimators of the lamp's light; otherwise a sphere of radius 100 below them, under the open
    sky.  What the camera sees of the lamp on the floor is a glossy reflection: with the floor booked specular a path finds it
    only by scattering into the lamp by chance."""
    floor = _sphere((0.0, 5.5, 0.0), 6.0, METAL, (0.8, 0.8, 0.7), 0.3) if enclosed else \
        _sphere((0.0, -100.5, 0.0), 100.0, METAL, (0.8, 0.8, 0.7), 0.3)
    recs = np.array([floor, _sphere((0.0, 0.0, 0.0), 0.5, LAMB, (0.7, 0.5, 0.3)), _sphere((1.0, 2.2, 4.2), 0.2, LAMB, (0.0, 0.0, 0.0))])
    emission = np.zeros((3, 3))
    emission[G_LAMP] = (60.0, 50.0, 40.0)
    return recs, emission


def glossy_camera(tor):
    return tor.camera(look_from=(0.0, 1.2, 3.5), look_at=(0.0, 0.0, 0.0), vertical_field_of_view=50.0, aspect_ratio=1.0,
                      aperture=0.0, focus_distance=1.0, shutter_open=0.0, shutter_close=0.0)


_all = {}


def all_items(oracle):
    """Every item -- random, named, scattered -- as (rays_in, raw, rays_out), the names of the named ones and where they start;
    built once."""
    if not _all:
        recs = scene()
        a = random_items(recs)
        names, *b = named_items(recs)
        c = scattered_items(oracle, recs)
        _all["items"] = tuple(np.concatenate([a[k], b[k], c[k]]) for k in range(3))
        _all["names"] = {name: N_RANDOM + k for k, name in enumerate(names)}
        _all["trip"] = (N_RANDOM + len(names), c[3])
        _all["recs"] = recs
    return _all
