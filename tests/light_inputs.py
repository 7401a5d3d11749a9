"""Shared inputs of the direct-light sampling tests (test_light_query.py on the CPU, test_gpu_light_query.py on the GPU): scenes as
flat (n, 16) records {kind, c0 xyz, c1 xyz, t0, t1, radius, material, albedo xyz, fuzz, ri}, light tables (objects, weights) and
3 * 64 + 5 points per table -- three full waves and a partial one -- among them the points that take each branch of
include/tor_lights.h: inside a light, exactly at its centre (d2 == 0), exactly on its surface (d2 == R * R), 1e6 units away (s2
near the underflow of 1 - s2), so far away that every importance by solid angle is 0, times outside a mover's interval, and a NaN
coordinate."""
import numpy as np

N_POINTS = 3 * 64 + 5
TABLES = ("one", "three", "many65", "random20")
LAMB, METAL, GLASS = 0.0, 1.0, 2.0


def _sphere(c, r, mat=LAMB, albedo=(0.5, 0.5, 0.5), fuzz=0.0, ri=1.5):
    return [0.0, c[0], c[1], c[2], 0.0, 0.0, 0.0, 0.0, 0.0, r, mat, albedo[0], albedo[1], albedo[2], fuzz, ri]


def _mover(c0, c1, t0, t1, r, mat=LAMB, albedo=(0.5, 0.5, 0.5)):
    return [1.0, c0[0], c0[1], c0[2], c1[0], c1[1], c1[2], t0, t1, r, mat, albedo[0], albedo[1], albedo[2], 0.0, 1.5]


def table(name, oracle=None):
    """(recs (n, 16), lights (L,) int32 object indices, weights (L,) float64 or None)."""
    if name == "one":
        recs = [_sphere((0.0, -100.5, -1.0), 100.0), _sphere((1.0, 2.0, 3.0), 0.5), _sphere((-1.0, 0.0, -1.0), 0.5, METAL)]
        return np.array(recs), np.array([1], dtype=np.int32), None
    if name == "three":                                                   # a mover, a negative radius, a weight 0; not in list order
        recs = [_sphere((0.0, -100.5, -1.0), 100.0), _sphere((1.0, 2.0, 3.0), -0.5, GLASS), _sphere((4.0, 1.0, 0.0), 0.75),
                _mover((-2.0, 1.0, 0.5), (-2.0, 1.5, 1.5), 0.25, 1.0, 0.5), _sphere((0.0, 0.0, -1.0), 0.5)]
        return np.array(recs), np.array([3, 1, 2], dtype=np.int32), np.array([2.0, 0.75, 0.0])
    if name == "many65":                                                  # past one wave's width
        rs = np.random.RandomState(65)
        recs = [_sphere((0.0, -100.5, -1.0), 100.0)]
        for k in range(70):
            c = (float(k % 10) - 4.5, 0.3 + 0.7 * float(k // 10), float(rs.uniform(-3, 3)))
            if k % 7 == 3:
                recs.append(_mover(c, (c[0], c[1] + 0.5, c[2]), 0.0, 1.0, 0.2))
            else:
                recs.append(_sphere(c, 0.05 + 0.25 * float(rs.uniform())))
        lights = np.array([1 + k for k in range(70) if k % 14 != 5], dtype=np.int32)
        assert lights.size == 65
        return np.array(recs), lights, rs.uniform(0.1, 3.0, size=65)
    if name == "random20":                                                # 20 of random_scene's objects, movers among them
        recs, _ = oracle.random_scene(0xFACADE)
        lights = np.arange(3, 3 + 20 * 24, 24, dtype=np.int32)
        assert (recs[lights, 0] == 1).any() and (recs[lights, 0] == 0).any()
        return recs, lights, np.abs(recs[lights, 9]) ** 2 * 10.0
    raise KeyError(name)


def points(recs, lights, seed=1):
    """(N_POINTS, 4) float64 {x, y, z, time}: random points about the lights, then the special ones (SPECIAL names their rows,
    counted from the end)."""
    rs = np.random.RandomState(seed)
    recs = np.asarray(recs, dtype=np.float64)
    first = recs[int(lights[0])]
    c = first[1:4].copy()
    R = abs(first[9])
    pts = np.empty((N_POINTS, 4))
    centres = recs[np.asarray(lights, dtype=np.int64), 1:4]
    pts[:, 0:3] = centres[rs.randint(len(lights), size=N_POINTS)] + rs.normal(scale=2.0, size=(N_POINTS, 3))
    pts[:, 3] = rs.uniform(0.0, 1.0, size=N_POINTS)
    static = first[0] == 0
    t_first = 0.0 if static else first[7]                                 # a mover sits at c0 at time0 (its fraction is 0 there)
    special = [
        (c + np.array([0.25 * R, 0.1 * R, 0.0]), t_first),                # inside the first light
        (c, t_first),                                                     # exactly at its centre: d2 == 0
        (c + np.array([R, 0.0, 0.0]), t_first),                           # on its surface; exactly (d2 == R * R) in `one` and `three`
        (c + np.array([1e6, 0.0, 0.0]), 0.5),                             # s2 ~ 1e-13
        (np.array([1e200, 0.0, 0.0]), 0.5),                               # d2 overflows: every m is 0
        (c + np.array([0.0, 3.0, 0.0]), -3.0),                            # times outside a mover's interval
        (c + np.array([0.0, 3.0, 0.0]), 7.0),
        (np.array([np.nan, 0.0, 1.0]), 0.5),                              # a NaN coordinate
    ]
    for k, (p, t) in enumerate(special):
        pts[N_POINTS - len(special) + k] = [p[0], p[1], p[2], t]
    return pts


SPECIAL = {"inside": -8, "centre": -7, "surface": -6, "far": -5, "overflow": -4, "early": -3, "late": -2, "nan": -1}


def states(n, seed=0x51A7E):
    """(n, 4) uint64 xoshiro256+ states, none of them zero."""
    rs = np.random.RandomState(seed & 0x7FFFFFFF)
    w = rs.randint(0, 1 << 32, size=(n, 4, 2), dtype=np.int64).astype(np.uint64)
    return (w[:, :, 0] << np.uint64(32)) | w[:, :, 1] | np.uint64(1)      # all 64 bits random (the first output is s0 + s3)


# ---- the frame of the trace_direct tests: an enclosed scene (no ray reaches the sky) with one small lamp -----------------------------
# The lamp's smallness decides which estimator is noisier.  From a wall point at distance d the lamp (radius 0.25) subtends the
# fraction (0.25 / d)^2 / 2 of the hemisphere, about 0.1 % at d ~ 5: a path that must HIT the lamp by chance sees it in about one
# bounce in a thousand and then adds about a thousand times the mean, so its per-sample variance is of the order of 1000 times the
# squared mean; the light sample reaches the lamp from every diffuse vertex the lamp is visible from, so its per-sample variance is
# of the order of the squared mean.  A lamp a few times larger would still separate the two by an order of magnitude.
LAMP = 1


def lamp_scene():
    """(recs, emission (n, 3), lamp object index): a hollow diffuse shell of radius 6 about the origin, a black-body lamp of radius
    0.25 above and behind the camera of the test (at (0, 0, 4.5), looking down -z: no camera ray sees the lamp itself, whose
    partial coverage of a pixel would add the same noise to every estimator), a diffuse ball and a small metal ball."""
    recs = np.array([_sphere((0.0, 0.0, 0.0), 6.0, LAMB, (0.6, 0.6, 0.6)), _sphere((0.0, 2.0, 5.0), 0.25, LAMB, (0.0, 0.0, 0.0)),
                     _sphere((-0.8, -1.0, 0.0), 1.0, LAMB, (0.7, 0.5, 0.3)), _sphere((1.6, -0.8, 0.3), 0.5, METAL, (0.8, 0.8, 0.8))])
    emission = np.zeros((4, 3))
    emission[LAMP] = (60.0, 50.0, 40.0)
    return recs, emission, LAMP
