"""Shared inputs of the light-tracing tests (test_camera_query.py on the CPU, test_gpu_camera_query.py on the GPU): cameras as the
24 float64 of the oracle's camera() (Camera.as_array's layout), frames, 3 * 64 + 5 points per (camera, frame) -- three full waves
and a partial one -- among them the points that take each branch of include/tor_camera.h, generator states with crafted ones
among them, and the scenes of the trace_light tests.  The light tables are those of light_inputs.py, plus one made of ties."""
import numpy as np

import light_inputs as LI

N_POINTS = LI.N_POINTS
FRAMES = ((2, 2), (5, 7), (48, 64))
CAMERAS = {
    "pinhole": dict(look_from=(0.0, 0.0, 4.5), look_at=(0.0, 0.0, 0.0), vfov=70.0, aspect=1.0, aperture=0.0, focus_dist=1.0),
    "lens": dict(look_from=(3.0, 2.0, 3.0), look_at=(0.0, 0.5, 0.0), vfov=40.0, aspect=1.0, aperture=0.5, focus_dist=3.0),
    "tilted": dict(look_from=(-2.0, 1.0, 5.0), look_at=(0.5, 0.0, 0.0), vup=(0.3, 1.0, 0.2), vfov=55.0, aspect=1.0, aperture=0.5,
                   focus_dist=3.0),
    "wide": dict(look_from=(13.0, 2.0, 3.0), look_at=(0.0, 0.0, 0.0), vfov=20.0, aspect=2.5, aperture=0.1, focus_dist=10.0),
}
TABLES = LI.TABLES + ("ties",)
TIME_RANGES = ((0.0, 0.0), (0.25, 1.5))


def camera(oracle, name):
    """The 24 float64 of the named camera: origin, lower_left_corner, horizontal, vertical, u, v, w, lens_radius, shutter."""
    return oracle.camera(shutter_open=0.0, shutter_close=0.0, **CAMERAS[name])


def camera_struct(tor, cam24):
    """The package's Camera of 24 float64."""
    return tor.Camera.from_buffer_copy(np.ascontiguousarray(cam24, dtype=np.float64).tobytes())


def parts(cam24):
    cam = np.asarray(cam24, dtype=np.float64)
    return tuple(cam[3 * k:3 * k + 3] for k in range(7))


SPECIAL = {"focus": -16, "border_s": -15, "border_t": -14, "left": -13, "right": -12, "below": -11, "above": -10, "lens_plane": -9,
           "behind": -8, "lens_point": -7, "far": -6, "overflow": -5, "overflow_z": -4, "nan": -3, "inf": -2, "centre": -1}


def points(cam24, nrows, ncols, seed=3):
    """(N_POINTS, 4) float64 {x, y, z, time}: random points in and around the frustum, then the special ones (SPECIAL names their
    rows, counted from the end)."""
    origin, llc, H, V, u, v, w = parts(cam24)
    rs = np.random.RandomState(seed + 1000 * nrows + ncols)
    s = rs.uniform(-0.3, 1.5, size=N_POINTS)
    t = rs.uniform(-0.3, 1.5, size=N_POINTS)
    lam = np.exp(rs.uniform(np.log(0.05), np.log(8.0), size=N_POINTS))
    F = llc[None, :] + s[:, None] * H[None, :] + t[:, None] * V[None, :]
    pts = np.empty((N_POINTS, 4))
    pts[:, 0:3] = origin[None, :] + (F - origin[None, :]) * lam[:, None]
    pts[:, 3] = rs.uniform(0.0, 1.0, size=N_POINTS)
    on = lambda a, b: llc + a * H + b * V                                  # a point of the focus plane
    sc, sr = 1.0 / float(ncols - 1), 1.0 / float(nrows - 1)
    special = [
        on(0.4, 0.6),                                                     # on the focus plane
        on(1.0 * sc, 0.3 * sr),                                           # on a pixel border: s * (ncols - 1) an integer
        on(0.3 * sc, 1.0 * sr),                                           # t * (nrows - 1) an integer
        on(-1e-9, 0.5), on(ncols * sc + 1e-9, 0.5),                       # just outside the left and right edges
        on(0.5, -1e-9), on(0.5, nrows * sr + 1e-9),                       # just below and above the frame
        origin + 0.7 * u + 0.2 * v,                                       # on the lens plane: z == 0
        origin + 2.0 * w,                                                 # behind it
        origin,                                                           # the lens point itself (of a pinhole)
        origin - 1e6 * w + 1e5 * u,                                       # 1e6 units away
        np.array([1e200, 0.0, 0.0]),                                      # beyond overflow: e . e is infinite
        origin - 1e120 * w,                                               # z * z * z overflows alone
        np.array([np.nan, 0.0, 1.0]),                                     # a NaN coordinate
        np.array([0.0, np.inf, 0.0]),                                     # an infinite one
        origin + (on(0.5 * ncols * sc, 0.5 * nrows * sr) - origin) * 2.5,  # the middle of the frame, beyond the focus plane
    ]
    assert len(special) == len(SPECIAL)
    for k, p in enumerate(special):
        pts[N_POINTS - len(special) + k, 0:3] = p
    return pts


HALF, LARGEST = (1 << 63, 0, 0x9E3779B97F4A7C15, 0), ((1 << 64) - 1, 0, 0x9E3779B97F4A7C15, 0)


def states(n, seed=0xCA3E7A):
    """(n, 4) uint64 xoshiro256+ states; the last two are crafted: with s1 = s3 = 0 the first TWO outputs are s0, so HALF draws
    0.5 twice and LARGEST the largest uniform01, 1 - 2^-52, twice -- the first and the second draw of either query (the lens
    radius; the emission's time and its pick: a pick of exactly half the total, a running-sum tie in table `ties`)."""
    st = LI.states(n, seed)
    st[n - 2] = np.array(HALF, dtype=np.uint64)
    st[n - 1] = np.array(LARGEST, dtype=np.uint64)
    return st


def table(name, oracle=None):
    """light_inputs.table, and `ties`: weights (1, 0, 1, 0, 2, 0) -- running sums 1, 1, 2, 2, 4, 4, so a draw of 0.5 is x == 2
    exactly, equal to two running sums, and the largest draw meets a last light of weight 0."""
    if name != "ties":
        return LI.table(name, oracle)
    recs = [LI._sphere((0.0, -100.5, -1.0), 100.0)]
    for k in range(6):
        c = (float(k) - 2.5, 1.0, 0.5 * float(k))
        recs.append(LI._mover(c, (c[0], c[1] + 1.0, c[2]), 0.0, 2.0, 0.3) if k == 4 else LI._sphere(c, 0.1 * float(k)))   # (k == 0: radius 0)
    return np.array(recs), np.array([1, 2, 3, 4, 5, 6], dtype=np.int32), np.array([1.0, 0.0, 1.0, 0.0, 2.0, 0.0])


# ---- the frames of the trace_light tests ---------------------------------------------------------------------------------------------
def diffuse_scene():
    """light_inputs.lamp_scene with the metal ball moved behind the camera (its z stays above the camera's 4.5, inside the shell):
    the camera at (0, 0, 4.5) looking down -z sees diffuse surfaces only, so a light tracer and a path tracer estimate the same
    frame.  (recs, emission, lamp)."""
    recs, emission, lamp = LI.lamp_scene()
    recs[3, 1:4] = (1.0, -0.8, 5.2)
    return recs, emission, lamp


def caustic_scene():
    """diffuse_scene with a glass ball two units from the lamp on the way to the visible floor: part of the lamp's light reaches
    that floor through the glass -- a caustic, which shadow rays cannot find (the glass blocks them).  The ball itself is in
    view at the top of the frame, and a light tracer cannot see what lies behind glass, so on this frame the two estimators'
    means differ; it serves the variance record of tools/light_trace_rate.py, not a test.  (recs, emission, lamp)."""
    recs, emission, lamp = diffuse_scene()
    recs = np.vstack([recs, np.array([LI._sphere((0.0, 0.83, 3.38), 0.4, LI.GLASS, (1.0, 1.0, 1.0))])])
    return recs, np.vstack([emission, np.zeros((1, 3))]), lamp


def frame_camera(tor):
    """The camera of the trace_light frames (test_gpu_light_query's)."""
    return tor.camera(look_from=(0.0, 0.0, 4.5), look_at=(0.0, 0.0, 0.0), vertical_field_of_view=70.0, aspect_ratio=1.0,
                      aperture=0.0, focus_distance=1.0, shutter_open=0.0, shutter_close=0.0)
