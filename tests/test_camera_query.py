"""The light-tracing queries without a GPU: the entries exist and refuse what include/tor_camera.h says they refuse, and the numpy
restatement of the header's text (tests/camera_restatement.py), which the GPU suite holds the kernels to bit for bit, is what a
light tracer needs -- a connection that inverts the camera's rays, a factor that is the density the header derives, an emission
that is uniform over the lamps and cosine-weighted about the normal, fixed draw counts, and the pick the header words.  Each check
also shows that the shared inputs (tests/camera_inputs.py) mean something."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import camera_inputs as I
import camera_restatement as CR
import light_inputs as LI
import nearest_restatement as N
import radiance_restatement as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
_big = {}


def _advance(oracle, st, k):
    """The states after k uniform01 draws each."""
    L = oracle.lib()
    st = np.ascontiguousarray(st, dtype=np.uint64).copy()
    for i in range(st.shape[0]):
        for _ in range(k):
            L.oracle_rng_uniform01(RR._ptr(st, i))
    return st


def _pinhole(oracle, name):
    kw = dict(I.CAMERAS[name], aperture=0.0)
    return oracle.camera(shutter_open=0.0, shutter_close=0.0, **kw)


def _emission(oracle, name, n=20000, tr=(0.0, 0.0)):
    """n emitted paths of a table: computed once, never changed."""
    key = (name, n, tr)
    if key not in _big:
        recs, lights, weights = I.table(name, oracle)
        _big[key] = (recs, lights, weights, CR.emit(oracle, recs, lights, weights, LI.states(n, 0xE717), tr[0], tr[1]))
    return _big[key]


def test_the_entries_are_declared_bound_and_exported(tor):
    src = open(os.path.join(ROOT, "include", "tor_camera.h")).read()
    assert '#include "tor_camera.h"' in open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in tor.CAMERA_SYMBOLS:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_camera.h"
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
    assert sorted(tor.CAMERA_SYMBOLS) == sorted(set(re.findall(r"TOR_API\s+int\s+(tor_\w+)\s*\(", src)))
    for method in ("connect_camera", "emit_lights", "trace_light"):
        assert callable(getattr(tor.Context, method))
    assert callable(tor.Film.add_light_pass)
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert mk.count("tor_camera.hip") == 2 and mk.count("tor_camera.h ") == 1      # SRCS and ASM_SRCS; HDRS


def test_refusals_that_need_no_device(tor, oracle):
    """The checks that come before any device work, in the header's order; nothing is touched.  (None of them reads the
    context, so a non-NULL pointer stands in for one.)"""
    L = tor.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.cast((C.c_char * 64)(), C.c_void_p)
    cam = I.camera_struct(tor, I.camera(oracle, "lens"))
    err = lambda: L.tor_last_error().decode()
    connect = L.tor_camera_connect_device
    assert connect(None, C.byref(cam), 4, 4, 1, p, p, None, 1, p, p, p, None, None) == -1 and "tor_camera_connect_device" in err()
    assert connect(ctx, None, 4, 4, 1, p, p, None, 1, p, p, p, None, None) == -1 and "NULL" in err()
    assert L.tor_camera_connect_host(None, C.byref(cam), 4, 4, 1, p, p, None, 1, p, p, p, None) == -1 and "tor_camera_connect_host" in err()
    assert connect(ctx, C.byref(cam), 1, 4, -1, p, p, None, 1, p, p, p, None, None) == -1 and ">= 2" in err()      # rows before counts
    assert connect(ctx, C.byref(cam), 4, 1, 1, p, p, None, 1, p, p, p, None, None) == -1 and ">= 2" in err()
    assert connect(ctx, C.byref(cam), 4, 4, -1, p, p, None, 1, p, p, p, None, None) == -1 and "< 0" in err()
    assert connect(ctx, C.byref(cam), 4, 4, 1, p, p, None, -1, p, p, p, None, None) == -1 and "n_list < 0" in err()
    assert connect(ctx, C.byref(cam), 4, 4, 2, p, p, None, 1, p, p, p, None, None) == -1 and "without a list" in err()
    for field, value in (("lens_radius", -0.5), ("lens_radius", float("nan")), ("lens_radius", float("inf"))):
        bad = I.camera_struct(tor, I.camera(oracle, "lens"))
        setattr(bad, field, value)
        assert connect(ctx, C.byref(bad), 4, 4, 1, None, p, None, 1, p, p, p, None, None) == -1 and "lens_radius" in err()   # before the NULLs
    for vec in ("horizontal", "vertical", "w"):                            # H . H, V . V, fd not > 0
        bad = I.camera_struct(tor, I.camera(oracle, "lens"))
        v = getattr(bad, vec)
        v.x = v.y = v.z = 0.0
        assert connect(ctx, C.byref(bad), 4, 4, 1, p, p, None, 1, p, p, p, None, None) == -1 and "focus distance" in err()
    bad = I.camera_struct(tor, I.camera(oracle, "lens"))
    bad.horizontal.x = float("inf")
    assert connect(ctx, C.byref(bad), 4, 4, 1, p, p, None, 1, p, p, p, None, None) == -1
    for hole in range(5):                                                  # NULL points, rng, rays, pixel or factor with work to do
        a = [p] * 5
        a[hole] = None
        assert connect(ctx, C.byref(cam), 4, 4, 1, a[0], a[1], None, 1, a[2], a[3], a[4], None, None) == -1 and "NULL" in err()
    assert connect(ctx, C.byref(cam), 4, 4, 0, None, None, None, 0, None, None, None, None, None) == 0     # nothing to do
    emit = L.tor_light_emit_device
    assert emit(None, 1, p, None, 1, 0.0, 0.0, p, p, p, p, None) == -1 and "tor_light_emit_device" in err()
    assert L.tor_light_emit_host(None, 1, p, None, 1, 0.0, 0.0, p, p, p, p) == -1 and "tor_light_emit_host" in err()
    assert emit(ctx, -1, p, None, 1, 0.0, 0.0, p, p, p, p, None) == -1
    assert emit(ctx, 2, p, None, 1, 0.0, 0.0, p, p, p, p, None) == -1 and "without a list" in err()
    for lo, hi in ((1.0, 0.5), (float("nan"), 1.0), (0.0, float("inf"))):
        assert emit(ctx, 1, None, None, 1, lo, hi, p, p, p, p, None) == -1 and "time range" in err()        # before the NULLs
    for hole in range(5):
        a = [p] * 5
        a[hole] = None
        assert emit(ctx, 1, a[0], None, 1, 0.0, 1.0, a[1], a[2], a[3], a[4], None) == -1 and "NULL" in err()
    assert all(v == 0.0 for v in buf)


@pytest.mark.parametrize("name", list(I.CAMERAS))
def test_the_inputs_take_every_branch(oracle, name):
    cam = I.camera(oracle, name)
    nrows, ncols = 5, 7
    pts = I.points(cam, nrows, ncols)
    st = I.states(len(pts))
    res = CR.connect(oracle, cam, nrows, ncols, pts, st)
    at = {k: len(pts) + v for k, v in I.SPECIAL.items()}
    pix = res["pixel"]
    rnd = pix[:len(pts) - len(I.SPECIAL)]
    assert (rnd >= 0).sum() > 30 and (rnd < 0).sum() > 30                 # in and around the frustum
    assert len(np.unique(rnd[rnd >= 0])) > 20
    for k in ("focus", "centre", "far"):
        assert pix[at[k]] >= 0 and res["factor"][at[k]] > 0, k
    for k in ("left", "right", "below", "above", "behind", "overflow", "overflow_z", "nan", "inf"):
        assert pix[at[k]] == -1 and res["factor"][at[k]] == 0 and (res["rays"][at[k]] == 0).all(), k
    if name == "pinhole":                                                 # axis-aligned: exactly on the lens plane, exactly the lens point
        assert pix[at["lens_plane"]] == -1 and pix[at["lens_point"]] == -1
        assert (res["lens"] == 0).all()
    else:
        assert (np.hypot(res["lens"][:, 0], res["lens"][:, 1]) <= cam[21] * (1 + 4 * EPS)).all() and (res["lens"] != 0).any()
    ok = pix >= 0
    assert (pix[ok] < nrows * ncols).all() and np.isfinite(res["factor"]).all() and np.isfinite(res["rays"]).all()
    # a connected ray starts at the point and ends, at parameter 1.0, on the lens
    c = CR.camera_constants(cam, nrows, ncols)
    end = res["rays"][ok, 0:3] + res["rays"][ok, 3:6] - c["origin"][None, :]
    assert (np.abs(end @ c["w"]) <= 1e-9 * (1 + np.abs(pts[ok, 0:3]).max(axis=1))).all()
    assert np.array_equal(res["rays"][ok, 0:3], pts[ok, 0:3]) and np.array_equal(res["rays"][ok, 6], pts[ok, 3])


@pytest.mark.parametrize("name", list(I.CAMERAS))
@pytest.mark.parametrize("frame", I.FRAMES)
def test_round_trip_pinhole(oracle, name, frame):
    """The connection inverts tor_camera_rays_device: a point on the camera ray of (row, col, U, U') connects to that pixel, for
    offsets in [2^-20, 1 - 2^-20] -- every one: no input is left out."""
    nrows, ncols = frame
    cam = _pinhole(oracle, name)
    origin, llc, H, V, u, v, w = I.parts(cam)
    rs = np.random.RandomState(7 + nrows)
    pix = np.arange(nrows * ncols) if nrows * ncols <= 64 else rs.choice(nrows * ncols, size=256, replace=False)
    pix = np.concatenate([pix, pix, pix])
    row, col = pix // ncols, pix % ncols
    lo, hi = 2.0 ** -20, 1.0 - 2.0 ** -20
    U, U2 = rs.uniform(lo, hi, size=pix.size), rs.uniform(lo, hi, size=pix.size)
    U[: pix.size // 3], U2[: pix.size // 3] = lo, hi                        # the ends of the range
    U[pix.size // 3: 2 * (pix.size // 3)], U2[pix.size // 3: 2 * (pix.size // 3)] = hi, lo
    s = (col.astype(np.float64) + U) / float(ncols - 1)
    t = (row.astype(np.float64) + U2) / float(nrows - 1)
    d = ((llc[None, :] + H[None, :] * s[:, None]) + V[None, :] * t[:, None]) - origin[None, :]          # cameras.nim:47-57, no lens
    c = CR.camera_constants(cam, nrows, ncols)
    for lam in (0.5, 1.0, 7.0):
        pts = np.zeros((pix.size, 4))
        pts[:, 0:3] = origin[None, :] + lam * d
        got = CR.connect_points(oracle.lib(), c, nrows, ncols, pts, rs.uniform(size=pix.size), rs.uniform(size=pix.size))
        assert np.array_equal(got["pixel"], pix.astype(np.int32)), (lam, int((got["pixel"] != pix).sum()))


@pytest.mark.parametrize("name", ("lens", "tilted", "wide"))
def test_a_point_of_the_focus_plane_lands_in_its_pixel_whatever_the_lens_draws(oracle, name):
    nrows, ncols = 5, 7
    cam = I.camera(oracle, name)
    origin, llc, H, V, u, v, w = I.parts(cam)
    rs = np.random.RandomState(11)
    pix = np.repeat(np.arange(nrows * ncols), 8)
    row, col = pix // ncols, pix % ncols
    s = (col + rs.uniform(0.05, 0.95, size=pix.size)) / float(ncols - 1)
    t = (row + rs.uniform(0.05, 0.95, size=pix.size)) / float(nrows - 1)
    pts = np.zeros((pix.size, 4))
    pts[:, 0:3] = llc[None, :] + s[:, None] * H[None, :] + t[:, None] * V[None, :]
    got = CR.connect_points(oracle.lib(), CR.camera_constants(cam, nrows, ncols), nrows, ncols, pts, rs.uniform(size=pix.size),
                            rs.uniform(size=pix.size))
    assert np.array_equal(got["pixel"], pix.astype(np.int32))
    assert len(np.unique(np.round(got["lens"], 6), axis=0)) > pix.size // 2                              # the lens points do vary


def _solid_angle(a, b, c):
    """Van Oosterom-Strackee: the solid angle of the triangles (a, b, c) seen from the origin, from the corners alone."""
    la, lb, lc = (np.linalg.norm(x, axis=1) for x in (a, b, c))
    num = np.abs(np.einsum("ij,ij->i", a, np.cross(b, c)))
    den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", a, c) * lb + np.einsum("ij,ij->i", b, c) * la
    return 2.0 * np.arctan2(num, den)


@pytest.mark.parametrize("lam", (0.5, 3.0))
def test_the_factor_is_a_density(oracle, lam):
    """Per pixel of the 5 x 7 frame the pinhole's factor * d^2 integrates to 1 over the solid angle of the pixel's footprint:
    the sum over a G x G tessellation of the footprint of factor(centre) * d^2 * Omega_cell, the solid angles from the cells'
    corners alone.  The tolerance is the quadrature's: in focus-plane coordinates (p, q) the measure is m = fd / (fd^2 + p^2 +
    q^2)^(3 / 2) dp dq and factor * d^2 is 1 / (m * the cell-count-normalised area), so the only error is the midpoint rule's on
    m over a cell, relatively at most (hp^2 * |m_pp| + hq^2 * |m_qq|) / (24 m) with |m_pp| / m <= 3 / fd^2 + 15 p^2 / (fd^2 +
    rho^2)^2 <= 6.75 / fd^2 (x / (a + x)^2 <= 1 / (4 a)), the same for q.  Points at lam times the footprint's distance: the
    factor falls as 1 / d^2."""
    nrows, ncols, G = 5, 7, 32
    cam = I.camera(oracle, "pinhole")
    origin, llc, H, V, u, v, w = I.parts(cam)
    c = CR.camera_constants(cam, nrows, ncols)
    hp, hq = np.linalg.norm(H) / (ncols - 1) / G, np.linalg.norm(V) / (nrows - 1) / G
    tol = (hp * hp + hq * hq) / 24.0 * 6.75 / c["fd"] ** 2 + 1e-12
    assert tol < 2e-4
    g = (np.arange(G + 1) / G)
    worst = 0.0
    for row in range(nrows):
        for col in range(ncols):
            s = (col + g) / (ncols - 1)
            t = (row + g) / (nrows - 1)
            S, T = np.meshgrid(s, t, indexing="xy")
            P = (llc[None, None, :] + S[:, :, None] * H[None, None, :] + T[:, :, None] * V[None, None, :]) - origin[None, None, :]
            p00, p10, p01, p11 = (P[:-1, :-1].reshape(-1, 3), P[:-1, 1:].reshape(-1, 3), P[1:, :-1].reshape(-1, 3), P[1:, 1:].reshape(-1, 3))
            omega = _solid_angle(p00, p10, p11) + _solid_angle(p00, p11, p01)
            sc, tc = (col + (g[:-1] + 0.5 / G)) / (ncols - 1), (row + (g[:-1] + 0.5 / G)) / (nrows - 1)
            Sc, Tc = np.meshgrid(sc, tc, indexing="xy")
            centre = (llc[None, :] + Sc.reshape(-1, 1) * H[None, :] + Tc.reshape(-1, 1) * V[None, :]) - origin[None, :]
            pts = np.zeros((G * G, 4))
            pts[:, 0:3] = origin[None, :] + lam * centre
            got = CR.connect_points(oracle.lib(), c, nrows, ncols, pts, np.full(G * G, 0.3), np.full(G * G, 0.6))
            assert (got["pixel"] == row * ncols + col).all()
            d2 = (lam * lam) * (centre * centre).sum(axis=1)
            total = float((got["factor"] * d2 * omega).sum())
            worst = max(worst, abs(total - 1.0))
    print(f"factor density: worst |sum - 1| = {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol


@pytest.mark.parametrize("name", ("pinhole", "lens"))
def test_a_lamp_seen_directly_has_its_radiance(oracle, name):
    """One lamp of radiance Le whose image covers the central pixel (2, 2) of a 5 x 5 frame: emitted points, connected, give the
    pixel (1 / N) sum Le * cos_y * factor / pdf_area = Le within 5 standard errors from 16 batches.  cos_y > 0 is the only
    visibility involved (a sphere is convex).  The thin lens has the lamp centred on the focus plane, with a radius above the
    pixel footprint's half diagonal, so every camera ray of the pixel from every lens point meets it."""
    nrows = ncols = 5
    Le, batches, per = 2.5, 16, 4096
    cam = I.camera(oracle, name)
    origin, llc, H, V, u, v, w = I.parts(cam)
    c = CR.camera_constants(cam, nrows, ncols)
    F = llc + 0.625 * H + 0.625 * V                                        # the middle of pixel (2, 2) on the focus plane
    half_diag = 0.5 * np.hypot(np.linalg.norm(H), np.linalg.norm(V)) / 4.0
    if name == "pinhole":
        centre, R = origin + 4.0 * (F - origin), 1.5
        assert np.arcsin(R / np.linalg.norm(centre - origin)) > 1.3 * np.arctan(half_diag / np.linalg.norm(F - origin))
    else:
        centre, R = F, 0.8
        assert R > 1.5 * half_diag
    recs = np.array([LI._sphere((0.0, -1000.0, 0.0), 1.0), LI._sphere(tuple(centre), R)])
    n = batches * per
    em = CR.emit(oracle, recs, [1], None, LI.states(n, 0xA11A), 0.0, 0.0)
    assert np.array_equal(em["pdf"][:, 0], np.full(n, 1.0 / ((4.0 * CR.PI) * (R * R))))
    pts = np.concatenate([em["rays"][:, 0:3], em["rays"][:, 6:7]], axis=1)
    con = CR.connect(oracle, cam, nrows, ncols, pts, LI.states(n, 0xC0CC))
    d = con["rays"][:, 3:6]
    with np.errstate(all="ignore"):
        cos_y = (em["normal"] * d).sum(axis=1) / np.sqrt((d * d).sum(axis=1))
    take = (con["pixel"] == 2 * ncols + 2) & (cos_y > 0)
    contrib = np.where(take, Le * cos_y * con["factor"] / em["pdf"][:, 0], 0.0)
    means = contrib.reshape(batches, per).mean(axis=1)
    mean, se = means.mean(), means.std(ddof=1) / np.sqrt(batches)
    print(f"{name}: {take.sum()} of {n} paths land in the pixel; estimate {mean:.4f} +- {se:.4f}, Le = {Le}")
    assert take.sum() > 500 and se > 0 and abs(mean - Le) <= 5 * se


@pytest.mark.parametrize("name", I.TABLES)
@pytest.mark.parametrize("tr", I.TIME_RANGES)
def test_emission_lands_on_the_lamp_and_leaves_it(oracle, name, tr):
    """|y - c| = R, |n| = |dir| = 1, n . dir = cos_t >= 0 within bounds from the operation counts, pdf_dir == cos_t / pi in every
    bit, the time inside its range and the centre the one at the drawn time."""
    recs, lights, weights = I.table(name, oracle)
    st = I.states(I.N_POINTS)
    res = CR.emit(oracle, recs, lights, weights, st, tr[0], tr[1])
    time = res["rays"][:, 6]
    assert (time >= tr[0]).all() and (time <= tr[1]).all() and (tr[0] == tr[1] or len(np.unique(time)) > 100)
    rec = recs[res["light"]]
    c = np.array([N._centre(rec[i], time[i]) for i in range(len(time))])
    R = np.abs(rec[:, 9])
    n, d, y = res["normal"], res["rays"][:, 3:6], res["rays"][:, 0:3]
    # n: three products and rr's sqrt of a three-operation argument: |n|^2 = 4 u (1 - u) + (1 - 2 u)^2 = 1 up to ~6 roundings
    assert (np.abs((n * n).sum(axis=1) - 1.0) <= 16 * EPS).all()
    # y = c + n * R: one product and one sum per component on top of n's error
    assert (np.abs(np.linalg.norm(y - c, axis=1) - R) <= 16 * EPS * (R + np.abs(c).sum(axis=1) + 1.0)).all()
    # dir: the frame's ~6 operations per entry, two sqrt, three products and two sums per component; the frame's entries are
    # bounded by 2, so 64 eps covers them
    assert (np.abs((d * d).sum(axis=1) - 1.0) <= 64 * EPS).all()
    assert (np.abs((n * d).sum(axis=1) - res["cos_t"]) <= 64 * EPS).all() and (res["cos_t"] >= 0).all()
    assert np.array_equal(res["pdf"][:, 1].view(np.uint64), (res["cos_t"] / CR.PI).view(np.uint64))
    with np.errstate(all="ignore"):
        P = CR.LR._weights(lights, weights)[res["pick"]] / CR.running_sums(CR.LR._weights(lights, weights))[-1]
        assert np.array_equal(res["pdf"][:, 0], P / ((4.0 * CR.PI) * (R * R)))
    assert (weights is None) or (np.asarray(weights)[res["pick"]] > 0).all()                   # a light of weight 0 is never picked
    if name == "ties":
        assert np.isinf(res["pdf"][res["pick"] == 0, 0]).all() and (res["pick"] == 0).any()    # radius 0: the point-light convention
    if name in ("three", "ties") and tr[1] > tr[0]:                                            # a mover's centre moves with the drawn time
        mover = rec[:, 0] == 1
        assert mover.any() and len(np.unique(c[mover, 1])) > 5


@pytest.mark.parametrize("name", ("three", "ties", "many65"))
def test_pick_frequencies_follow_the_weights(oracle, name):
    recs, lights, weights, res = _emission(oracle, name)
    w = np.asarray(weights, dtype=np.float64)
    n = len(res["pick"])
    share = w / w.sum()
    counts = np.bincount(res["pick"], minlength=len(w))
    sigma = np.sqrt(n * share * (1 - share))
    assert (np.abs(counts - n * share) <= 5 * sigma + 1e-9).all(), (counts, n * share)
    assert (counts[w == 0] == 0).all()


def test_positions_are_uniform_and_directions_cosine_weighted(oracle):
    recs, lights, weights, res = _emission(oracle, "one")
    n = len(res["pick"])
    zc = res["normal"][:, 2]
    az = np.arctan2(res["normal"][:, 1], res["normal"][:, 0])
    for values, lo, hi, bins in ((zc, -1.0, 1.0, 10), (az, -np.pi, np.pi, 8)):
        counts, _ = np.histogram(values, bins=bins, range=(lo, hi))
        p = 1.0 / bins
        assert (np.abs(counts - n * p) <= 5 * np.sqrt(n * p * (1 - p))).all(), counts
    cos_t = res["cos_t"]
    assert abs(cos_t.mean() - 2.0 / 3.0) <= 5 * cos_t.std(ddof=1) / np.sqrt(n)
    # the azimuth of the direction about the normal is uniform too: the projection on the frame's first axis averages 0
    d = res["rays"][:, 3:6] - res["normal"] * cos_t[:, None]
    assert (np.abs(d.mean(axis=0)) <= 5 * d.std(axis=0, ddof=1) / np.sqrt(n)).all()


def test_a_movers_centre_is_the_one_at_the_drawn_time(oracle):
    recs, lights, weights, res = _emission(oracle, "three", 2000, (0.25, 1.5))
    mover = res["light"] == 3
    assert mover.sum() > 500
    y, n, time = res["rays"][mover, 0:3], res["normal"][mover], res["rays"][mover, 6]
    c = np.array([N._centre(recs[3], t) for t in time])
    assert np.abs(y - n * abs(recs[3, 9]) - c).max() <= 1e-14 * 8 and len(np.unique(time)) > 400
    assert time.max() > 1.0                                               # beyond the mover's own interval: extrapolated, as the reference does


def test_draw_counts_are_fixed(oracle):
    """Every listed point draws exactly two, every listed path exactly six, whatever becomes of it; the others are untouched."""
    cam = I.camera(oracle, "lens")
    pts = I.points(cam, 5, 7)
    st = I.states(len(pts))
    res = CR.connect(oracle, cam, 5, 7, pts, st)
    assert (res["pixel"] < 0).any() and np.array_equal(res["states"], _advance(oracle, st, 2))
    pin = CR.connect(oracle, I.camera(oracle, "pinhole"), 5, 7, pts, st)
    assert np.array_equal(pin["states"], res["states"])                  # a pinhole draws its lens point too
    index = np.array([0, 3, -2, len(pts) + 5, 100, len(pts) - 1])
    listed = [0, 3, 100, len(pts) - 1]
    part = CR.connect(oracle, cam, 5, 7, pts, st, index)
    rest = np.ones(len(pts), dtype=bool)
    rest[listed] = False
    assert np.array_equal(part["states"][rest], st[rest]) and np.array_equal(part["states"][listed], res["states"][listed])
    assert (part["pixel"][rest] == -1).all() and np.array_equal(part["pixel"][listed], res["pixel"][listed])
    recs, lights, weights = I.table("three", oracle)
    for tr in I.TIME_RANGES:
        em = CR.emit(oracle, recs, lights, weights, st, tr[0], tr[1])
        assert np.array_equal(em["states"], _advance(oracle, st, 6))
        part = CR.emit(oracle, recs, lights, weights, st, tr[0], tr[1], index)
        assert np.array_equal(part["states"][rest], st[rest]) and np.array_equal(part["states"][listed], em["states"][listed])
        assert (part["light"][rest] == -1).all() and np.array_equal(part["rays"][listed], em["rays"][listed])


def test_ties_and_fallbacks_pick_what_the_header_says(oracle):
    w = np.array([1.0, 0.0, 1.0, 0.0, 2.0, 0.0])
    runs = CR.running_sums(w)
    assert runs.tolist() == [1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    x = np.array([0.0, np.nextafter(1.0, 0.0), 1.0, 1.5, 2.0, 3.0, np.nextafter(4.0, 0.0), 4.0, 5.0])
    assert CR.pick(runs, w, x).tolist() == [0, 0, 2, 2, 4, 4, 4, 4, 4]    # a tie goes past the equal sums; past the total: the last weight > 0
    assert CR.pick(np.array([0.0, 0.0, 3.0]), np.array([0.0, 0.0, 3.0]), np.array([0.0, 3.0])).tolist() == [2, 2]
    # the crafted states reach the tie through the entry: both draw 0.5 (HALF) or 1 - 2^-52 (LARGEST) for the time and the pick
    recs, lights, weights = I.table("ties", oracle)
    st = I.states(I.N_POINTS)
    res = CR.emit(oracle, recs, lights, weights, st, 0.0, 2.0)
    assert res["u"][-2, 0] == 0.5 and res["rays"][-2, 6] == 1.0 and res["pick"][-2] == 4 and res["light"][-2] == 5
    assert res["u"][-1, 0] == 1.0 - 2.0 ** -52 and res["pick"][-1] == 4
    recs, lights, weights = I.table("three", oracle)
    res = CR.emit(oracle, recs, lights, weights, st, 0.0, 0.0)
    assert res["pick"][-2] == 0 and res["pick"][-1] == 1                  # 1.375 < 2; just below 2.75: not the last light, whose weight is 0
