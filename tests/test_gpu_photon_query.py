"""The photon-map queries on the MI355X (tor_photons_build_device / _gather_device, the _host twins, tor_photons_info): for every case
of tests/photon_inputs.py sums and counts are those of the brute-force numpy restatement of include/tor_photons.h
(tests/photon_restatement.py), bit for bit, for both kernels at max_value 0.25, 1 and 128; lists, optional arrays and out= through
the Python layer; a rebuild replaces the map, which survives scene changes; a permuted build gives identical bits; 2^16 photons x
2^14 queries against the integer statement in torch; the refusals that read the context; trace_photons / trace_photon_map; and one
physics check: the irradiance under a spherical lamp against its closed form."""
import ctypes as C

import numpy as np
import pytest
import torch

import camera_inputs as CI
import light_inputs as LI
import photon_inputs as I
import photon_restatement as R

pytestmark = pytest.mark.gpu
_state = {}
KERNELS = ("constant", "epanechnikov")
MAX_VALUES = (0.25, 1.0, 128.0)


def _ctx(tor):
    if "ctx" not in _state:
        _state["ctx"] = tor.Context(0)
    return _state["ctx"]


def _cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _host(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    if a is None:
        return None
    return (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data) or None


def _want(case, kernel, mv):
    """The restatement's answer for a case: computed once, never changed."""
    key = (case["name"], kernel, mv)
    if key not in _state:
        _state[key] = R.agree(I.stored(case), case["points"], case["normals"], case["radius"], kernel, mv)
    return _state[key]


def raw_build(tor, ctx, pos, pw, dr, index, radius, device=True):
    """The C entry itself, on tensors or on host arrays; returns what must stay alive."""
    put = _cuda if device else _host
    arrs = [put(pos), put(pw), None if dr is None else put(dr), None if index is None else put(index, np.int32)]
    n, n_list = len(pos), (len(pos) if index is None else len(index))
    L = tor.lib()
    if device:
        rc = L.tor_photons_build_device(ctx._h, n, *[_ptr(a) for a in arrs], n_list, float(radius), torch.cuda.current_stream().cuda_stream)
    else:
        rc = L.tor_photons_build_host(ctx._h, n, *[_ptr(a) for a in arrs], n_list, float(radius))
    assert rc == 0, L.tor_last_error().decode()
    torch.cuda.synchronize()
    return arrs


def raw_gather(tor, ctx, pts, nrm, rad, index, kernel, mv, device=True, fill=7.0):
    put = _cuda if device else _host
    n = len(pts)
    arrs = [put(pts), None if nrm is None else put(nrm), None if rad is None else put(rad), None if index is None else put(index, np.int32)]
    sums, count = put(np.full((n, 3), fill)), put(np.full(n, 77), np.int32)
    L = tor.lib()
    args = (ctx._h, n, *[_ptr(a) for a in arrs], n if index is None else len(index), R.KERNELS[kernel], float(mv), _ptr(sums), _ptr(count))
    rc = L.tor_photons_gather_device(*args, torch.cuda.current_stream().cuda_stream) if device else L.tor_photons_gather_host(*args)
    assert rc == 0, L.tor_last_error().decode()
    torch.cuda.synchronize()
    f = (lambda v: v.cpu().numpy()) if device else np.asarray
    return {"sums": f(sums), "count": f(count)}


def build_case(tor, ctx, case, device=True):
    return raw_build(tor, ctx, case["position"], case["power"], case["direction"], case["index"], case["R"], device)


@pytest.mark.parametrize("name", [c["name"] for c in I.CASES])
def test_every_bit_against_the_restatement(tor, name):
    """The kernels on device arrays and the _host twins on host arrays: the map's counts, and sums and count of every point of the
    case in every bit, for both kernels at three clamps."""
    case = I.BY_NAME[name]
    ctx = _ctx(tor)
    m = I.stored(case)
    for device in (True, False):
        build_case(tor, ctx, case, device)
        assert ctx.photons_info() == R.info(m), (name, device)
        assert tor.last_note() == f"photons build: {m['n_buckets']} buckets"
        for kernel in KERNELS:
            for mv in MAX_VALUES:
                got = raw_gather(tor, ctx, case["points"], case["normals"], case["radius"], None, kernel, mv, device)
                want = _want(case, kernel, mv)
                print(name, device, kernel, mv, "accepted", int(want["count"].sum()), "mismatches", R.mismatches(got, want))
                assert not R.mismatches(got, want), (name, device, kernel, mv, R.mismatches(got, want))
                assert tor.last_note() == "photons gather"
    if name not in ("dense0",):
        assert _want(case, "constant", 1.0)["count"].sum() > 0        # not a comparison of zeros


def test_lists_optional_arrays_and_out_reuse(tor):
    """Through the Python layer, on tensors and on numpy operands: the power scale, a listed gather leaves the other points alone,
    normals and radius are optional, out= is written again."""
    case = I.BY_NAME["dense257"]
    ctx = _ctx(tor)
    rs = np.random.RandomState(5)
    n = len(case["points"])
    listed = rs.permutation(n)[: n // 3]
    index = np.concatenate([listed[:10], [-1, n, n + 700, -2 ** 31], listed[10:]]).astype(np.int32)
    for put in (_cuda, _host):
        power = case["power"] * 48.0                                   # the largest channel above 1: scaled by 2^-6
        pm = ctx.build_photons(put(case["position"]), put(power), put(case["direction"]), radius=case["R"])
        assert pm.scale == 2.0 ** -6 and pm.radius == case["R"] and pm.note.startswith("photons build")
        m = R.store(case["position"], power * pm.scale, case["direction"], case["R"])
        assert pm.info() == R.info(m) and pm.info() is pm.info()
        pts, nrm = put(case["points"]), put(case["normals"])
        for normals, radius, r_want in ((nrm, None, None), (None, None, None), (None, 0.7 * case["R"], np.full(n, 0.7 * case["R"])),
                                        (nrm, put(np.linspace(-0.1, 0.4, n)), np.linspace(-0.1, 0.4, n))):
            want = R.agree(m, case["points"], None if normals is None else case["normals"], r_want, "epanechnikov", 1.0)
            g = ctx.gather_photons(pts, normals, radius)
            torch.cuda.synchronize()
            as_np = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            got = {"sums": as_np(g.sums), "count": as_np(g.count)}
            assert not R.mismatches(got, want) and str(g.count.dtype).endswith("int32") and g.note == "photons gather"
            assert g.check_budget() == int(want["count"].max())
            # irradiance: the scale undone, 2 / (pi r^2), per path
            rr = np.full(n, case["R"]) if r_want is None else np.minimum(r_want, case["R"])
            with np.errstate(all="ignore"):
                e_want = np.where(want["count"][:, None] > 0, want["sums"] / pm.scale * (2.0 / (np.pi * rr * rr * 1000.0))[:, None], 0.0)
            assert np.allclose(as_np(g.irradiance(1000)), e_want, rtol=1e-14, atol=0.0)
            # a listed gather into the same buffers: sentinels outside the list
            g.sums[:], g.count[:] = 7.0, 77
            again = ctx.gather_photons(pts, normals, radius, index=put(index, np.int32), out=g)
            torch.cuda.synchronize()
            assert again.sums is g.sums and again.count is g.count
            got = {"sums": as_np(again.sums), "count": as_np(again.count)}
            rest = np.ones(n, dtype=bool)
            rest[listed] = False
            assert np.array_equal(R.bits(got["sums"][listed]), R.bits(want["sums"][listed])) and np.array_equal(got["count"][listed], want["count"][listed])
            assert (got["sums"][rest] == 7.0).all() and (got["count"][rest] == 77).all()
            # an empty list writes nothing
            ctx.gather_photons(pts, normals, radius, index=np.zeros(0, dtype=np.int32), out=g)
            torch.cuda.synchronize()
            assert (as_np(g.sums)[rest] == 7.0).all() and np.array_equal(R.bits(as_np(g.sums)[listed]), R.bits(want["sums"][listed]))
        with pytest.raises(ValueError):
            ctx.gather_photons(pts, out=ctx.gather_photons(pts[:5]))
        g0 = ctx.gather_photons(pts[:0])
        assert tuple(g0.sums.shape) == (0, 3) and g0.check_budget() == 0
    with pytest.raises(ValueError):
        ctx.build_photons(case["position"], case["power"])                                            # radius is required


def test_rebuild_replaces_and_the_map_survives_scene_changes(tor):
    ctx = _ctx(tor)
    a, b = I.BY_NAME["dense65"], I.BY_NAME["one_cell"]
    build_case(tor, ctx, a)
    first = raw_gather(tor, ctx, a["points"], a["normals"], None, None, "epanechnikov", 1.0)
    assert not R.mismatches(first, _want(a, "epanechnikov", 1.0))
    # scene uploads, a light table, an environment and other queries in between: the same bits afterwards
    recs, emission, lamp = LI.lamp_scene()
    ctx.upload(tor.Scene.from_records(recs).list())
    ctx.set_lights([lamp])
    ctx.set_environment(np.full((4, 4, 3), 0.5))
    rays = _cuda(np.array([[0.0, 0.0, 4.5, 0.0, 0.0, -1.0, 0.0]] * 70))
    ctx.hit(rays)
    ctx.upload(tor.Scene.from_records(recs[:2]).list())
    again = raw_gather(tor, ctx, a["points"], a["normals"], None, None, "epanechnikov", 1.0)
    assert not R.mismatches(again, first)
    # a rebuild replaces the map: a smaller one after a larger one, then the empty one
    build_case(tor, ctx, b)
    assert ctx.photons_info() == R.info(I.stored(b))
    assert not R.mismatches(raw_gather(tor, ctx, b["points"], None, None, None, "constant", 1.0), _want(b, "constant", 1.0))
    got_a_on_b = raw_gather(tor, ctx, a["points"], None, None, None, "constant", 1.0)
    assert not R.mismatches(got_a_on_b, R.agree(I.stored(b), a["points"], None, None, "constant", 1.0))
    build_case(tor, ctx, I.BY_NAME["dense0"])
    empty = raw_gather(tor, ctx, a["points"], None, None, None, "constant", 1.0)
    assert (empty["sums"] == 0).all() and (empty["count"] == 0).all()
    assert ctx.photons_info() == {"stored": 0, "dropped": 0, "n_buckets": 16, "largest_bucket": 0}
    # a list without a valid entry builds an empty map too (n_photons = 0 with a list; every entry out of range)
    raw_build(tor, ctx, a["position"], a["power"], None, np.array([-1, 65, 1000], dtype=np.int32), a["R"])
    assert ctx.photons_info() == {"stored": 0, "dropped": 0, "n_buckets": 16, "largest_bucket": 0}


@pytest.mark.parametrize("name", ["dense257", "one_cell", "listed"])
def test_a_permuted_build_gives_identical_bits(tor, name):
    case = I.BY_NAME[name]
    ctx = _ctx(tor)
    n = len(case["position"])
    perm = np.random.RandomState(9).permutation(n)
    index = None
    if case["index"] is not None:
        old = case["index"].astype(np.int64)
        index = np.where((old >= 0) & (old < n), np.argsort(perm)[np.clip(old, 0, n - 1)], -1).astype(np.int32)
    raw_build(tor, ctx, case["position"][perm], case["power"][perm], None if case["direction"] is None else case["direction"][perm],
              index, case["R"])
    for kernel in KERNELS:
        got = raw_gather(tor, ctx, case["points"], case["normals"], case["radius"], None, kernel, 1.0)
        assert not R.mismatches(got, _want(case, kernel, 1.0)), kernel
    # and twice the same build: the scatter's atomics may order a bucket differently, the bits do not move
    build_case(tor, ctx, case)
    one = raw_gather(tor, ctx, case["points"], case["normals"], case["radius"], None, "epanechnikov", 128.0)
    build_case(tor, ctx, case)
    two = raw_gather(tor, ctx, case["points"], case["normals"], case["radius"], None, "epanechnikov", 128.0)
    assert not R.mismatches(one, two) and not R.mismatches(one, _want(case, "epanechnikov", 128.0))


def test_large_map_against_the_integer_statement_in_torch(tor):
    """2^16 photons x 2^14 queries: the grid against brute force over all pairs, in integers (units of 2^-36), chunked in torch."""
    ctx = _ctx(tor)
    g = torch.Generator(device="cpu").manual_seed(77)
    n_ph, n_q, rad = 1 << 16, 1 << 14, 0.25
    h = float(R.cell_size(rad))
    pos = ((torch.rand((n_ph, 3), generator=g, dtype=torch.float64) - 0.5) * 32.0 * h).cuda()
    pw = torch.rand((n_ph, 3), generator=g, dtype=torch.float64).cuda()
    dr = (torch.rand((n_ph, 3), generator=g, dtype=torch.float64) - 0.5).cuda()
    pts = ((torch.rand((n_q, 3), generator=g, dtype=torch.float64) - 0.5) * 33.0 * h).cuda()
    nrm = (torch.rand((n_q, 3), generator=g, dtype=torch.float64) - 0.5).cuda()
    pm = ctx.build_photons(pos, pw, dr, radius=rad)
    assert pm.scale == 1.0 and pm.info()["stored"] == n_ph and pm.info()["n_buckets"] == 1 << 17 and pm.info()["dropped"] == 0
    for kernel, normals in (("epanechnikov", nrm), ("constant", None)):
        got = ctx.gather_photons(pts, normals, kernel=kernel)
        r2 = rad * rad
        sums, count = torch.zeros((n_q, 3), dtype=torch.int64, device="cuda"), torch.zeros(n_q, dtype=torch.int64, device="cuda")
        for lo in range(0, n_q, 512):
            x = pts[lo:lo + 512]
            e0, e1, e2 = (pos[None, :, k] - x[:, None, k] for k in range(3))
            d2 = (e0 * e0 + e1 * e1) + e2 * e2
            acc = d2 < r2
            if normals is not None:
                nn = normals[lo:lo + 512]
                acc &= ((dr[None, :, 0] * nn[:, None, 0] + dr[None, :, 1] * nn[:, None, 1]) + dr[None, :, 2] * nn[:, None, 2]) < 0.0
            w = 1.0 - d2 / r2 if kernel == "epanechnikov" else torch.ones_like(d2)
            for ch in range(3):
                a = pw[None, :, ch] * w
                a = torch.where(a < 1.0, a, torch.ones_like(a))
                sums[lo:lo + 512, ch] = torch.where(acc, torch.round(a * 2.0 ** 36).to(torch.int64), torch.zeros_like(count[:1])).sum(dim=1)
            count[lo:lo + 512] = acc.sum(dim=1)
        assert int(count.max()) * 1.0 < 2 ** 17 and got.check_budget() == int(count.max())
        assert torch.equal(got.count.long(), count) and int(count.sum()) > 2 * n_q
        assert torch.equal(got.sums.view(torch.int64), (sums.double() * 2.0 ** -36).view(torch.int64))


def test_refusals_that_read_the_context(tor):
    L = tor.lib()
    fresh = tor.Context(0)
    err = lambda: L.tor_last_error().decode()
    pts = _cuda(np.zeros((4, 3)))
    with pytest.raises(tor.TorError, match="no photon map built"):
        fresh.gather_photons(pts)
    with pytest.raises(tor.TorError, match="no photon map built"):
        fresh.gather_photons(np.zeros((4, 3)))
    with pytest.raises(tor.TorError, match="no photon map built"):
        fresh.photons_info()
    # the order: the NULL outputs come before the map
    assert L.tor_photons_gather_device(fresh._h, 4, pts.data_ptr(), None, None, None, 4, 1, 1.0, None, None, None) == -1 and "NULL" in err()
    # a refused build keeps the previous map; a map without directions refuses normals
    case = I.BY_NAME["one_cell"]
    build_case(tor, fresh, case)
    assert L.tor_photons_build_device(fresh._h, 4, pts.data_ptr(), pts.data_ptr(), None, None, 4, float("nan"), None) == -1 and "radius" in err()
    assert fresh.photons_info() == R.info(I.stored(case))
    with pytest.raises(tor.TorError, match="built without directions"):
        fresh.gather_photons(pts, normals=pts)
    fresh.close()


def _lamp_over_floor(tor, ctx, le, rho=0.25, h0=2.0):
    """A lamp sphere of radius rho and radiance le, its centre h0 above the top (the origin) of a diffuse sphere of radius 1000."""
    recs = np.array([LI._sphere((0.0, -1000.0, 0.0), 1000.0, LI.LAMB, (0.5, 0.25, 0.125)),
                     LI._sphere((0.0, h0, 0.0), rho, LI.LAMB, (0.0, 0.0, 0.0))])
    emission = np.zeros((2, 3))
    emission[1] = le
    ctx.upload(tor.Scene.from_records(recs).list())
    ctx.set_lights([1])
    return recs, emission, np.array([True, False])


def _states(tor, n, seed):
    return torch.from_numpy(tor.rng_seed2(np.full(n, seed, dtype=np.uint64), np.arange(n, dtype=np.uint64)).view(np.int64)).cuda()


def test_irradiance_under_a_spherical_lamp(tor):
    """The one asserted physics check.  A sphere of radius rho and uniform radiance Le, centre at height h0 above a plane, gives
    the point under it the irradiance E = pi Le sin^2(theta) = pi Le rho^2 / h0^2, exactly.  2^18 light paths, one step each
    (the lamp is black, the floor's reflections find no second emitter: only direct photons carry power), gathered with the
    Epanechnikov kernel of radius r about the nadir.

    Expected count: the disc receives E pi r^2 of the lamp's Le pi 4 pi rho^2, a share r^2 / (4 h0^2) = 0.0025: about 655 photons.
    Noise: the weights are w = 1 - u, u uniform on (0, 1) over the disc, E[w] = 1/2, E[w^2] = 1/3; a Poisson number N of equal
    photons gives the weighted sum the relative variance E[w^2] / (N E[w]^2) = 4 / (3 N): five standard errors, from the
    gathered count.
    Bias: at the distance s from the nadir the plane receives E (1 + s^2 / h0^2)^(-3/2); under the kernel E[s^2] = r^2 / 3 and
    E[s^4] = r^4 / 6, so the estimate is low by r^2 / (2 h0^2) = 0.5 % to first order, with a second-order term of
    (15 / 8) r^4 / (6 h0^4) = 3e-5.  The floor is a sphere of radius 1000: within r it drops by r^2 / 2000 = 2e-5 and tilts by
    r / 1000 = 2e-4 rad, which move distance and cosine by less than 1e-4 relative.  The tolerance takes the first-order bias
    whole plus 2e-4 for the rest -- computed before the run, not fitted to it."""
    ctx = _ctx(tor)
    le = np.array([8.0, 4.0, 2.0])
    rho, h0, r, paths = 0.25, 2.0, 0.2, 1 << 18
    _, emission, diffuse = _lamp_over_floor(tor, ctx, le, rho, h0)
    ph = ctx.trace_photons(_states(tor, paths, 0xF070), emission, diffuse, max_depth=1)
    assert ph.paths == paths and len(ph.position) > paths // 20 and (ph.direction[:, 1] < 0).all()
    pm = ctx.build_photons(ph.position, ph.power, ph.direction, radius=r)
    assert pm.info()["dropped"] == 0 and pm.info()["stored"] == len(ph.position)
    g = ctx.gather_photons(_cuda([[0.0, 0.0, 0.0]]), _cuda([[0.0, 1.0, 0.0]]))
    g.check_budget()
    count = int(g.count[0])
    est = g.irradiance(paths)[0].cpu().numpy()
    want = np.pi * le * rho * rho / (h0 * h0)
    tol = 5.0 * np.sqrt(4.0 / (3.0 * count)) + r * r / (2.0 * h0 * h0) + 2e-4
    print("count", count, "estimate / analytic", est / want, "tolerance", tol)
    assert 400 <= count <= 950                                     # 655 expected: +-10 sigma of a Poisson count
    assert (np.abs(est / want - 1.0) <= tol).all(), (est, want, tol)
    # the constant kernel agrees within its own noise (relative variance 1 / N) and half the bias
    g0 = ctx.gather_photons(_cuda([[0.0, 0.0, 0.0]]), _cuda([[0.0, 1.0, 0.0]]), kernel="constant")
    est0 = g0.irradiance(paths)[0].cpu().numpy()
    assert (np.abs(est0 / want - 1.0) <= 5.0 / np.sqrt(count) + 3.0 * r * r / (4.0 * h0 * h0) + 2e-4).all(), (est0, want)

    # trace_photon_map on the same map: a ray straight down sees albedo / pi * the estimate at its hit, a ray at the lamp sees Le,
    # a ray past everything is black
    rays = _cuda([[0.0, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0], [0.05, 1.0, 0.02, 0.0, -1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0],
                  [0.0, 1.0, 0.0, 1.0, 0.3, 0.0, 0.0]])
    color, _, mode = ctx.trace_photon_map(rays, _states(tor, 4, 3), emission, diffuse, paths)
    hits = ctx.hit(rays[:2])
    ge = ctx.gather_photons(hits.p.contiguous(), hits.normal.contiguous()).irradiance(paths).cpu().numpy()
    albedo = np.array([0.5, 0.25, 0.125])
    assert np.allclose(color[:2].cpu().numpy(), albedo / np.pi * ge, rtol=1e-12) and (ge > 0).all()
    assert np.array_equal(color[2].cpu().numpy(), le) and (color[3] == 0).all()


def test_caustic_only_keeps_what_went_through_glass(tor):
    ctx = _ctx(tor)
    n = 1 << 14
    for scene, expect_caustics in ((CI.diffuse_scene, False), (CI.caustic_scene, True)):
        recs, emission, lamp = scene()
        ctx.upload(tor.Scene.from_records(recs).list())
        ctx.set_lights([lamp])
        diffuse = tor.diffuse_objects(recs)
        every = ctx.trace_photons(_states(tor, n, 11), emission, diffuse, max_depth=8)
        caus = ctx.trace_photons(_states(tor, n, 11), emission, diffuse, max_depth=8, caustic_only=True)
        assert len(every.position) > n and every.paths == caus.paths == n
        assert torch.isfinite(every.power).all() and (every.power >= 0).all()
        if not expect_caustics:       # the metal ball is the only specular object; few paths meet it first
            assert len(caus.position) < len(every.position) // 20
        else:
            assert 0 < len(caus.position) < len(every.position) // 2
            assert len(caus.position) <= n                             # at most one photon per path: it stops at its first diffuse hit
        host = ctx.trace_photons(tor.rng_seed2(np.full(64, 11, dtype=np.uint64), np.arange(64, dtype=np.uint64)), emission, diffuse, max_depth=3)
        assert isinstance(host.position, np.ndarray) and host.position.shape[1] == 3 and host.paths == 64
