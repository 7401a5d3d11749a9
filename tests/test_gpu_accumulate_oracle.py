"""The sample-range kernels held to the CPU oracle (oracle.accumulate): the raw sums and second moments of every sample-stream
variant of integrate_kernel -- SEEDING 1 (plain passes), 3 (+ second moments), 4 (+ over a pixel list), each in its 12 builds --
equal the oracle's bit for bit, on scenes that reach every build; the list path at its edges; the noise estimate and the select on
oracle-confirmed data, including exact ties with the tolerance; and the select's ordered compaction at its block boundaries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W = 24, 40
PASSES = ((5, 12), (12, 22))  # [5, 12) + [12, 22): first_sample != 0, 17 samples in all
FIRST, TOTAL = PASSES[0][0], PASSES[-1][1] - PASSES[0][0]
Q = 2.0 ** -36

# the 36 sample-stream variants: {seeding, arith, w, f32, blocks}
ALL_VARIANTS = {(s, 2, w, 0, 0) for s in (1, 3, 4) for w in (2, 3)} | \
               {(s, 0, w, f, b) for s in (1, 3, 4) for w in (2, 3) for f, b in ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2))}


@pytest.fixture(scope="module")
def torch():
    import torch as T
    return T


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
# kind c0 c1 t0 t1 radius mat albedo fuzz ri
EDGE_RECORDS = [
    [0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0],
    [1, 0, 1, 0, 0, 1.5, 0, 0.0, 1.0, 1.0, 0, .8, .3, .3, 0, 0],       # group (0,1)
    [1, -4, 1, 0, -4, 1, 1, 0.25, 0.75, 1.0, 1, .7, .6, .5, 0.3, 0],   # group (.25,.75), moves in z
    [1, 4, 1, 0, 5, 1, 0, 0.25, 0.75, 1.0, 2, 0, 0, 0, 0, 1.5],        # same group, glass, moves in x
    [1, 2, .5, 2, 2, .5, 2, 0.5, 0.5, 0.5, 0, .1, .9, .1, 0, 0],       # time0 == time1: never hit
    [0, 1, .4, 3, 1, .4, 3, 0, 1, 0.4, 1, .9, .9, .9, 0.0, 0],
    [0, 1, .4, 3, 1, .4, 3, 0, 1, 0.4, 0, .2, .2, .9, 0.0, 0],         # exact duplicate: tie -> lowest index
    [0, -1, .3, 2, -1, .3, 2, 0, 1, -0.3, 2, 0, 0, 0, 0, 1.5],         # negative radius (hollow glass)
]
# every sphere encloses the camera: all 300 are candidates of every ray -- the object loop's queue overflows and resumes
# (every path ends inside them at depth 8: the frame is black, so it only holds the overflow path to depositing nothing wrong)
OVERFLOW_RECORDS = [[0, 13, 2, 3, 13, 2, 3, 0, 1, 5.0 + 0.01 * i, 2, 0, 0, 0, 0, 1.5] for i in range(300)]
# ... and a lit one: 300 concentric spheres in front of the camera, lambertian, metal and glass in turn -- a ray near the centre
# has all 300 as candidates, and the frame is not black
OVERFLOW_LIT_RECORDS = [[0, 0, 1, 0, 0, 1, 0, 0, 1, 0.5 + 0.01 * i, i % 3, .9, .7 - 0.001 * i, .5, 0.1, 1.5] for i in range(300)]


def _two_level_records(n=900, seed=20261016):
    """A ground sphere and n small spheres in front of the default camera: static ones and movers, lambertian, metal and glass, a
    few hollow -- more than 96 blocks of 8, so a two-level culling layout.  The movers share one time group, as random_scene's do:
    the float32 block records (and with them the blocks = 2 variants) need at most one."""
    rng = np.random.default_rng(seed)
    recs = [[0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0]]
    for _ in range(n):
        x, z = rng.uniform(-11, 11), rng.uniform(-11, 11)
        r = float(rng.choice([0.15, 0.2, 0.25])) * (1 if rng.random() > 0.05 else -1)
        y = abs(r) + rng.uniform(0.0, 0.5)
        mat = int(rng.integers(0, 3))
        alb = rng.uniform(0.1, 0.95, 3)
        fuzz, ri = rng.uniform(0, 0.5), rng.uniform(1.3, 1.7)
        if rng.random() < 0.5:
            recs.append([0, x, y, z, x, y, z, 0, 1, r, mat, *alb, fuzz, ri])
        else:
            d = rng.uniform(-0.4, 0.4, 3) * np.array([1.0, 0.5, 1.0])
            recs.append([1, x, y, z, x + d[0], y + d[1], z + d[2], 0.0, 1.0, r, mat, *alb, fuzz, ri])
    return np.asarray(recs, dtype=np.float64)


@pytest.fixture(scope="module")
def scenes(tor, ref_scene):
    """name -> (tor.Scene, oracle records, max_depth, two_level)"""
    out = {"facade": (tor.random_scene(0xFACADE), ref_scene[0], 50)}
    for name, recs, depth in (("edge", EDGE_RECORDS, 50), ("overflow", OVERFLOW_RECORDS, 8),
                              ("overflow_lit", OVERFLOW_LIT_RECORDS, 50), ("two_level", _two_level_records(), 50)):
        recs = np.asarray(recs, dtype=np.float64)
        out[name] = (tor.Scene.from_records(recs), recs, depth)
    res = {}
    for name, (scene, recs, depth) in out.items():
        lay = tor.debug_accel_layout(scene.list(), 0.0, 1.0)
        res[name] = (scene, recs, depth, lay is not None and lay[3])
    assert not res["facade"][3] and tor.debug_accel_layout(res["facade"][0].list(), 0.0, 1.0) is not None
    assert res["two_level"][3], "the two-level scene must have a two-level culling layout"
    return res


_ORACLE = {}


def _oracle(oracle, ref_camera, scenes, name, first, n, h=H, w=W, pixels=None):
    """(S, M) of the oracle, cached: the same samples are asked for by many variants."""
    key = (name, first, n, h, w, None if pixels is None else np.asarray(pixels).tobytes())
    if key not in _ORACLE:
        _, recs, depth, _ = scenes[name]
        _ORACLE[key] = oracle.accumulate(h, w, first, n, ref_camera, recs, depth, pixels=pixels)
    return _ORACLE[key]


def _expect(seeding, accel, w, screen, two_level):
    f32 = 1 if accel & 2 else 0
    blocks = (2 if two_level and f32 else 1) if accel & 1 else 0
    arith = 2 if (screen and f32 == 0 and blocks == 0) else 0
    return (seeding, arith, w, f32, blocks)


def _prior(torch, shape, seed):
    """A non-zero prior: multiples of 2^-36 up to 4, as a pixel's sums after earlier passes could be."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(1, 2 ** 38, size=shape).astype(np.float64) * Q).cuda()


def _gapped_list(npix, length, seed):
    """Strictly ascending, with gaps; holds pixel 0 and the last pixel when length >= 2."""
    rng = np.random.default_rng(seed)
    if length == 1:
        return np.array([int(rng.integers(0, npix))], dtype=np.int32)
    mid = rng.choice(np.arange(1, npix - 1), size=length - 2, replace=False)
    return np.sort(np.concatenate([[0, npix - 1], mid])).astype(np.int32)


def _run_passes(tor, torch, ctx, seeding, accel, h, w, depth, passes, lst=None, seed=0, **opt):
    """Passes of one variant into fresh buffers; returns (S, M or None, prior S, prior M, variants seen)."""
    options = tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel, **opt)
    rows = len(tor.shard_rows(h, max(opt.get("row_tile", 1), 1), opt.get("shard_index", 0), max(opt.get("shard_count", 1), 1)))
    shape = (rows, w, 3)
    if seeding == 4:
        sums, mom = _prior(torch, shape, seed), _prior(torch, shape, seed + 1)
    else:
        sums = torch.zeros(shape, dtype=torch.float64, device="cuda")
        mom = torch.zeros_like(sums) if seeding == 3 else None
    s0 = sums.cpu().numpy()
    m0 = mom.cpu().numpy() if mom is not None else None
    seen = []
    for first, end in passes:
        if seeding == 4:
            ctx.accumulate_list_device(tor.camera(), h, w, lst.data_ptr(), lst.numel(), first, end - first, depth, options, sums.data_ptr(),
                                       mom.data_ptr(), _stream(torch))
        else:
            ctx.accumulate_device(tor.camera(), h, w, first, end - first, depth, options, sums.data_ptr(),
                                  mom.data_ptr() if mom is not None else 0, _stream(torch))
        seen.append(ctx.last_variant())
    torch.cuda.synchronize()
    return sums.cpu().numpy(), (mom.cpu().numpy() if mom is not None else None), s0, m0, seen


def _check_against_oracle(tag, seeding, got_s, got_m, s0, m0, want_s, want_m, pix=None):
    if seeding != 4:
        assert np.array_equal(got_s, want_s), f"{tag}: sums differ from the oracle in {(got_s != want_s).sum()} values"
        if seeding == 3:
            assert np.array_equal(got_m, want_m), f"{tag}: moments differ from the oracle in {(got_m != want_m).sum()} values"
        return
    on = np.zeros(got_s.shape[0] * got_s.shape[1], dtype=bool)
    on[pix] = True
    for what, got, prior, want in (("sums", got_s, s0, want_s), ("moments", got_m, m0, want_m)):
        g, p0, wv = got.reshape(-1, 3), prior.reshape(-1, 3), want.reshape(-1, 3)
        bad = (g[on] != p0[on] + wv[on]).sum()
        assert bad == 0, f"{tag}: listed {what} differ from prior + oracle in {bad} values"
        assert np.array_equal(g[~on], p0[~on]), f"{tag}: unlisted {what} changed"


def _list_for(h, w, seed):
    npix = h * w
    pix = _gapped_list(npix, npix // 3 + 7, seed)
    assert len(pix) % 64 != 0
    return pix


# ---- 1. every variant against the oracle ----------------------------------------------------------------------------------------
def test_all_36_variants_match_the_oracle(tor, torch, oracle, ref_camera, scenes, monkeypatch):
    seen = set()
    pix = _list_for(H, W, 7)
    lst = torch.from_numpy(pix).cuda()
    for wps in (2, 3):
        for screen in (0, 1):
            monkeypatch.setenv("TOR_WAVES_PER_SIMD", str(wps))
            monkeypatch.setenv("TOR_SCREEN", str(screen))
            ctx = tor.Context()
            assert ctx.last_variant() == (-1, -1, -1, -1, -1)
            for name, accels in (("facade", (0, 1, 2, 3)), ("two_level", (1, 3))):
                scene, _, depth, two = scenes[name]
                ctx.upload(scene.list())
                want_s, want_m = _oracle(oracle, ref_camera, scenes, name, FIRST, TOTAL)
                for accel in accels:
                    for seeding in (1, 3, 4):
                        tag = f"W={wps} screen={screen} {name} accel={accel} seeding={seeding}"
                        S, M, s0, m0, got = _run_passes(tor, torch, ctx, seeding, accel, H, W, depth, PASSES, lst, seed=seeding * 10 + accel)
                        want_v = _expect(seeding, accel, wps, screen, two)
                        assert all(v == want_v for v in got), f"{tag}: launched {got}, expected {want_v}"
                        seen.add(want_v)
                        _check_against_oracle(tag, seeding, S, M, s0, m0, want_s, want_m, pix)
            ctx.close()
    assert seen == ALL_VARIANTS, f"variants never run: {sorted(ALL_VARIANTS - seen)}"


# ---- 2. the scenes of the parity suite, on a default context -------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_ctx(tor):
    import os
    saved = {k: os.environ.pop(k) for k in ("TOR_WAVES_PER_SIMD", "TOR_SCREEN") if k in os.environ}
    try:
        c = tor.Context()
    finally:
        os.environ.update(saved)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["facade", "edge", "overflow", "overflow_lit", "two_level"])
def test_scenes_match_the_oracle(tor, torch, oracle, ref_camera, scenes, default_ctx, name):
    scene, _, depth, _ = scenes[name]
    default_ctx.upload(scene.list())
    want_s, want_m = _oracle(oracle, ref_camera, scenes, name, FIRST, TOTAL)
    assert (float(want_s.max()) == 0.0) if name == "overflow" else (float(want_s.min()) >= 0.0 and float(want_s.max()) > 0.0)
    pix = _list_for(H, W, 11)
    lst = torch.from_numpy(pix).cuda()
    for accel in (0, 1, 2, 3):
        for seeding in (1, 3, 4):
            tag = f"{name} accel={accel} seeding={seeding}"
            S, M, s0, m0, got = _run_passes(tor, torch, default_ctx, seeding, accel, H, W, depth, PASSES, lst, seed=100 + accel)
            assert all(v[0] == seeding and v[2] in (2, 3) for v in got), f"{tag}: launched {got}"
            _check_against_oracle(tag, seeding, S, M, s0, m0, want_s, want_m, pix)


# ---- 3. edges of the list path ---------------------------------------------------------------------------------------------------
LH, LW = 32, 48  # 1536 pixels: room for a list of 1000
LIST_EDGES = [(1, 1), (1, 1000), (2, 2), (2, 65), (3, 63), (3, 1000), (63, 2), (63, 64), (64, 1), (64, 65), (65, 63), (65, 1000)]


@pytest.mark.parametrize("accel", [0, 3])
def test_list_edges_match_the_oracle(tor, torch, oracle, ref_camera, scenes, default_ctx, accel):
    scene, _, depth, _ = scenes["facade"]
    default_ctx.upload(scene.list())
    for k, (n, length) in enumerate(LIST_EDGES):
        # every other pair ends its range at the 2^17 bound
        first = 2 ** 17 - n if k % 2 else 3 * k + 1
        pix = _gapped_list(LH * LW, length, 1000 + k)
        lst = torch.from_numpy(pix).cuda()
        want_s, want_m = _oracle(oracle, ref_camera, scenes, "facade", first, n, LH, LW, pixels=pix)
        S, M, s0, m0, got = _run_passes(tor, torch, default_ctx, 4, accel, LH, LW, depth, ((first, first + n),), lst, seed=2000 + k)
        assert got[0][0] == 4
        _check_against_oracle(f"accel={accel} n={n} list={length} first={first}", 4, S, M, s0, m0, want_s, want_m, pix)


@pytest.mark.parametrize("accel", [0, 3])
def test_list_entries_outside_the_shard_deposit_nothing(tor, torch, oracle, ref_camera, scenes, default_ctx, accel):
    scene, _, depth, _ = scenes["facade"]
    default_ctx.upload(scene.list())
    npix, guard = H * W, 4096
    inside = _gapped_list(npix, 150, 31)
    pix = np.concatenate([inside, [npix, npix + 1, npix + 63, npix + 1000]]).astype(np.int32)
    lst = torch.from_numpy(pix).cuda()
    opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel)
    # buffers with a guard region behind the frame: an entry >= npix that deposited would land there
    sums = _prior(torch, (npix + guard, 3), 41)
    mom = _prior(torch, (npix + guard, 3), 42)
    s0, m0 = sums.cpu().numpy(), mom.cpu().numpy()
    for first, end in PASSES:
        default_ctx.accumulate_list_device(tor.camera(), H, W, lst.data_ptr(), lst.numel(), first, end - first, depth, opt, sums.data_ptr(),
                                           mom.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    assert default_ctx.last_variant()[0] == 4
    S, M = sums.cpu().numpy(), mom.cpu().numpy()
    assert np.array_equal(S[npix:], s0[npix:]) and np.array_equal(M[npix:], m0[npix:]), "an entry outside the shard deposited"
    want_s, want_m = _oracle(oracle, ref_camera, scenes, "facade", FIRST, TOTAL)
    _check_against_oracle(f"accel={accel} off-shard entries", 4, S[:npix].reshape(H, W, 3), M[:npix].reshape(H, W, 3),
                          s0[:npix].reshape(H, W, 3), m0[:npix].reshape(H, W, 3), want_s, want_m, inside)


@pytest.mark.parametrize("accel", [0, 3])
def test_list_on_a_row_shard(tor, torch, oracle, ref_camera, scenes, default_ctx, accel):
    scene, _, depth, _ = scenes["facade"]
    default_ctx.upload(scene.list())
    shard = dict(shard_index=1, shard_count=3, row_tile=4)
    rows = tor.shard_rows(H, 4, 1, 3)
    local = _gapped_list(len(rows) * W, 101, 51)   # shard-local indices
    image = (rows[local // W] * W + local % W).astype(np.int32)
    lst = torch.from_numpy(local).cuda()
    S, M, s0, m0, got = _run_passes(tor, torch, default_ctx, 4, accel, H, W, depth, PASSES, lst, seed=61, **shard)
    assert S.shape == (len(rows), W, 3) and all(v[0] == 4 for v in got)
    ws, wm = _oracle(oracle, ref_camera, scenes, "facade", FIRST, TOTAL, pixels=image)
    _check_against_oracle(f"accel={accel} shard 1 of 3", 4, S, M, s0, m0, ws[rows], wm[rows], local)


# ---- 4. noise estimate and select on oracle-confirmed data ----------------------------------------------------------------------
def _numpy_err(S, M, n):
    n = np.float64(n)
    var = (M - S * S / n) / (n - np.float64(1.0))
    var = np.where(var > 0.0, var, 0.0)
    return np.sqrt(var / n).max(axis=-1)


def _oracle_confirmed(tor, torch, oracle, ref_camera, scenes, ctx, n):
    """Sums and moments of samples [0, n) on the GPU, checked against the oracle: (S, M) on the host and on the device."""
    scene, _, depth, _ = scenes["facade"]
    ctx.upload(scene.list())
    S, M, _, _, _ = _run_passes(tor, torch, ctx, 3, 3, H, W, depth, ((0, n),))
    want_s, want_m = _oracle(oracle, ref_camera, scenes, "facade", 0, n)
    assert np.array_equal(S, want_s) and np.array_equal(M, want_m), "sums / moments differ from the oracle"
    return S, M, torch.from_numpy(S).cuda(), torch.from_numpy(M).cuda()


@pytest.mark.parametrize("n", [2, 17, 24])
def test_noise_estimate_on_oracle_data(tor, torch, oracle, ref_camera, scenes, default_ctx, n):
    S, M, sums, mom = _oracle_confirmed(tor, torch, oracle, ref_camera, scenes, default_ctx, n)
    npix = H * W
    err = torch.full((npix,), -1.0, dtype=torch.float64, device="cuda")
    mean, mx = default_ctx.accum_noise_device(sums.data_ptr(), mom.data_ptr(), npix, n, err.data_ptr(), _stream(torch))
    want = _numpy_err(S, M, n).reshape(-1)
    e = err.cpu().numpy()
    assert np.array_equal(e, want), f"per-pixel standard error differs from numpy in {(e != want).sum()} pixels"
    assert mx == float(want.max()) and mx > 0.0
    assert mean == pytest.approx(float(np.sum(want) / npix), rel=1e-13, abs=0)


@pytest.mark.parametrize("n", [2, 17, 24])
def test_select_ties_on_oracle_data(tor, torch, oracle, ref_camera, scenes, default_ctx, n):
    """abs_tol exactly at a pixel's standard error keeps it converged, one ulp below makes it active -- and the whole kept set is
    adaptive_select_host's both times."""
    S, M, sums, mom = _oracle_confirmed(tor, torch, oracle, ref_camera, scenes, default_ctx, n)
    npix = H * W
    want = _numpy_err(S, M, n).reshape(-1)
    # 20 pixels: where var * (1 / n) rounds differently from var / n (a rounding change would show there), then random ones
    rng = np.random.default_rng(n)
    var = np.maximum((M - S * S / n) / (n - 1.0), 0.0).reshape(-1, 3)
    c = np.argmax(np.sqrt(var / n), axis=1)
    v = var[np.arange(npix), c]
    sensitive = np.flatnonzero((want > 0.0) & (np.sqrt(v * (1.0 / n)) != want))
    picks = list(rng.permutation(sensitive)[:10])
    rest = np.setdiff1d(np.flatnonzero(want > 0.0), picks)
    picks += list(rng.choice(rest, size=20 - len(picks), replace=False))
    full = np.arange(npix, dtype=np.int32)
    lst = torch.from_numpy(full).cuda()
    out = torch.empty_like(lst)
    counts = torch.zeros(npix, dtype=torch.int32, device="cuda")
    for p in picks:
        for tol, active in ((float(want[p]), False), (float(np.nextafter(want[p], 0.0)), True)):
            k = default_ctx.adaptive_select_device(sums.data_ptr(), mom.data_ptr(), lst.data_ptr(), npix, n, tol, 0.0, out.data_ptr(),
                                                   counts.data_ptr(), _stream(torch))
            host = tor.adaptive_select_host(S, M, full, n, tol, 0.0)
            kept = out[:k].cpu().numpy()
            assert np.array_equal(kept, host), f"n={n} pixel {p} abs_tol={tol!r}: the select differs from adaptive_select_host"
            assert (p in set(kept.tolist())) == active, f"n={n} pixel {p} abs_tol={tol!r}: expected active={active}"


# ---- 5. the select's compaction at its block boundaries --------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", [1, 1023, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1])
def test_select_compaction_boundaries(tor, torch, default_ctx, n_in):
    n = 24
    npix = n_in + n_in // 3 + 5
    rng = np.random.default_rng(n_in)
    q = rng.uniform(0.01, 1.0, (npix, 3))
    u = rng.uniform(0.0, 1.0, (npix, 3))
    S = np.round(q * n / Q) * Q                               # multiples of 2^-36 in (0, n]
    M = np.round(S * S / n * (1.0 + 0.5 * u + 1e-3) / Q) * Q  # a variance > 0 in every channel
    pix = np.sort(rng.choice(npix, size=n_in, replace=False)).astype(np.int32)
    sums, mom = torch.from_numpy(S).cuda(), torch.from_numpy(M).cuda()
    lst = torch.from_numpy(pix).cuda()
    e = _numpy_err(S[pix], M[pix], n)
    for abs_tol, keep in ((1e9, "none"), (float(np.median(e)), "half"), (0.0, "all")):
        out = torch.full((n_in + 64,), -9, dtype=torch.int32, device="cuda")
        counts = torch.full((npix,), -7, dtype=torch.int32, device="cuda")
        k = default_ctx.adaptive_select_device(sums.data_ptr(), mom.data_ptr(), lst.data_ptr(), n_in, n, abs_tol, 0.0, out.data_ptr(),
                                               counts.data_ptr(), _stream(torch))
        want = tor.adaptive_select_host(S, M, pix, n, abs_tol, 0.0)
        if keep == "none":
            assert len(want) == 0
        elif keep == "all":
            assert len(want) == n_in
        else:
            assert abs(len(want) - n_in / 2) <= 1
        o = out.cpu().numpy()
        assert k == len(want), f"n_in={n_in} {keep}: n_out {k}, expected {len(want)}"
        assert np.array_equal(o[:k], want), f"n_in={n_in} {keep}: output order differs"
        assert np.all(o[k:] == -9), f"n_in={n_in} {keep}: the tail of list_out was written"
        c = counts.cpu().numpy()
        on = np.zeros(npix, dtype=bool)
        on[pix] = True
        assert np.all(c[on] == n) and np.all(c[~on] == -7), f"n_in={n_in} {keep}: counts not exactly on the listed pixels"
