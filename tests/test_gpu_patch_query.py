"""Planar patch queries on the MI355X (tor_scene_patches, tor_patch_info, tor_patch_hit_device / _host, tor_patch_occluded_device /
_host): for every case of tests/patch_inputs.py every bit of the records, patch, uv and the any-hit bits is the numpy restatement's
(tests/patch_restatement.py, which tests/test_patch_query.py anchors), through device and host entries, tensors and numpy, merge 0
and 1, a NULL d_uv, lists and out=; the any-hit merge ORs into occluded()'s bits; scatter() serves merged records; trace_patches
with a table no ray reaches is trace() and radiance(), and on a room it is the restated loop, bit for bit; the lifecycle; the
refusals that need a context."""
import ctypes as C

import numpy as np
import pytest
import torch

import bounce_restatement as BR
import hit_restatement as H
import patch_inputs as I
import patch_restatement as R
import radiance_restatement as RR

pytestmark = pytest.mark.gpu


def _patches(tor, table):
    return [tor.Patch(p["kind"], p["q"], p["u"], p["v"], p["material"], p["groups"]) for p in table]


def _ctx(tor, recs, table=None):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    if table is not None:
        ctx.set_patches(_patches(tor, table))
    return ctx


def _cuda(a, dtype=np.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np(ph):
    if isinstance(ph.raw, torch.Tensor):
        torch.cuda.synchronize()
        return {"raw": ph.raw.cpu().numpy(), "patch": ph.patch.cpu().numpy(), "uv": ph.uv.cpu().numpy()}
    return {"raw": ph.raw, "patch": ph.patch, "uv": ph.uv}


def _bits(oc):
    if isinstance(oc.raw, torch.Tensor):
        torch.cuda.synchronize()
        return oc.raw.cpu().numpy()
    return oc.raw


def _eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("name", I.NAMES)
def test_every_bit_of_every_case(tor, name):
    c, want = I.BY_NAME[name], I.answer(name)
    ctx = _ctx(tor, c["recs"], c["table"])
    assert ctx.patches() == (len(c["table"]), sum(p["material"] >= 0 for p in c["table"]))
    n = len(c["rays"])
    rays, tr, mask = _cuda(c["rays"]), _cuda(c["t_range"]), c["mask"]
    sphere = I.sphere_records(c)
    # tensors, the device entries
    ph = ctx.hit_patches(rays, tr, mask=mask)
    assert ph.mode == "patch hit" and tor.last_note() == "patch hit"
    bad = R.mismatches(_np(ph), want["hit"])
    assert not bad, bad
    oc = ctx.occluded_patches(rays, tr, mask=mask)
    assert oc.mode == "patch occluded" and not R.mismatches(_bits(oc), want["occluded"])
    ones = torch.ones(n, dtype=torch.int32, device="cuda")
    assert (_bits(ctx.occluded_patches(rays, tr, mask=mask, merge=ones)) == 1).all()                  # merge only ever writes 1
    assert not R.mismatches(_bits(ctx.occluded_patches(rays, tr, mask=mask, merge=0 * ones)), want["occluded"])
    # numpy, the blocking entries
    host = ctx.hit_patches(c["rays"], c["t_range"], mask=mask)
    assert isinstance(host.raw, np.ndarray) and not R.mismatches(_np(host), want["hit"])
    assert not R.mismatches(_bits(ctx.occluded_patches(c["rays"], c["t_range"], mask=mask)), want["occluded"])
    if sphere is not None:
        mg = ctx.hit_patches(rays, tr, mask=mask, merge=_cuda(sphere))
        bad = R.mismatches(_np(mg), want["merge"])
        assert not bad, bad
        hm = ctx.hit_patches(c["rays"], c["t_range"], mask=mask, merge=sphere)
        assert hm.raw is not sphere and not R.mismatches(_np(hm), want["merge"])
    # two halves through lists, the second into the first's result
    key = "merge" if sphere is not None else "hit"
    first, rest = np.arange(0, n, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)
    kw = dict(mask=mask, merge=None if sphere is None else _cuda(sphere))
    half = ctx.hit_patches(rays, tr, index=_cuda(first, np.int32), **kw)
    both = ctx.hit_patches(rays, tr, index=_cuda(rest, np.int32), out=half, **kw)
    assert both.raw.data_ptr() == half.raw.data_ptr() and not R.mismatches(_np(both), want[key])
    hh = ctx.hit_patches(c["rays"], c["t_range"], index=first, mask=mask, merge=sphere)
    hb = ctx.hit_patches(c["rays"], c["t_range"], index=rest, mask=mask, merge=sphere, out=hh)
    assert hb.raw is hh.raw and not R.mismatches(_np(hb), want[key])
    oh = ctx.occluded_patches(rays, tr, index=_cuda(first, np.int32), mask=mask)
    ob = ctx.occluded_patches(rays, tr, index=_cuda(rest, np.int32), mask=mask, out=oh)
    assert ob.raw.data_ptr() == oh.raw.data_ptr() and not R.mismatches(_bits(ob), want["occluded"])
    # the C entries themselves, without a uv output (it is nullable)
    L = tor.lib()
    words = None if mask is None or isinstance(mask, int) else np.ascontiguousarray(mask, dtype=np.uint32)
    m_ptr, m_word = (None, 0xFFFFFFFF if mask is None else int(mask)) if words is None else (words.ctypes.data, 0)
    raw, patch = np.full((n, 8), 7.0), np.full(n, 77, dtype=np.int32)
    tp = None if c["t_range"] is None else c["t_range"].ctypes.data
    assert L.tor_patch_hit_host(ctx._h, n, c["rays"].ctypes.data, tp, None, n, 0, raw.ctypes.data, patch.ctypes.data, None, m_ptr, m_word) == 0
    assert not H.mismatches(raw, want["hit"]["raw"]) and np.array_equal(patch, want["hit"]["patch"])
    d_raw, d_patch = torch.full((n, 8), 7.0, dtype=torch.float64, device="cuda"), torch.full((n,), 77, dtype=torch.int32, device="cuda")
    d_words = _cuda(words.view(np.int32), np.int32) if words is not None else None
    assert L.tor_patch_hit_device(ctx._h, n, rays.data_ptr(), None if tr is None else tr.data_ptr(), None, n, 0, d_raw.data_ptr(), d_patch.data_ptr(),
                                  None, torch.cuda.current_stream().cuda_stream, None if d_words is None else d_words.data_ptr(), m_word) == 0
    torch.cuda.synchronize()
    assert not H.mismatches(d_raw.cpu().numpy(), want["hit"]["raw"]) and np.array_equal(d_patch.cpu().numpy(), want["hit"]["patch"])


@pytest.mark.parametrize("length", [1, 63, 64, 65, 255])
def test_lists_leave_the_other_rays_alone(tor, length):
    c, want = I.BY_NAME["soup65"], I.answer("soup65")
    ctx = _ctx(tor, c["recs"], c["table"])
    n = len(c["rays"])
    index = I.lists(n)[length]
    listed = index[(index >= 0) & (index < n)]
    rest = np.ones(n, dtype=bool)
    rest[listed] = False

    def check(got, bits):
        assert not R.mismatches({k: v[listed] for k, v in got.items()}, {k: v[listed] for k, v in want["hit"].items()})
        assert (got["raw"][rest] == 7.0).all() and (got["patch"][rest] == 77).all() and (got["uv"][rest] == 7.0).all()
        assert np.array_equal(bits[listed], want["occluded"][listed]) and (bits[rest] == 77).all()
    raw = torch.full((n, 8), 7.0, dtype=torch.float64, device="cuda")
    out = tor.PatchHits(raw, raw.view(torch.int32), torch.full((n,), 77, dtype=torch.int32, device="cuda"),
                        torch.full((n, 2), 7.0, dtype=torch.float64, device="cuda"), "")
    bits = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    idx = _cuda(index, np.int32)
    check(_np(ctx.hit_patches(_cuda(c["rays"]), index=idx, out=out)), _bits(ctx.occluded_patches(_cuda(c["rays"]), index=idx, out=bits)))
    raw = np.full((n, 8), 7.0)
    hout = tor.PatchHits(raw, raw.view(np.int32), np.full(n, 77, dtype=np.int32), np.full((n, 2), 7.0), "")
    check(_np(ctx.hit_patches(c["rays"], index=index, out=hout)), _bits(ctx.occluded_patches(c["rays"], index=index, out=np.full(n, 77, dtype=np.int32))))
    empty = ctx.hit_patches(_cuda(c["rays"]), index=_cuda(np.zeros(0), np.int32), out=out)
    assert empty.mode == "patch_hit: nothing to do"


def test_occluded_patches_ors_into_occludeds_bits(tor):
    c = I.BY_NAME["room"]
    ctx = _ctx(tor, c["recs"], c["table"])
    rays = _cuda(c["rays"])
    spheres = ctx.occluded(rays)
    both = ctx.occluded_patches(rays, merge=spheres)
    torch.cuda.synchronize()
    s, b = spheres.raw.cpu().numpy(), both.raw.cpu().numpy()
    want = R.occluded(c["table"], c["rays"])
    assert np.array_equal(s != 0, H.fields(H.world_hit(c["recs"], c["rays"]))["object"] >= 0)
    assert np.array_equal(b, (s | want).astype(np.int32)) and (b[s != 0] == 1).all() and (s != 0).any() and (b != s).any()
    assert both.raw.data_ptr() != spheres.raw.data_ptr()
    in_place = ctx.occluded_patches(rays, merge=spheres, out=spheres)               # in place
    assert in_place.raw.data_ptr() == spheres.raw.data_ptr() and np.array_equal(_bits(in_place), b)


def test_scatter_serves_the_merged_records(tor, oracle):
    c = I.BY_NAME["room"]
    ctx = _ctx(tor, c["recs"], c["table"])
    n = len(c["rays"])
    st = tor.rng_seed1(np.arange(n) + 11)
    want_rec = I.answer("room")["merge"]
    want = BR.scatter(oracle, c["recs"], c["rays"], want_rec["raw"], st)
    rays, rng = _cuda(c["rays"]), _cuda(np.ascontiguousarray(st).view(np.int64), np.int64)
    merged = ctx.hit_patches(rays, merge=ctx.hit(rays))
    assert not R.mismatches(_np(merged), want_rec)
    res = ctx.scatter(rays.clone(), merged, rng.clone())
    torch.cuda.synchronize()
    assert _eq(res.rays.cpu().numpy(), want["rays"]) and np.array_equal(res.rng.cpu().numpy().view(np.uint64), want["states"])
    assert _eq(res.attenuation.cpu().numpy(), want["attenuation"]) and np.array_equal(res.status.cpu().numpy(), want["status"])
    lamp = want_rec["patch"] == I.ROOM_LAMP
    assert lamp.any() and (want["status"][lamp] == BR.MISS).all() and set(want["status"]) >= {BR.MISS, BR.SCATTERED}


def test_trace_patches_with_a_table_no_ray_reaches_is_trace_and_radiance(tor):
    scene = tor.random_scene()
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    rays, rng = ctx.camera_rays(tor.camera(), 16, 16, 0, 1, tor.SEED_SAMPLE)
    ctx.set_patches([tor.Patch.quad((2000.0, -1.0, -1.0), (0, 2, 0), (0, 0, 2), material=0), tor.Patch.triangle((2000, 0, 0), (2001, 0, 0), (2000, 1, 0))])
    want_c, want_s, _ = ctx.radiance(rays, rng.clone(), 8)
    for kw in ({}, {"emission": np.linspace(0.0, 1.0, 3 * len(scene)).reshape(-1, 3)}):
        tc, ts, _ = ctx.trace(rays, rng.clone(), 8, **kw)
        pc, ps, _ = ctx.trace_patches(rays, rng.clone(), 8, patch_emission=np.ones((2, 3)), **kw)
        torch.cuda.synchronize()
        assert torch.equal(ps, ts) and _eq(pc.cpu().numpy(), tc.cpu().numpy())
        if not kw:
            assert torch.equal(ps, want_s) and _eq(pc.cpu().numpy(), want_c.cpu().numpy()) and float(want_c.sum()) > 0
    masked_t, s1, _ = ctx.trace(rays, rng.clone(), 4, mask=5)
    masked_p, s2, _ = ctx.trace_patches(rays, rng.clone(), 4, mask=5)
    torch.cuda.synchronize()
    assert torch.equal(s1, s2) and _eq(masked_p.cpu().numpy(), masked_t.cpu().numpy())


def test_trace_patches_on_a_room_equals_the_restated_loop(tor, oracle):
    c = I.BY_NAME["room"]
    cam = oracle.camera(look_from=(0.0, 2.5, 9.0), look_at=(0.0, 2.25, 0.0), vfov=38.0, aspect=1.0)
    rays, st = RR.camera_rays(oracle, cam, 10, 10, None, 0, 2)
    depth = 6
    patch_emission = np.zeros((len(c["table"]), 3))
    patch_emission[I.ROOM_LAMP] = (12.0, 11.0, 9.0)
    emission = np.zeros((3, 3))
    emission[1] = (0.25, 0.5, 0.125)
    want_c, want_s = R.trace(oracle, c["recs"], c["table"], rays, st, depth, emission=emission, patch_emission=patch_emission)
    plain_c, _ = BR.trace(oracle, c["recs"], rays, st, depth, emission=emission)
    assert not _eq(want_c, plain_c) and (want_c > 0).any() and np.isfinite(want_c).all()
    ctx = _ctx(tor, c["recs"], c["table"])
    color, st_out, _ = ctx.trace_patches(_cuda(rays), _cuda(st.view(np.int64), np.int64), depth, emission=_cuda(emission), patch_emission=patch_emission)
    torch.cuda.synchronize()
    assert _eq(color.cpu().numpy(), want_c) and np.array_equal(st_out.cpu().numpy().view(np.uint64), want_s)
    color, st_out, _ = ctx.trace_patches(rays, st, depth, emission=emission, patch_emission=patch_emission)   # numpy operands
    assert _eq(color, want_c) and np.array_equal(st_out, want_s)
    color, _, _ = ctx.trace(rays, st, depth, emission=emission)                     # trace() never reads the table
    assert _eq(color, plain_c)


# ---- the lifecycle, the refusals, the info --------------------------------------------------------------------------------------------

def test_lifecycle(tor):
    c, want = I.BY_NAME["soup9"], I.answer("soup9")
    ctx = _ctx(tor, c["recs"])
    n_obj = len(c["recs"])
    assert ctx.patches() == (0, 0)
    ctx.set_lights([0, 1], [1.0, 2.0])
    ctx.set_environment(np.ones((4, 4, 3)))
    ctx.set_media([2], [0.5])
    ctx.set_textures([tor.Texture.constant((0.5, 0.25, 0.125))], [0, -1, 0])
    ctx.set_groups(np.arange(1, n_obj + 1, dtype=np.uint32))
    pts = np.zeros((5, 4))
    ctx.build_photons(np.zeros((3, 3)), np.ones((3, 3)), radius=0.5)
    probe = np.ones((5, 7))
    probe[:, 2] = 490.0

    def others():
        rec = ctx.hit(probe, mask=2)
        return (ctx.light_pdf(pts + 5.0, np.zeros(5, dtype=np.int32)), ctx.environment(np.ones((5, 7))), ctx.march_media(np.ones((5, 7)), 1.0).depth,
                ctx.photons_info(), rec.object, ctx.albedo(ctx.hit(probe)).color, ctx.textures())
    before = others()
    ctx.set_patches(_patches(tor, c["table"]))
    for a, b in zip(before, others()):
        assert a == b if isinstance(a, (dict, tuple)) else np.array_equal(a, b)
    info = ctx.patches()
    assert info == (9, sum(p["material"] >= 0 for p in c["table"])) and not R.mismatches(_np(ctx.hit_patches(c["rays"])), want["hit"])
    # ... and they leave it alone, as an identical upload does
    ctx.set_lights([1])
    ctx.set_environment(np.full((2, 2, 3), 0.5))
    ctx.set_media([0, 1], [0.5, 0.25])
    ctx.set_media_phase([0.3, -0.2])
    ctx.set_media_grid(0, np.ones((2, 2, 2)))
    ctx.set_textures([], np.zeros(n_obj))
    ctx.set_groups(None)
    ctx.build_photons(np.zeros((2, 3)), np.ones((2, 3)), radius=0.25)
    hits_before = ctx.scene_counters()[1]
    ctx.upload(tor.Scene.from_records(c["recs"]).list())
    assert ctx.scene_counters()[1] == hits_before + 1                               # a byte-identical upload: a cache hit
    assert ctx.patches() == info and not R.mismatches(_np(ctx.hit_patches(c["rays"])), want["hit"])
    # clearing, and a replacing upload
    ctx.set_patches([])
    assert ctx.patches() == (0, 0)
    with pytest.raises(tor.TorError, match="no patch table"):
        ctx.hit_patches(c["rays"])
    with pytest.raises(tor.TorError, match="no patch table"):
        ctx.occluded_patches(c["rays"])
    ctx.set_patches(_patches(tor, c["table"]))
    assert ctx.patches() == info
    other = c["recs"].copy()
    other[0, 9] = 1.25
    ctx.upload(tor.Scene.from_records(other).list())
    assert ctx.patches() == (0, 0)
    with pytest.raises(tor.TorError, match="no patch table"):
        ctx.hit_patches(c["rays"])
    with pytest.raises(ValueError, match="needs a patch table"):
        ctx.trace_patches(np.ones((2, 7)), np.ones((2, 4), dtype=np.uint64), 2)
    # a second context has a table of its own
    second = _ctx(tor, c["recs"], c["table"][:2])
    assert second.patches()[0] == 2 and ctx.patches() == (0, 0)


def test_refusals_that_need_a_context(tor):
    """The header's order, provoked with no kernel launch: a later fault is present in every call, the earlier one is what is
    reported, and nothing has changed after each."""
    c, want = I.BY_NAME["soup9"], I.answer("soup9")
    L = tor.lib()
    err = lambda: L.tor_last_error().decode()
    table = tor.pack_patches(_patches(tor, c["table"]))
    tp, n_p = C.addressof(table), len(c["table"])
    n = len(c["rays"])
    raw, patch, occ = np.full((n, 8), 7.0), np.full(n, 77, dtype=np.int32), np.full(n, 77, dtype=np.int32)
    hit = lambda h: L.tor_patch_hit_host(h, n, c["rays"].ctypes.data, None, None, n, 0, raw.ctypes.data, patch.ctypes.data, None, None, 0xFFFFFFFF)
    occluded = lambda h: L.tor_patch_occluded_host(h, n, c["rays"].ctypes.data, None, None, n, 0, occ.ctypes.data, None, 0xFFFFFFFF)
    empty = tor.Context(0)
    assert L.tor_scene_patches(empty._h, -1, None) == -1 and "no scene uploaded" in err()
    assert hit(empty._h) == -1 and "no scene uploaded" in err() and occluded(empty._h) == -1 and "no scene uploaded" in err()
    ctx = _ctx(tor, c["recs"])
    assert hit(ctx._h) == -1 and "no patch table" in err() and occluded(ctx._h) == -1 and "no patch table" in err()
    assert (raw == 7.0).all() and (patch == 77).all() and (occ == 77).all()
    assert L.tor_scene_patches(ctx._h, n_p, tp) == 0
    info = ctx.patches()

    def unchanged():
        assert ctx.patches() == info and not R.mismatches(_np(ctx.hit_patches(c["rays"])), want["hit"])
    unchanged()

    def broken(j, **fields):
        rec = (tor.PatchRecord * n_p)()
        C.memmove(rec, table, 88 * n_p)
        for k, v in fields.items():
            if k in ("q", "u", "v"):
                getattr(rec[j], k)[:] = v
            else:
                setattr(rec[j], k, v)
        return rec
    last = broken(n_p - 1, kind=2)                                                   # the later fault every call carries
    for args, word in (((-1, None), "n_patches"), ((tor.PATCH_MAX + 1, None), "n_patches"), ((n_p, None), "table is NULL")):
        assert L.tor_scene_patches(ctx._h, *args) == -1 and word in err(), (word, err())
        unchanged()
    big = 1e200
    per_record = [(dict(kind=5, material=99, q=(np.nan, 0, 0)), "unknown kind"), (dict(material=3, q=(np.nan, 0, 0)), "material outside"),
                  (dict(material=-2), "material outside"), (dict(q=(0, np.inf, 0), u=(0, 0, 0)), "must be finite"),
                  (dict(v=(0, 0, np.nan), u=(0, 0, 0)), "must be finite"), (dict(u=(big, 0, 0), v=(0, big, 0)), "cross(u, v) is not finite"),
                  (dict(u=(1, 2, 3), v=(2, 4, 6)), "no area"), (dict(u=(0, 0, 0)), "no area"), (dict(u=(1e-170, 0, 0), v=(0, 1e-170, 0)), "no area"),
                  (dict(u=(1e90, 0, 0), v=(0, 1e90, 0)), "overflows")]
    for fields, word in per_record:
        rec = broken(0, **fields)
        rec[n_p - 1].kind = 2
        assert L.tor_scene_patches(ctx._h, n_p, C.addressof(rec)) == -1 and "table[0]" in err() and word in err(), (word, err())
        unchanged()
    assert L.tor_scene_patches(ctx._h, n_p, C.addressof(last)) == -1 and f"table[{n_p - 1}]: unknown kind" in err()
    unchanged()
    with pytest.raises(tor.TorError, match="material outside"):
        ctx.set_patches([tor.Patch.quad((0, 0, 0), (1, 0, 0), (0, 1, 0), material=3)])
    unchanged()
    # the queries: the earlier refusals come first with a table present too
    assert L.tor_patch_hit_host(ctx._h, n, None, None, None, n - 1, 0, None, None, None, None, 0) == -1 and "without a list" in err()
    assert L.tor_patch_hit_host(ctx._h, n, None, None, None, n, 0, None, None, None, None, 0) == -1 and "NULL rays, hits or patch" in err()
    assert L.tor_patch_occluded_host(ctx._h, n, c["rays"].ctypes.data, None, None, n, 0, None, None, 0) == -1 and "NULL rays or occluded" in err()
    assert L.tor_patch_hit_host(ctx._h, 0, None, None, None, 0, 0, None, None, None, None, 0) == 0            # nothing to do
    unchanged()
    assert L.tor_patch_info(ctx._h, None) == -1
