"""Surface-texture queries on the MI355X (tor_scene_textures, tor_texture_info, tor_texture_eval_device / _host): for every case of
tests/texture_inputs.py every bit of colour and texel is the numpy restatement's (tests/texture_restatement.py, which
tests/test_texture_query.py anchors), through device and host entries, tensors and numpy, lists and out=; an unbound object
answers bounce()'s attenuation; trace(textures=True) with constant textures equal to the albedos is trace(); trace and trace_direct
with textures against the restated loops, bit for bit; the lifecycle; the refusals that need a context; the info and the note."""
import ctypes as C

import numpy as np
import pytest
import torch

import bounce_restatement as BR
import phase_inputs as PI
import radiance_restatement as RR
import texture_inputs as I
import texture_restatement as R

pytestmark = pytest.mark.gpu


def _textures(tor, textures):
    out = []
    for t in textures:
        if t["kind"] == R.CONSTANT:
            out.append(tor.Texture.constant(t["a"]))
        elif t["kind"] == R.CHECKER:
            out.append(tor.Texture.checker(t["a"], t["b"], t["freq"], "world" if t["option"] == R.WORLD else "normal"))
        else:
            out.append(tor.Texture.image(t["rgb"], "nearest" if t["option"] == R.NEAREST else "bilinear"))
    return out


def _ctx(tor, recs, textures=None, binding=None):
    ctx = tor.Context(0)
    ctx.upload(tor.Scene.from_records(np.asarray(recs, dtype=np.float64).reshape(-1, 16)).list())
    if textures is not None:
        ctx.set_textures(_textures(tor, textures), binding)
    return ctx


def _cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _np(ev):
    if isinstance(ev.color, torch.Tensor):
        torch.cuda.synchronize()
        return {"color": ev.color.cpu().numpy(), "texel": ev.texel.cpu().numpy()}
    return {"color": ev.color, "texel": ev.texel}


def _eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


@pytest.mark.parametrize("name", I.NAMES)
def test_every_bit_of_every_case(tor, name):
    c, want = I.BY_NAME[name], I.answer(name)
    ctx = _ctx(tor, c["recs"], c["textures"], c["binding"])
    table, atlas = R.pack(c["textures"])
    assert ctx.textures() == (len(table), len(atlas), int((c["binding"] >= 0).sum()))
    n = len(c["hits"])
    hits = _cuda(c["hits"])
    ev = ctx.albedo(hits)
    assert ev.mode == "texture eval" and tor.last_note() == "texture eval"
    bad = R.mismatches(_np(ev), want)
    assert not bad, bad
    host = ctx.albedo(c["hits"])                                                     # the blocking entry on numpy operands
    assert isinstance(host.color, np.ndarray) and not R.mismatches(_np(host), want)
    # two halves through lists, the second into the first's result
    first, rest = np.arange(0, n, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)
    half = ctx.albedo(hits, index=_cuda(first, np.int32))
    both = ctx.albedo(hits, index=_cuda(rest, np.int32), out=half)
    assert both.color.data_ptr() == half.color.data_ptr() and both.texel.data_ptr() == half.texel.data_ptr() and not R.mismatches(_np(both), want)
    hh = ctx.albedo(c["hits"], index=first)
    hb = ctx.albedo(c["hits"], index=rest, out=hh)
    assert hb.color is hh.color and not R.mismatches(_np(hb), want)
    # the C entries themselves, without a texel output (it is nullable)
    L = tor.lib()
    color = np.full((n, 3), 7.0)
    assert L.tor_texture_eval_host(ctx._h, n, c["hits"].ctypes.data, None, n, color.ctypes.data, None) == 0
    assert _eq(color, want["color"])
    dcol = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    assert L.tor_texture_eval_device(ctx._h, n, hits.data_ptr(), None, n, dcol.data_ptr(), None, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert _eq(dcol.cpu().numpy(), want["color"])


@pytest.mark.parametrize("length", [1, 63, 64, 65, 255])
def test_lists_leave_the_other_records_alone(tor, length):
    c, want = I.BY_NAME["wave16"], I.answer("wave16")
    ctx = _ctx(tor, c["recs"], c["textures"], c["binding"])
    n = len(c["hits"])
    index = I.lists()[length]
    listed = index[(index >= 0) & (index < n)]
    rest = np.ones(n, dtype=bool)
    rest[listed] = False
    out = tor.TextureEval(torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda"), torch.full((n,), 77, dtype=torch.int32, device="cuda"), "")
    got = _np(ctx.albedo(_cuda(c["hits"]), index=_cuda(index, np.int32), out=out))
    assert _eq(got["color"][listed], want["color"][listed]) and np.array_equal(got["texel"][listed], want["texel"][listed])
    assert (got["color"][rest] == 7.0).all() and (got["texel"][rest] == 77).all()
    hout = tor.TextureEval(np.full((n, 3), 7.0), np.full(n, 77, dtype=np.int32), "")
    got = _np(ctx.albedo(c["hits"], index=index, out=hout))
    assert _eq(got["color"][listed], want["color"][listed]) and np.array_equal(got["texel"][listed], want["texel"][listed])
    assert (got["color"][rest] == 7.0).all() and (got["texel"][rest] == 77).all()
    empty = ctx.albedo(_cuda(c["hits"]), index=_cuda(np.zeros(0), np.int32), out=out)
    assert empty.mode == "texture_eval: nothing to do"


# ---- an unbound object answers the scatter's attenuation; constant textures equal to the albedos change nothing ------------------------

def _random_frame(tor, nrows=16, ncols=16):
    scene = tor.random_scene()
    ctx = tor.Context(0)
    ctx.upload(scene.list())
    rays, rng = ctx.camera_rays(tor.camera(), nrows, ncols, 0, 1, tor.SEED_SAMPLE)
    return scene, ctx, rays, rng


def test_an_unbound_object_answers_the_attenuation_and_constants_change_nothing(tor):
    scene, ctx, rays, rng = _random_frame(tor)
    recs = scene.to_records()
    n_obj = len(recs)
    ctx.set_textures([tor.Texture.constant((0.5, 0.5, 0.5))], np.full(n_obj, -1))        # a table with NO bindings
    assert ctx.textures() == (1, 0, 0)
    work, st = rays.clone(), rng.clone()
    seen, total = set(), 0
    for _ in range(4):                                                               # four steps: mirrors and glass come into view
        res = ctx.bounce(work, st)
        ev = ctx.albedo(res)
        torch.cuda.synchronize()
        scat = (res.status == tor.BOUNCE_SCATTERED).cpu().numpy()
        assert _eq(ev.color.cpu().numpy()[scat], res.attenuation.cpu().numpy()[scat])
        total += int(scat.sum())
        assert (ev.texel == -1).all()
        seen |= set(recs[res.object.cpu().numpy()[scat], 10].astype(int).tolist())
        work = res.rays
    print("scattered rays compared:", total, "of materials", sorted(seen))
    assert total >= 64 and {0, 1} <= seen                                                            # (the Dielectric's (1, 1, 1): the untextured case)
    want_c, want_s, _ = ctx.trace(rays, rng.clone(), 8)
    got_c, got_s, _ = ctx.trace(rays, rng.clone(), 8, textures=True)
    torch.cuda.synchronize()
    assert torch.equal(got_s, want_s) and _eq(got_c.cpu().numpy(), want_c.cpu().numpy())
    # the bound alternative: one CONSTANT per object, equal to its albedo ((1, 1, 1) for a Dielectric)
    albedo = np.where((recs[:, 10] == 2)[:, None], 1.0, recs[:, 11:14])
    ctx.set_textures([tor.Texture.constant(a) for a in albedo], np.arange(n_obj))
    assert ctx.textures() == (n_obj, 0, n_obj)
    got_c, got_s, _ = ctx.trace(rays, rng.clone(), 8, textures=True)
    torch.cuda.synchronize()
    assert torch.equal(got_s, want_s) and _eq(got_c.cpu().numpy(), want_c.cpu().numpy())
    assert float(want_c.sum()) > 0


# ---- the integrators against the restated loops -----------------------------------------------------------------------------------------

DEPTH = 6
_frame = {}


def _frame_rays(oracle):
    if not _frame:
        cam = oracle.camera(look_from=(0.5, 2.2, 9.0), look_at=(0.2, 0.8, 0.0), vfov=42.0, aspect=1.0)
        _frame["rays"], _frame["st"] = RR.camera_rays(oracle, cam, 10, 10, None, 0, 2)
    return _frame["rays"], _frame["st"]


def test_trace_with_textures_equals_the_restated_loop(tor, oracle):
    recs, textures, binding, emission, _ = I.frame_scene()
    rays, st = _frame_rays(oracle)
    want_c, want_s = R.trace(oracle, recs, textures, binding, rays, st, DEPTH, emission=emission)
    plain_c, _ = BR.trace(oracle, recs, rays, st, DEPTH, emission=emission)
    assert not _eq(want_c, plain_c) and (want_c > 0).any()                           # the textures are in view
    ctx = _ctx(tor, recs, textures, binding)
    color, st_out, _ = ctx.trace(_cuda(rays), _cuda(st.view(np.int64), np.int64), DEPTH, emission=_cuda(emission), textures=True)
    torch.cuda.synchronize()
    assert _eq(color.cpu().numpy(), want_c) and np.array_equal(st_out.cpu().numpy().view(np.uint64), want_s)
    color, st_out, _ = ctx.trace(rays, st, DEPTH, emission=emission, textures=True)  # numpy operands: through the device and back
    assert _eq(color, want_c) and np.array_equal(st_out, want_s)
    color, _, _ = ctx.trace(rays, st, DEPTH, emission=emission)                      # textures=False: the table is not read
    assert _eq(color, plain_c)


def _restated_direct(tor, ctx, case, rays, st, depth, glossy):
    """trace_direct(textures=True, mis=False) restated on the context's own steps and samplers (each held to its restatement by its
    own suite) with the colours of tests/texture_restatement.py: per step bounce the live paths; sky on a miss; emission found after
    a specular vertex; att *= colour for the rays that scattered; a light sample at the diffuse (glossy=: diffuse or glossy)
    vertices, which is att * emitted * cos / pi / pdf on the default path and att_before * colour * p_b * emitted / pdf with
    glossy=."""
    recs, textures, binding, emission, _ = case
    n = len(rays)
    dev = "cuda"
    work, rng = _cuda(rays), _cuda(st.view(np.int64), np.int64)
    lrng = _cuda(PI.derived_states(st).view(np.int64), np.int64)
    emission_t = _cuda(emission)
    diffuse = torch.from_numpy(tor.diffuse_objects(recs)).to(dev)
    nee_ok = diffuse | torch.from_numpy(tor.glossy_objects(recs)).to(dev) if glossy else diffuse
    color = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    att = torch.ones((n, 3), dtype=torch.float64, device=dev)
    specular = torch.ones(n, dtype=torch.bool, device=dev)
    points = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    t_range = torch.empty((n, 2), dtype=torch.float64, device=dev)
    t_range[:, 0], t_range[:, 1] = 0.001, 1.0 - 1e-9
    live = torch.arange(n, dtype=torch.int32, device=dev)
    tr = (float(rays[:, 6].min()), float(rays[:, 6].max()))
    for step in range(depth):
        if live.numel() == 0:
            break
        win = work.clone()
        res = ctx.bounce(work, rng, live, tr)
        idx = live.long()
        status = res.status[idx]
        miss = idx[status == tor.BOUNCE_MISS]
        color[miss] = ctx.sky(work, miss.int())[miss] * att[miss]
        hit = idx[status != tor.BOUNCE_MISS]
        obj = res.object[hit].long()
        color[hit] = color[hit] + att[hit] * emission_t[obj] * specular[hit].to(torch.float64)[:, None]
        torch.cuda.synchronize()
        tex = R.evaluate(recs, textures, binding, res.raw.cpu().numpy(), live.cpu().numpy())
        tcol = _cuda(tex["color"])
        att_before = att.clone()
        scat = idx[status == tor.BOUNCE_SCATTERED]
        att[scat] = att[scat] * tcol[scat]
        specular[scat] = ~nee_ok[res.object[scat].long()]
        nee = hit[nee_ok[obj]] if glossy else scat[diffuse[res.object[scat].long()]]
        live = scat.int()
        if nee.numel() == 0 or step == depth - 1:
            continue
        points[nee, 0:3], points[nee, 3] = res.p[nee], win[nee, 6]
        ls = ctx.sample_lights(points, lrng, nee.int())
        occ = ctx.occluded(ls.rays, t_range, nee.int(), tr)
        pdf, lamp = ls.pdf[nee], ls.light[nee].long()
        emitted = emission_t[lamp.clamp(min=0)]
        free = (~occ.occluded[nee]) & (lamp >= 0) & (pdf > 0) & torch.isfinite(pdf)
        if glossy:
            ev = ctx.bsdf(win, res, ls.rays, nee.int())
            p_b = ev.pdf[nee]
            ok = free & (p_b > 0) & torch.isfinite(p_b)
            add = att_before[nee] * (tcol[nee] * p_b[:, None]) * emitted * (torch.ones_like(pdf) / pdf)[:, None]
        else:
            sd = ls.rays[nee, 3:6]
            cos_l = (res.normal[nee] * sd).sum(1) / torch.sqrt((sd * sd).sum(1))
            ok = free & (cos_l > 0)
            add = att[nee] * emitted * (cos_l / np.pi / pdf * torch.ones_like(pdf))[:, None]
        color[nee] = color[nee] + torch.where(ok[:, None], add, torch.zeros_like(add))
    torch.cuda.synchronize()
    return color.cpu().numpy(), rng.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("glossy", [False, True], ids=["default", "glossy"])
def test_trace_direct_with_textures_equals_the_restated_loop(tor, oracle, glossy):
    case = I.frame_scene()
    recs, textures, binding, emission, lights = case
    rays, st = _frame_rays(oracle)
    ctx = _ctx(tor, recs, textures, binding)
    ctx.set_lights(lights)
    want_c, want_s = _restated_direct(tor, ctx, case, rays, st, DEPTH, glossy)
    kw = dict(glossy=tor.glossy_objects(recs)) if glossy else {}
    color, st_out, _ = ctx.trace_direct(_cuda(rays), _cuda(st.view(np.int64), np.int64), emission, tor.diffuse_objects(recs), DEPTH,
                                        textures=True, **kw)
    torch.cuda.synchronize()
    assert _eq(color.cpu().numpy(), want_c) and np.array_equal(st_out.cpu().numpy().view(np.uint64), want_s)
    plain, _, _ = ctx.trace_direct(_cuda(rays), _cuda(st.view(np.int64), np.int64), emission, tor.diffuse_objects(recs), DEPTH, **kw)
    torch.cuda.synchronize()
    assert not _eq(plain.cpu().numpy(), want_c) and (want_c > 0).any() and np.isfinite(want_c).all()


# ---- the lifecycle, the refusals, the info --------------------------------------------------------------------------------------------

def test_lifecycle(tor):
    c, want = I.BY_NAME["wave16"], I.answer("wave16")
    ctx = _ctx(tor, c["recs"])
    n_obj = len(c["recs"])
    assert ctx.textures() == (0, 0, 0)
    # the other tables first: the texture table leaves them alone
    ctx.set_lights([0, 1], [1.0, 2.0])
    ctx.set_environment(np.ones((4, 4, 3)))
    ctx.set_media([2], [0.5])
    ctx.set_groups(np.arange(1, n_obj + 1, dtype=np.uint32))
    pts = np.zeros((5, 4))
    ctx.build_photons(np.zeros((3, 3)), np.ones((3, 3)), radius=0.5)
    before = (ctx.light_pdf(pts + 5.0, np.zeros(5, dtype=np.int32)), ctx.environment(np.ones((5, 7))), ctx.march_media(np.ones((5, 7)), 1.0).depth,
              ctx.photons_info(), ctx.hit(np.ones((5, 7)), mask=2).object)
    ctx.set_textures(_textures(tor, c["textures"]), c["binding"])
    after = (ctx.light_pdf(pts + 5.0, np.zeros(5, dtype=np.int32)), ctx.environment(np.ones((5, 7))), ctx.march_media(np.ones((5, 7)), 1.0).depth,
             ctx.photons_info(), ctx.hit(np.ones((5, 7)), mask=2).object)
    for a, b in zip(before, after):
        assert a == b if isinstance(a, dict) else np.array_equal(a, b)
    info = ctx.textures()
    assert info == (5, 50, 5) and not R.mismatches(_np(ctx.albedo(c["hits"])), want)
    # ... and they leave it alone, as an identical upload does
    ctx.set_lights([1])
    ctx.set_environment(np.full((2, 2, 3), 0.5))
    ctx.set_media([0, 1], [0.5, 0.25])
    ctx.set_media_phase([0.3, -0.2])
    ctx.set_media_grid(0, np.ones((2, 2, 2)))
    ctx.set_groups(None)
    ctx.build_photons(np.zeros((2, 3)), np.ones((2, 3)), radius=0.25)
    hits_before = ctx.scene_counters()[1]
    ctx.upload(tor.Scene.from_records(c["recs"]).list())
    assert ctx.scene_counters()[1] == hits_before + 1                                # a byte-identical upload: a cache hit
    assert ctx.textures() == info and not R.mismatches(_np(ctx.albedo(c["hits"])), want)
    # clearing, and a replacing upload
    ctx.set_textures([], np.zeros(n_obj))
    assert ctx.textures() == (0, 0, 0)
    with pytest.raises(tor.TorError, match="no texture table"):
        ctx.albedo(c["hits"])
    ctx.set_textures(_textures(tor, c["textures"]), c["binding"])
    other = c["recs"].copy()
    other[0, 9] = 1.25
    ctx.upload(tor.Scene.from_records(other).list())
    assert ctx.textures() == (0, 0, 0)
    with pytest.raises(tor.TorError, match="no texture table"):
        ctx.albedo(c["hits"])
    with pytest.raises(ValueError, match="textures=True needs a texture table"):
        ctx.trace(np.ones((2, 7)), np.ones((2, 4), dtype=np.uint64), 2, textures=True)


def test_refusals_that_need_a_context(tor):
    c, want = I.BY_NAME["two_images"], I.answer("two_images")
    L = tor.lib()
    err = lambda: L.tor_last_error().decode()
    table, atlas = tor.pack_textures(_textures(tor, c["textures"]))
    binding = np.ascontiguousarray(c["binding"], dtype=np.int32)
    n_obj, n_tex, n_texels = len(binding), 2, len(atlas)
    tp, bp, ap = C.addressof(table), binding.ctypes.data, atlas.ctypes.data
    empty = tor.Context(0)
    assert L.tor_scene_textures(empty._h, n_tex, tp, n_obj, bp, n_texels, ap) == -1 and "no scene uploaded" in err()
    color = np.zeros((2, 3))
    assert L.tor_texture_eval_host(empty._h, 2, c["hits"].ctypes.data, None, 2, color.ctypes.data, None) == -1 and "no scene uploaded" in err()
    ctx = _ctx(tor, c["recs"])
    assert L.tor_texture_eval_host(ctx._h, 2, c["hits"].ctypes.data, None, 2, color.ctypes.data, None) == -1 and "no texture table" in err()
    assert (color == 0).all()
    assert L.tor_scene_textures(ctx._h, n_tex, tp, n_obj, bp, n_texels, ap) == 0

    def unchanged():
        assert ctx.textures() == (2, 25, 3) and not R.mismatches(_np(ctx.albedo(c["hits"])), want)
    unchanged()
    # the header's order: a later fault is present in every call, and the earlier one is what is reported
    nan_atlas = atlas.copy()
    nan_atlas[3, 1] = np.nan
    bad_bind = binding.copy()
    bad_bind[1] = 2
    past = (tor.TextureRecord * 2)()
    C.memmove(past, table, 192)
    past[1].offset = 17                                                              # 17 + 9 > 25
    np_ = nan_atlas.ctypes.data
    steps = [((-1, C.addressof(past), n_obj + 1, None, -1, None), "n_textures"),
             ((tor.TEXTURE_MAX + 1, C.addressof(past), n_obj + 1, None, -1, None), "n_textures"),
             ((n_tex, C.addressof(past), n_obj + 1, None, -1, None), "n_objects must be"),
             ((n_tex, C.addressof(past), n_obj, None, tor.TEXTURE_MAX_TEXELS + 1, None), "n_texels"),
             ((n_tex, None, n_obj, bad_bind.ctypes.data, n_texels, None), "table or binding is NULL"),
             ((n_tex, C.addressof(past), n_obj, None, n_texels, None), "table or binding is NULL"),
             ((n_tex, C.addressof(past), n_obj, bad_bind.ctypes.data, n_texels, None), "texels is NULL"),
             ((n_tex, C.addressof(past), n_obj, bad_bind.ctypes.data, n_texels, np_), "table[1]: the image does not lie inside the atlas"),
             ((n_tex, tp, n_obj, bad_bind.ctypes.data, n_texels, np_), "binding[1] is outside"),
             ((n_tex, tp, n_obj, bp, n_texels, np_), "texels must be finite")]
    for args, word in steps:
        assert L.tor_scene_textures(ctx._h, *args) == -1 and word in err(), (word, err())
        unchanged()
    for field, value, word in (("kind", 3, "unknown kind"), ("option", 2, "unknown option"), ("side", 0, "side outside"), ("side", 2049, "side outside"),
                               ("offset", -1, "inside the atlas")):
        rec = (tor.TextureRecord * 2)()
        C.memmove(rec, table, 192)
        setattr(rec[0], field, value)
        assert L.tor_scene_textures(ctx._h, n_tex, C.addressof(rec), n_obj, bp, n_texels, ap) == -1 and "table[0]" in err() and word in err(), word
        unchanged()
    for t in (tor.Texture.constant((0.5, -0.0, -1.0)), tor.Texture.constant((np.inf, 0, 0)), tor.Texture.checker((1, 1, 1), (0, np.nan, 0), 1.0),
              tor.Texture.checker((1, 1, 1), (0, 0, 0), (1.0, np.inf, 1.0))):
        with pytest.raises(tor.TorError, match="colours must be finite|freq must be finite"):
            ctx.set_textures([t], np.zeros(n_obj))
        unchanged()
    with pytest.raises(tor.TorError, match="n_objects must be"):
        ctx.set_textures(_textures(tor, c["textures"]), [0, 1])
    unchanged()
    ctx.set_textures([tor.Texture.constant((0.5, -0.0, 0.0)), tor.Texture.checker((1, 1, 1), (0, 0, 0), (-1.0, 0.0, 1e300))], [0, 1, -1])
    assert ctx.textures() == (2, 0, 2)
