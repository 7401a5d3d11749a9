"""One long-lived context per script on the MI355X (tests/context_scripts.py): uploads, tables, queries of every family, renders and
two open accumulations interleaved on one stream, with no host synchronisation between the steps other than what the library and
its Python layer force themselves: a numpy operand (the blocking _host twins), a refusal, a replacing upload (tor_scene_upload
waits for the device before it overwrites the scene), a block query on device tensors with time_range=None, whose range the
Python layer reads back from the tensor's times (torch.aminmax, a download), and build_photons on device tensors, which reads the
largest power back for its scale.  The test adds none: every device operand is uploaded
before the first step, every device output is kept and downloaded after the last.

Arbiter: every answer is compared bit for bit with the family's restatement under the MODEL's state (context_scripts.Model: which
records, words, table and map the step must see), NaNs as the families' own tests compare them (a NaN on both sides of a float
field is equal, every other bit counts); renders and the accumulations with oracle.render / oracle.accumulate (PORTABLE math), the
film with deposit_restatement; PhotonGather.irradiance alone to 2^-50 (its docstring leaves the order of four roundings open; a
scale that is a power of two off shows at any tolerance).  No fresh context answers for another.  What ran (res.mode / tor.last_note()) is asserted where the
per-family tests fix it: `brute` is the brute force, odd_objects falls back and says why, the media queries name the model's count
of media ("media march: 4 media"), a build the restatement's bucket count and scale, a grid march the model's medium and its
grid's dimensions ("media grid march: medium 1, 2x3x7"), the patch steps "patch hit" / "patch occluded", a texture step "texture
eval".  At the end ctx.scene_counters()[:2] is the model's count of uploads and cache hits, and ctx.patches(), ctx.textures() and
ctx.media_grids() say what the model's final state says.  tests/test_context_scripts.py shows on the CPU that a
stale cache behind any of the steps would change a quarter of its rows; profiles/context_script_mutants.txt what the same_size
script fails on when a cache key is broken.

test_script_on_a_stream_of_its_own runs the two cheapest scripts once more inside one torch.cuda.Stream(): the scripts above run on
torch's default stream, the legacy one, with which every blocking hipMemcpy of a setter serialises by itself, so a setter that
forgot to wait for the context's last query could not show there.

Measured wall time on an MI355X, restatements and oracle renders included, this module and its parent commit's in one visit.  The
parent (before the photon, media and phase steps): 15.9 s for 5 tests, 13.5 s in the tests themselves -- same_size (290 steps)
6.0 s, same_size_g9 (290) 0.36 s, sizes (384) 6.7 s, seeded_1 (123) 0.35 s, seeded_2 (123) 0.12 s: 11.2 ms per step.  This module:
17.1 s for 7 tests, 15.3 s in the tests -- same_size (435 steps) 6.0 s, same_size_g9 (435) 0.68 s, sizes (561) 6.8 s, seeded_1 (123)
0.36 s, seeded_2 (123) 0.36 s, and on a stream of its own same_size_g9 0.64 s, seeded_2 0.37 s: 6.8 ms per step over 2235 steps.
The cost per step fell: nearly all of the time is the restatements of bounce, scatter and radiance on the 724 and 1300 objects of
same_size and sizes (they loop in Python), and the new steps' restatements see four media or a few thousand photons; the
library's share of a script is tens of milliseconds.

With the grid, texture and patch steps, again this module and its parent commit's in one visit.  The parent: 17.2 s for 7 tests,
15.1 s in the tests -- same_size (435 steps) 5.74 s, same_size_g9 (435) 0.67 s, sizes (561) 6.98 s, seeded_1 (123) 0.37 s, seeded_2
(123) 0.36 s, on a stream of its own same_size_g9 0.64 s, seeded_2 0.36 s: 6.8 ms per step over 2235 steps.  This module: 21.4 s
for 7 tests, 19.3 s in the tests -- same_size (654 steps) 7.32 s, same_size_g9 (654) 0.83 s, sizes (842) 8.00 s, seeded_1 (153)
0.49 s, seeded_2 (153) 0.91 s, on a stream of its own same_size_g9 0.83 s, seeded_2 0.90 s: 5.9 ms per step over 3263 steps (one
step was added to the same_size scripts afterwards: 655 steps, 7.32 s and 0.82 s in a later visit).  The new steps cost their
Python restatements -- the grid march and lookup loop per ray at 64 rows and at most 257 points on grids of at most 7 cells per
axis, albedo loops per record, the patch restatement walks 65 patches over all rays at once --; the library's share stays
milliseconds."""
import numpy as np
import pytest
import torch

import context_scripts as S
import deposit_restatement as D
import patch_restatement as PT
import render_regimes as R
import texture_restatement as TR

pytestmark = pytest.mark.gpu
_scenes = {}


def _scene(tor, name, bad=False):
    """The Scene of a named list, built once and kept alive (the library keeps a byte copy, the test keeps the caller's); `bad`: the
    same list with an unknown kind in its middle."""
    key = (name, bad)
    if key not in _scenes:
        sc = tor.Scene.from_records(np.asarray(S.records(name)))
        if bad:
            sc.objects[len(sc) // 2].kind = 7
        _scenes[key] = sc
    return _scenes[key]


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _host(t):
    """A kept output as numpy (after the last step): 64-bit and 32-bit integers by their bits, as the restatements hold them."""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _records_as_fields(outs):
    """Keys that end in `raw` hold TorHit records: their fields, as context_scripts.answer names them."""
    done = {}
    for k, v in outs.items():
        if k.endswith("raw"):
            done.update(S._hit_fields(_host(v), k[:-3]))
        else:
            done[k] = _host(v)
    return done


def _call(tor, ctx, step, op, env):
    """One query, render or pass: returns (the kept outputs, what ran or None).  `op(name)`: the operand as the step wants it -- a
    device tensor uploaded before the script began, or the numpy array itself (the blocking twin)."""
    f, b = step["family"], S.base(step["family"])
    mask = {"mask": op("masks")} if f in S.MASKED else {}
    tr, mode = step.get("time_range"), step.get("mode")
    if b == "hit":
        res = ctx.hit(op("rays"), op("t_range"), tr, mode, **mask)
        return {"raw": res.raw}, res.mode
    if b == "occluded":
        res = ctx.occluded(op("rays"), op("t_range"), None, tr, mode, **mask)
        return {"occluded": res.raw}, res.mode
    if b == "crossings":
        res = ctx.crossings(op("rays"), step["k"], op("t_range"), None, tr, mode, mask.get("mask"), bool(step.get("records")))
        out = {"t": res.t, "object": res.object, "which": res.which, "count": res.count}
        if step.get("records"):
            out["hits_raw"] = res.hits
        return out, res.mode
    if b == "nearest":
        res = ctx.nearest(op("points"), step["k"], op("dmax"), None, tr, mode, mask.get("mask"))
        return {"distance": res.distance, "object": res.object, "inside": res.inside, "count": res.count}, res.mode
    if b == "bounce":
        res = ctx.bounce(op("rays"), op("states"), None, tr, mode, **mask)
        return {"raw": res.raw, "status": res.status, "attenuation": res.attenuation, "rays": res.rays, "states": res.rng}, res.mode
    if f == "scatter":
        res = ctx.scatter(op("rays"), op("hits"), op("states"))
        return {"status": res.status, "attenuation": res.attenuation, "rays": res.rays, "states": res.rng}, None
    if f == "radiance":
        color, rng, ran = ctx.radiance(op("rays"), op("states"), S.RADIANCE_DEPTH, tr, mode)
        return {"color": color, "states": rng}, ran
    if f == "bsdf":
        ev = ctx.bsdf(op("rays_in"), op("hits"), op("rays_out"))
        return {"value": ev.value, "pdf": ev.pdf, "kind": ev.kind}, None
    if f == "sample_lights":
        ls = ctx.sample_lights(op("points"), op("states"))
        return {"rays": ls.rays, "pdf": ls.pdf, "light": ls.light, "dist": ls.dist, "states": ls.rng}, None
    if f == "light_pdf":
        return {"pdf": ctx.light_pdf(op("points"), op("objects"))}, None
    if f == "emit_lights":
        em = ctx.emit_lights(op("states"), step["shutter"])
        return {"rays": em.rays, "normal": em.normal, "light": em.light, "pdf": em.pdf, "states": em.rng}, None
    if f == "connect_camera":
        import camera_inputs as CI
        cc = ctx.connect_camera(CI.camera_struct(tor, env["x"]["cam24"]), *env["x"]["frame"], op("points"), op("states"))
        return {"rays": cc.rays, "pixel": cc.pixel, "factor": cc.factor, "lens": cc.lens, "states": cc.rng}, None
    if f == "environment":
        ev = ctx.environment(op("rays"), pdf=True)
        return {"color": ev.color, "pdf": ev.pdf, "texel": ev.texel}, None
    if f == "sample_environment":
        es = ctx.sample_environment(op("points"), op("states"))
        return {"rays": es.rays, "pdf": es.pdf, "texel": es.texel, "color": es.color, "states": es.rng}, None
    if f == "deposit":
        env["film"].deposit(env["dev"]["pixels"], env["dev"]["colors"])
        return {}, None
    if f in S.MEDIA_FAMILIES:                             # the note names the table's count: the model's
        note = f"{len(S.MEDIA[env['state'].media or 'A'][0])} media"   # (without a table the call is refused before any note)
        if f == "march_media":
            res = ctx.march_media(op("rays"), op("tau"))
            assert res.mode == note, (step, res.mode)
            return {"status": res.status, "t": res.t, "depth": res.depth, "rho": res.rho, "active": res.active}, None
        if f == "phase":
            res = ctx.phase(op("rays_in"), op("active"), op("rays_out"))
            assert res.mode == note, (step, res.mode)
            return {"value": res.value, "pdf": res.pdf}, None
        res = (ctx.scatter_media if f == "scatter_media" else ctx.sample_phase)(op("rays"), (op("t"), op("active")), op("states"))
        assert res.mode == note, (step, res.mode)
        out = {"rays": res.rays, "attenuation": res.attenuation, "states": res.rng}
        if f == "sample_phase":
            out["pdf"] = res.pdf
        return out, None
    if f == "uniform":
        res = ctx.uniform(op("states"), step["draws"])
        assert res.mode == f"{step['draws']} draw" + ("s" if step["draws"] > 1 else ""), (step, res.mode)
        return {"u": res.u, "states": res.rng}, None
    if f == "gather_photons":
        res = ctx.gather_photons(op("points"), op("normals"), op("radius"), None, step["kernel"], 1.0)
        assert res.note == "photons gather", (step, res.note)
        return {"sums": res.sums, "count": res.count, "irradiance": res.irradiance(S.PATHS)}, None
    if f in S.GRID_FAMILIES:                              # the note names the model's medium and its grid's dimensions
        state = env["state"]
        m = S.medium_of(state.media, step["who"]) if state.media else 0
        dims = "x".join(str(v) for v in S.GRIDS[state.grids[m]][0]) if m in state.grids else None   # (else the call is refused)
        if f == "march_media_grid":
            res = ctx.march_media_grid(op("rays"), op("tau"), m)
            assert res.mode == f"medium {m}, {dims}" and tor.last_note() == f"media grid march: medium {m}, {dims}", (step, res.mode, tor.last_note())
            return {"status": res.status, "t": res.t, "depth": res.depth, "rho": res.rho, "active": res.active, "cell": res.cell}, None
        cell, value = ctx.media_density(op("points"), m)
        assert tor.last_note() == f"media grid density: medium {m}, {dims}", (step, tor.last_note())
        return {"cell": cell, "density": value}, None
    if f == "albedo":
        ev = ctx.albedo(op("hits"))
        assert tor.last_note() == "texture eval", (step, tor.last_note())
        return {"color": ev.color, "texel": ev.texel}, None
    if f in S.PATCH_FAMILIES:
        mask = S.patch_mask(step, {"masks": op("masks")})
        if f == "occluded_patches":                       # merged: into occluded()'s bits (the brute force: it keys no bounds)
            start = ctx.occluded(op("rays"), op("t_range"), None, (0.0, 1.0), "brute") if step.get("merge") else None
            res = ctx.occluded_patches(op("rays"), op("t_range"), mask=mask, merge=start)
            assert tor.last_note() == "patch occluded", (step, tor.last_note())
            return {"occluded": res.raw}, None
        start = ctx.hit(op("rays"), op("t_range"), (0.0, 1.0), "brute") if f == "hit_patches_merged" else None
        res = ctx.hit_patches(op("rays"), op("t_range"), mask=mask, merge=start)
        assert tor.last_note() == "patch hit", (step, tor.last_note())
        return {"raw": res.raw, "patch": res.patch, "uv": res.uv}, None
    cam = tor.camera(**env["x"]["camera"])
    stream = torch.cuda.current_stream().cuda_stream
    if f == "render":
        buf = torch.zeros((R.H, R.W, 3), dtype=torch.float64, device="cuda")
        ctx.render_device(cam, R.H, R.W, R.SPP, 2.2, R.DEPTH, tor.make_options(seeding=step["seeding"], accel=step["accel"]),
                          buf.data_ptr(), stream)
        return {"pixels": buf.view(-1, 3)}, None
    if f not in env["open"]:                              # an accumulation is opened at its first pass and stays open
        make = tor.Progressive if f == "progressive" else tor.PixelProgressive
        seeding = tor.SEED_SAMPLE if f == "progressive" else tor.SEED_PIXEL
        env["open"][f] = make(ctx, cam, R.H, R.W, R.DEPTH, tor.make_options(seeding=seeding, accel=3))
    assert env["open"][f].samples == step["first"]
    env["open"][f].add(3)
    return {}, None


def _set_media(ctx, step, state):
    if state.scene is None:                               # refused before the table is looked at
        return ctx.set_media([S.MOVED], [1.0])
    if step["table"] is None:
        return ctx.set_media([], [])
    return ctx.set_media(*S.media_table(step["table"], state.scene, step.get("bad")))


def _set_media_phase(ctx, step, state):
    if step["g"] is None:
        return ctx.set_media_phase(None)
    g = S.g_vector(step["g"], len(S.MEDIA[state.media][0]) if state.media else 4)
    return ctx.set_media_phase(g[:-1] if step.get("wrong_count") else g)


def _set_media_grid(ctx, step, state):
    """The medium the step's role names under the model's table (0 where the call is refused before the medium is looked at)."""
    m = S.medium_of(state.media, step["who"]) if state.media else 0
    if step["grid"] is None:
        return ctx.set_media_grid(m, None)
    objects = S.media_table(state.media, state.scene)[0] if state.media else None
    inside = objects is not None and 0 <= m < len(objects)
    box = S.grid_box(step["grid"], state.scene, int(objects[m])) if inside else None
    return ctx.set_media_grid(m, S.grid_density(step["grid"]), box)


def _textures(tor, textures):
    out = []
    for t in textures:
        if t["kind"] == TR.CONSTANT:
            out.append(tor.Texture.constant(t["a"]))
        elif t["kind"] == TR.CHECKER:
            out.append(tor.Texture.checker(t["a"], t["b"], t["freq"], "world" if t["option"] == TR.WORLD else "normal"))
        else:
            out.append(tor.Texture.image(t["rgb"], "nearest" if t["option"] == TR.NEAREST else "bilinear"))
    return out


def _set_textures(tor, ctx, step, state):
    if state.scene is None:                               # refused before the table is looked at
        return ctx.set_textures([tor.Texture.constant((0.5, 0.5, 0.5))], [0])
    if step["table"] is None:
        return ctx.set_textures([], np.zeros(len(S.records(state.scene))))
    tex, binding = S.texture_table(step["table"], state.scene, step.get("bad"))
    if step.get("count_of"):                              # the binding built for another list
        binding = S.texture_table(step["table"], step["count_of"])[1]
    return ctx.set_textures(_textures(tor, tex), binding)


def _set_patches(tor, ctx, step, state):
    if state.scene is None:                               # refused before the table is looked at
        return ctx.set_patches([tor.Patch.quad((0, 0, 0), (1, 0, 0), (0, 1, 0))])
    if step["table"] is None:
        return ctx.set_patches([])
    table = S.patch_table(step["table"], state.scene, step.get("bad"), step.get("of"))
    return ctx.set_patches([tor.Patch(p["kind"], p["q"], p["u"], p["v"], p["material"], p["groups"]) for p in table])


def _build_photons(ctx, step, dev_maps):
    """From numpy (the blocking twin) or from tensors that were uploaded before the script began; the Python layer's scale and the
    note are the restatement's."""
    m = S.photon_map(step["map"], step["listed"])
    src = m if step["host"] else dev_maps[(step["map"], step["listed"])]
    built = ctx.build_photons(src["position"], src["power"], src["direction"], radius=m["radius"], index=src["index"])
    assert built.scale == m["scale"] and built.radius == m["radius"], (step, built.scale, m["scale"])
    assert built.note == f"photons build: {m['stored']['n_buckets']} buckets", (step, built.note)


def _check_what_ran(tor, step, state, ran, model_range):
    f = step["family"]
    if not S.takes_mode(f) or ran is None:
        return
    if step["mode"] == "brute":
        assert ran == "brute force", (step, ran)
    elif state.scene == "odd_objects":                   # radii for which the boxes' margin holds for no origin: the blocks fall back
        assert ran.startswith("brute force ("), (step, ran)
        if S.base(f) != "nearest" and model_range == (0.0, 1.0):
            assert ran == f"brute force ({S.WHY_RADII})", (step, ran)
    elif S.has_blocks(state.scene):                      # dense, dense2, tiny, noground and the edited copy: the blocks run, in every
        # range (a silent fallback would take `bnd` and `grp` out of the script); nearest's `auto` may choose the brute force, and says so
        auto_nearest = S.base(f) == "nearest" and step["mode"] == "auto" and ran.startswith("brute force (auto: ")
        assert ran == "blocks" or auto_nearest, (step, state.key(), ran)
    else:                                                # nine objects: no culling layout
        assert ran.startswith("brute force ("), (step, state.key(), ran)


def _run(tor, oracle, name):
    steps = S.script(name)
    model = S.Model()
    expects = model.replay(steps, oracle)
    asks = [e.step["op"] in ("query", "render", "pass") for e in expects]
    xs = [S.inputs(oracle, e.step, e.state) if a else None for e, a in zip(expects, asks)]
    devs = [{k: _dev(v) for k, v in x.items() if isinstance(v, np.ndarray)} if x is not None else None for x in xs]
    dev_maps = {(st["map"], st["listed"]): None for st in steps if st["op"] == "build_photons" and not st["host"]}
    for key in dev_maps:
        m = S.photon_map(*key)
        dev_maps[key] = {k: None if m[k] is None else _dev(m[k]) for k in ("position", "power", "direction", "index")}
    torch.cuda.synchronize()                              # the operands are on the device; from here on nothing waits

    ctx = tor.Context(0)
    env = {"open": {}, "film": tor.Film(ctx, *S.FILM, moments=True, counts=True)}
    kept, ranges = {}, {}
    try:
        for i, e in enumerate(expects):
            step, op = e.step, e.step["op"]
            call = None
            if op == "upload":
                call = lambda: ctx.upload(_scene(tor, step["scene"], bool(step.get("bad"))).list())
            elif op == "set_groups":
                n = len(S.records(e.state.scene))
                call = lambda: ctx.set_groups(S.words(step["words"], n))
            elif op == "set_lights":
                call = lambda: ctx.set_lights(*S.light_table(step["table"])) if step["table"] else ctx.set_lights([])
            elif op == "set_environment":
                call = lambda: ctx.set_environment(*S.env_map(step["map"])[:2]) if step["map"] else ctx.set_environment(None)
            elif op == "set_media":
                call = lambda: _set_media(ctx, step, e.state)
            elif op == "set_media_phase":
                call = lambda: _set_media_phase(ctx, step, e.state)
            elif op == "build_photons":
                call = lambda: _build_photons(ctx, step, dev_maps)
            elif op == "set_media_grid":
                call = lambda: _set_media_grid(ctx, step, e.state)
            elif op == "set_textures":
                call = lambda: _set_textures(tor, ctx, step, e.state)
            elif op == "set_patches":
                call = lambda: _set_patches(tor, ctx, step, e.state)
            else:
                host = bool(step.get("host")) and step["family"] != "deposit" and op == "query"
                env["x"], env["dev"], env["state"] = xs[i], devs[i], e.state
                operand = lambda k: (xs[i].get(k) if host else devs[i].get(k))
                call = lambda: _call(tor, ctx, step, operand, env)
            where = f"{name}: step {i} {step} under {e.state.key()}"
            try:
                got = call()
            except tor.TorError as err:
                assert e.refuse is not None, f"{where} raised {err}"
                assert err.code == e.refuse[0] and e.refuse[1] in str(err), f"{where} was refused with {err}"
                continue
            assert e.refuse is None, f"{where} was not refused {e.refuse}"
            if asks[i]:
                kept[i] = got[0]
                times = xs[i].get("points", xs[i].get("rays"))[:, -1] if S.takes_mode(step["family"]) else None
                _check_what_ran(tor, step, e.state, got[1], S.Model().effective_range(step, times) if times is not None else None)
        assert tuple(ctx.scene_counters()[:2]) == (model.n_uploads, model.n_cache_hits)
        last = model.state                                # the three tables say what the model's final state says
        table = S.patch_table(last.patches, last.scene) if last.patches else []
        assert ctx.patches() == (len(table), sum(p["material"] >= 0 for p in table)), (name, ctx.patches(), last.key())
        tex, binding = S.texture_table(last.textures, last.scene) if last.textures else ([], np.zeros(0))
        texels = sum(t["rgb"].shape[0] ** 2 for t in tex if t["rgb"] is not None)
        assert ctx.textures() == (len(tex), texels, int((binding >= 0).sum())), (name, ctx.textures(), last.key())
        assert ctx.media_grids() == sorted(last.grids), (name, ctx.media_grids(), last.key())
        torch.cuda.synchronize()

        bad = []
        film, sums = D.deposit(np.zeros((0, 3)), np.zeros(0, dtype=np.int32), S.FILM[0] * S.FILM[1]), np.zeros((R.H * R.W, 3))
        for i, e in enumerate(expects):
            if i not in kept:
                continue
            want = S.answer(oracle, e.step, xs[i], e.state)
            f = e.step["family"]
            if f == "deposit":                            # the film stays open: every deposit so far, in any order
                film = D.deposit(xs[i]["colors"], xs[i]["pixels"], S.FILM[0] * S.FILM[1], 1.0, None, film)
                continue
            if f == "progressive":
                sums = sums + want["sums"]               # (multiples of 2^-36 far below 2^17: the sum is exact)
                continue
            if f == "pixel_progressive":
                last_canvas = want["pixels"]
                continue
            got = _records_as_fields(kept[i])
            if "irradiance" in want:                      # four roundings in an order the docstring leaves open: 2^-50, zeros exact
                wi, gi = want.pop("irradiance"), got.pop("irradiance")
                if not ((gi == wi) | (np.abs(gi - wi) <= 2.0 ** -50 * np.abs(wi))).all():
                    bad.append((i, f, "the irradiance is not sums / scale x the kernel's normalisation", e.step, e.state.key()))
            rows = S.differing_rows(want, {k: got[k].reshape(np.asarray(want[k]).shape) for k in want})
            if rows.any():
                bad.append((i, f, f"{int(rows.sum())} of {rows.size} rows", {k: v for k, v in e.step.items() if k != "op"}, e.state.key()))
        fl = env["film"]
        got_film = {"sums": _host(fl.sums).reshape(-1, 3), "moments": _host(fl.moments).reshape(-1, 3), "counts": _host(fl.counts).reshape(-1),
                    "rejected": int(fl.rejected())}
        if D.mismatches(got_film, film):
            bad.append(("film", D.mismatches(got_film, film)))
        pg, pp = env["open"]["progressive"], env["open"]["pixel_progressive"]
        assert pg.samples == pp.samples == 6
        if S.differing_rows({"sums": sums}, {"sums": _host(pg.sums).reshape(-1, 3)}).any():
            bad.append(("progressive", "the sums of the two passes are not the oracle's"))
        if S.differing_rows({"pixels": last_canvas}, {"pixels": _host(pp.image(2.2)).reshape(-1, 3)}).any():
            bad.append(("pixel_progressive", "the canvas after two passes is not the oracle's"))
        assert not bad, f"{name}: {len(bad)} steps differ from their restatements: {[b[:3] for b in bad]}; the first in full: {bad[:4]}"
    finally:
        ctx.close()


@pytest.mark.parametrize("name", S.SCRIPTS)
def test_script_against_the_restatements(tor, oracle, name):
    import time
    t = time.perf_counter()
    _run(tor, oracle, name)
    print(f"{name}: {len(S.script(name))} steps, {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("name", ("same_size_g9", "seeded_2"))
def test_script_on_a_stream_of_its_own(tor, oracle, name):
    """The two cheapest scripts once more, the whole script inside one non-default stream (the library's rule: one stream per
    context).  On torch's default stream -- the legacy one -- every blocking copy of a setter waits for the queued work by itself; a
    stream made by torch.cuda.Stream() does not block against it, so a setter that forgot to wait for the context's last query would
    overwrite a table under a running kernel here.  The expectations are the same."""
    import time
    t = time.perf_counter()
    with torch.cuda.stream(torch.cuda.Stream()):
        _run(tor, oracle, name)
    print(f"{name} on a stream of its own: {len(S.script(name))} steps, {time.perf_counter() - t:.2f} s")
