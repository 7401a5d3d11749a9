"""The host integrators of Context: trace, trace_direct, trace_light, trace_photons, trace_photon_map, trace_environment,
trace_media and trace_media_direct -- wavefront loops over the path-step queries (bounce, bounce_select, sky, occluded, the samplers).  What the loops
share is written once here: the entry and exit for numpy and torch operands, the step's head and tail (_Paths), the sky on a miss,
the Lambertian next-event bookkeeping (_LambertianNee) and the conversion of the per-object operands.  Each integrator keeps a body
of its own for what is its own.  The package's __init__ gives the functions named in INTEGRATORS to Context as methods; their first
parameter is the context."""
from __future__ import annotations

import numpy as np

from . import BOUNCE_MISS, BOUNCE_SCATTERED, MEDIA_COLLIDED, MEDIA_ESCAPED, Camera, MediaMarch, Photons, _Arrays, _Tensors, _is_tensor

INTEGRATORS = ("trace", "trace_direct", "trace_light", "trace_photons", "trace_photon_map", "trace_environment", "trace_media",
               "trace_media_direct", "trace_patches")


def _flags(x, dev):
    """A per-object bool operand (diffuse_objects, glossy_objects; a tensor or anything numpy takes) as a flat bool tensor on dev."""
    import torch
    return torch.as_tensor(np.asarray(x.cpu() if _is_tensor(x) else x).astype(bool)).to(dev).reshape(-1)


def _colours(x, dev):
    """A per-object colour operand (emission) as an (n_objects, 3) float64 tensor on dev."""
    import torch
    return torch.as_tensor(x, dtype=torch.float64).to(dev).reshape(-1, 3)


def _light_states(rng):
    """The light-draw states of trace_direct: per path and word k the splitmix64 finaliser (rng.nim:31-36's mixing) of
    s_k xor rotl(s_(k+1), 23) + (k + 1) * golden, in wrapping int64 tensor arithmetic -- a second stream per path that shares no
    draw with the path's own."""
    return _derived_states(rng, 0x9e3779b97f4a7c15)


_ENV_STREAM = 0xd1342543de82ef95   # the odd constant of trace_environment's third stream (where _light_states has the golden ratio's)
_CAMERA_STREAM = 0xf1357aea2e62a9c5   # the odd constant of trace_light's connection stream


def _derived_states(rng, constant):
    """A further stream per path: per path and word k the splitmix64 finaliser (rng.nim:31-36's mixing) of
    s_k xor rotl(s_(k+1), 23) + (k + 1) * constant, in wrapping int64 tensor arithmetic.  Streams of different odd constants
    share no draw with the path's own or with each other."""
    def lsr(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)

    def signed(c):
        return c - (1 << 64) if c >= (1 << 63) else c

    mix = signed(0xbf58476d1ce4e5b9)
    out = rng.clone()
    for k in range(4):
        nxt = rng[:, (k + 1) % 4]
        z = (rng[:, k] ^ ((nxt << 23) | lsr(nxt, 41))) + signed(((k + 1) * constant) & ((1 << 64) - 1))
        z = (z ^ lsr(z, 30)) * mix
        z = (z ^ lsr(z, 27)) * mix
        out[:, k] = z ^ lsr(z, 31)
    return out


class _Paths:
    """The path state of one integrator call, on the context's device: work (n, 7) the rays as the steps leave them, rng (n, 4)
    the path states (the caller's own tensor when it is contiguous, so it is updated in place), tr the one time range of all
    steps, color (n, 3), att (n, 3) the throughput of every path (`beta` for the light paths), live the int32 list of the paths
    that go on, res the BounceResult every step writes again and ran, the mode the first step ran.  from_rays starts camera
    paths, from_states and emit light paths; steps / step / advance are the loop's head and tail; finish is the exit."""
    __slots__ = ("ctx", "as_numpy", "n", "dev", "rng", "tr", "work", "color", "att", "live", "res", "ran", "skybuf")

    def __init__(self, ctx, as_numpy, rng, tr):
        import torch
        self.ctx, self.as_numpy, self.rng, self.tr = ctx, as_numpy, rng, tr
        self.n, self.dev = int(rng.shape[0]), rng.device
        self.live = torch.arange(self.n, dtype=torch.int32, device=self.dev)
        self.work = self.color = self.att = self.res = self.ran = self.skybuf = None

    @classmethod
    def from_rays(cls, ctx, who, rays, rng, time_range):
        """Camera paths along the caller's rays (CUDA tensors, or numpy operands through the device), which are not modified:
        color 0, att 1.  time_range None: the rays' finite times."""
        import torch
        as_numpy = not _is_tensor(rays)
        if as_numpy:
            host = _Arrays(ctx, who, np.asarray(rays, dtype=np.float64).reshape(-1, 7), "rays", 7)
            rays, rng = ctx._to_device(host.lead), ctx._to_device(host.states(rng).view(np.int64))
        ops = _Tensors(ctx, who, rays, "rays", 7)
        self = cls(ctx, as_numpy, ops.states(rng), ops.times(6, time_range))
        self.work = ops.lead.clone()
        self.color = torch.zeros((ops.n, 3), dtype=torch.float64, device=ops.dev)
        self.att = torch.ones((ops.n, 3), dtype=torch.float64, device=ops.dev)
        return self

    @classmethod
    def from_states(cls, ctx, who, rng, time_range):
        """Light paths, which start from states alone (a CUDA tensor, or numpy states through the device): emit() gives them
        their rays and att.  time_range: the emission's (lo, hi)."""
        import torch
        as_numpy = not _is_tensor(rng)
        if as_numpy:
            st = np.asarray(rng)
            if st.ndim != 2 or st.shape[1] != 4 or st.dtype.kind not in "iu" or st.dtype.itemsize != 8:
                raise ValueError(f"Context.{who}: rng must be an (n, 4) array of 64-bit integers")
            rng = ctx._to_device(np.ascontiguousarray(st).view(np.int64))
        elif rng.dtype not in (torch.int64, torch.uint64) or rng.dim() != 2 or rng.shape[1] != 4 or not rng.is_cuda:
            raise ValueError(f"Context.{who}: rng must be an (n, 4) int64 CUDA tensor")
        return cls(ctx, as_numpy, rng.contiguous(), (float(time_range[0]), float(time_range[1])))

    def emit(self, emission):
        """Start every path on a lamp of the light table (emit_lights; n > 0): work the emitted rays, att = Le * pi / pdf_area.
        Returns (the LightEmission, the lamps' object indices)."""
        em = self.ctx.emit_lights(self.rng, self.tr)
        lamp = em.light.long().clamp(min=0)
        self.work = em.rays.clone()
        self.att = emission[lamp] * (np.pi / em.pdf_area)[:, None]   # (a lamp of radius 0 has no area: it emits nothing)
        return em, lamp

    def entry(self):
        """The path states as int64 words, for _derived_states: ask before the first draw moves them."""
        import torch
        return self.rng.view(torch.int64) if self.rng.dtype != torch.int64 else self.rng

    def steps(self, max_depth):
        """The step numbers 0 .. max_depth - 1 for as long as a path is live."""
        for step in range(int(max_depth)):
            if self.live.numel() == 0:
                return
            yield step

    def step(self, mode, mask=None):
        """The head of a step: bounce the live paths.  Returns (idx: the live list as int64, st: their status, the BounceResult)."""
        self.res = res = self.ctx.bounce(self.work, self.rng, self.live, self.tr, mode, out=self.res, mask=mask)
        self.ran = self.ran or res.mode
        idx = self.live.long()
        return idx, res.status[idx], res

    def advance(self, stop=None, albedo=None):
        """The tail of a step: the paths that scattered stay live, in order (bounce_select) -- but for those that hit an object
        flagged in `stop` (one bool per object), which end here -- and att *= attenuation for them (render.nim:35); with
        `albedo` ((n, 3), Context.albedo's colours of the step's records) att *= albedo instead.  Returns the new live list as
        int64."""
        live = self.ctx.bounce_select(self.res.status, self.live)
        if stop is not None:
            live = live[~stop[self.res.object[live.long()].long().clamp(min=0)]]
        self.live = live
        scat = live.long()
        self.att[scat] = self.att[scat] * (self.res.attenuation if albedo is None else albedo)[scat]
        return scat

    def sky_on_miss(self, sky, idx, st):
        """A stepped path that missed ends with sky * att (render.nim:45).  sky None: Context.sky for every stepped ray, kept
        where it missed -- no list of the misses, so no host synchronisation; else the caller's sky(rays, index) for the misses."""
        import torch
        if sky is not None:
            self.caller_sky(sky, idx[st == BOUNCE_MISS])
            return
        if self.skybuf is None:
            self.skybuf = torch.zeros((self.n, 3), dtype=torch.float64, device=self.dev)
        self.ctx.sky(self.work, self.live, out=self.skybuf)
        self.color[idx] = torch.where((st == BOUNCE_MISS)[:, None], self.skybuf[idx] * self.att[idx], self.color[idx])

    def caller_sky(self, sky, miss):
        """color = sky(rays, index) * att for the paths of the int64 list `miss`, if there are any."""
        import torch
        if miss.numel():
            self.color[miss] = torch.as_tensor(sky(self.work, miss.int()), dtype=torch.float64).to(self.dev).reshape(-1, 3) \
                * self.att[miss]

    def finish(self, *results):
        """The exit: (*results, rng, the mode that ran or "nothing to do") -- the tensors as numpy arrays, the states as uint64,
        when the operands came as numpy."""
        ran = self.ran or "nothing to do"
        if not self.as_numpy:
            return (*results, self.rng, ran)
        return (*(r.cpu().numpy() if _is_tensor(r) else r for r in results), self.rng.cpu().numpy().view(np.uint64), ran)


class _LambertianNee:
    """The next-event bookkeeping of the integrators that restate the Lambertian density themselves (trace_direct's default path,
    trace_environment): per path the shading point of its last diffuse hit, the density cos / pi of the direction it left in,
    and whether it left a camera, a Metal or a Dielectric instead.  Which sampler is asked, the cosine of its direction and the
    emitted colour are the caller's."""
    __slots__ = ("paths", "diffuse", "points", "p_bsdf", "specular")

    def __init__(self, paths, diffuse):
        import torch
        n, dev = paths.n, paths.dev
        self.paths, self.diffuse = paths, diffuse
        self.points = torch.zeros((n, 4), dtype=torch.float64, device=dev)      # the shading point of every ray's last diffuse hit ...
        self.p_bsdf = torch.zeros((n,), dtype=torch.float64, device=dev)        # ... the Lambertian density of the direction it left in ...
        self.specular = torch.ones((n,), dtype=torch.bool, device=dev)          # ... or: the ray left a camera, a Metal or a Dielectric

    def vertices(self, scat, last):
        """After advance(): books the paths `scat` that go on as diffuse or specular, and for the diffuse ones their point and
        p_bsdf.  Returns (nee: the diffuse ones as int64, the same list as int32, their normals) -- or None when there are none
        or this is the last step (a light sample after it would be one vertex more than trace() follows)."""
        import torch
        work, res = self.paths.work, self.paths.res
        isdiff = self.diffuse[res.object[scat].long()]
        self.specular[scat] = ~isdiff
        nee = scat[isdiff]
        if nee.numel() == 0 or last:
            return None
        self.points[nee, 0:3], self.points[nee, 3] = res.p[nee], work[nee, 6]
        nrm = res.normal[nee]
        d = work[nee, 3:6]
        cos_out = (nrm * d).sum(1) / torch.sqrt((d * d).sum(1))
        self.p_bsdf[nee] = torch.clamp(cos_out, min=0.0) / np.pi
        return nee, nee.int(), nrm

    def add(self, nee, cos_l, pdf, free, emitted, mis):
        """color += att * emitted * (cos_l / pi / pdf * share) for the vertices `nee` whose sample is `free`, has a usable
        density `pdf` and lies above the surface; share = pdf / (pdf + cos_l / pi) with mis, else 1."""
        import torch
        color, att = self.paths.color, self.paths.att
        ok = free & (pdf > 0) & torch.isfinite(pdf) & (cos_l > 0)
        share = pdf / (pdf + cos_l / np.pi) if mis else torch.ones_like(pdf)
        add = att[nee] * emitted * (cos_l / np.pi / pdf * share)[:, None]
        color[nee] = color[nee] + torch.where(ok[:, None], add, torch.zeros_like(add))


def _need_textures(ctx, who):
    """textures=True asks for a texture table (set_textures): refused before the first launch."""
    if ctx.textures()[0] == 0:
        raise ValueError(f"Context.{who}: textures=True needs a texture table (set_textures)")


def trace(ctx, rays, rng, max_depth=50, sky=None, emission=None, time_range=None, mode="auto", on_bounce=None, textures=False,
          mask=None):
    """A wavefront path tracer on top of bounce(): radiance()'s loop (render.nim:21-47) one step per launch, open where the
    reference is closed.  att = 1; per step: bounce the live rays; a miss ends with sky * att; with `emission` every hit adds
    att * emission[object] (before the attenuation is updated); att *= attenuation for the rays that scattered, which stay
    live, in order; rays still live after max_depth steps are black.  Returns (color (n, 3), rng (n, 4) after the path's last
    draw, the mode that ran).  With sky, emission and on_bounce all None this is Context.radiance: colours and states, bit
    for bit.

    sky: None (Context.sky, the reference's gradient) or sky(rays, index) -> (len(index), 3) colours of the listed rays.
    emission: (n_objects, 3) float64.  on_bounce(step, index, result): called after every step with the list that was
    stepped (int32 tensor) and its BounceResult (result.rays are the scattered rays) -- the hook for feature buffers.
    rays are not modified; a contiguous CUDA rng tensor is updated in place; numpy operands go through the device and come
    back as numpy.  One time range for all steps: time_range, or the rays' finite times (the library adds 0).
    mask: as for bounce(), for every step; or a callable mask(step) -> int | per-ray words, so that step 0 (the camera's rays)
    sees other objects than the later steps.
    textures: False -- every launch and every bit as above; True -- the surfaces take their colour from the texture table
    (set_textures; a ValueError without one): after each step albedo(result, the stepped list) runs, and att *= its colour
    replaces att *= attenuation for the rays that scattered.  An object without a texture answers its attenuation, so with no
    object bound the colours and states are those of textures=False, bit for bit.  `mask` stays the trailing parameter; a call
    from before `textures` existed that passes its mask by POSITION lands in `textures`, which is a bool (Python's or numpy's)
    and nothing else: any other value there is taken as that mask, so every such call keeps its meaning -- unless `mask` is given
    too, which no such call could do: that is a ValueError."""
    if not isinstance(textures, (bool, np.bool_)):
        if mask is not None:
            raise ValueError("Context.trace: textures must be a bool (a mask goes into mask=)")
        mask, textures = textures, False
    if textures:
        _need_textures(ctx, "trace")
    p = _Paths.from_rays(ctx, "trace", rays, rng, time_range)
    color, att, tex = p.color, p.att, None
    if emission is not None:
        emission = _colours(emission, p.dev)
    for step in p.steps(max_depth):
        idx, st, res = p.step(mode, mask(step) if callable(mask) else mask)
        p.sky_on_miss(sky, idx, st)
        if emission is not None:
            hit = idx[st != BOUNCE_MISS]
            color[hit] = color[hit] + att[hit] * emission[res.object[hit].long()]
        if on_bounce is not None:
            on_bounce(step, p.live, res)
        if textures:
            tex = ctx.albedo(res, p.live, out=tex)
            p.advance(albedo=tex.color)
        else:
            p.advance()
    return p.finish(color)


def trace_patches(ctx, rays, rng, max_depth=50, sky=None, emission=None, patch_emission=None, time_range=None, mode="auto",
                  mask=None):
    """trace()'s loop over the spheres AND the patch table (set_patches; a ValueError without one): a floor, walls, a lamp
    panel, boxes.  att = 1; per step, for the live rays: hit() (with `mask`, if given), then hit_patches(merge=) of the same
    rays with the same mask -- the closest of spheres and patches, a tie staying with the sphere --; a ray with neither an
    object nor a patch ends with sky * att; every record with object >= 0 adds att * emission[object], every patch hit adds
    att * patch_emission[patch]; a patch without a material (-1) ends its path there, with no sky; the rest go through
    scatter(), att *= attenuation for the rays that scattered, which stay live, in order.  Returns (color, rng, the mode hit()
    ran).

    With a table that no ray reaches, colours and states are trace()'s with the same arguments, bit for bit (bounce() equals
    hit() followed by scatter()), and Context.radiance's when sky, emission and patch_emission are None.
    sky, emission, time_range, mode as for trace(); patch_emission: (n_patches, 3) float64; mask: None, an int or per-ray
    words, for every step.  rays are not modified; a contiguous CUDA rng tensor is updated in place; numpy operands go through
    the device and come back as numpy."""
    import torch
    if ctx.patches()[0] == 0:
        raise ValueError("Context.trace_patches: needs a patch table (set_patches)")
    p = _Paths.from_rays(ctx, "trace_patches", rays, rng, time_range)
    color, att, work, states = p.color, p.att, p.work, p.entry()
    if emission is not None:
        emission = _colours(emission, p.dev)
    if patch_emission is not None:
        patch_emission = _colours(patch_emission, p.dev)
    if mask is not None and not isinstance(mask, (int, np.integer)):
        mask = torch.as_tensor(np.asarray(mask.cpu() if _is_tensor(mask) else mask).astype(np.int64) & 0xFFFFFFFF).to(p.dev)
    for step in p.steps(max_depth):
        idx = p.live.long()
        r, s = work[idx], states[idx]   # the live rays and their states, compacted: every query of the step answers all of them
        m = mask if mask is None or isinstance(mask, (int, np.integer)) else mask[idx].to(torch.int32)
        spheres = ctx.hit(r, None, p.tr, mode, mask=m)
        p.ran = p.ran or spheres.mode
        rec = ctx.hit_patches(r, mask=m, merge=spheres)
        obj, patch = rec.object.long(), rec.patch.long()
        on_patch, has_obj = patch >= 0, obj >= 0
        miss = ~on_patch & ~has_obj
        if sky is None:
            color[idx] = torch.where(miss[:, None], ctx.sky(r) * att[idx], color[idx])
        else:
            p.caller_sky(sky, idx[miss])
        if emission is not None:
            color[idx] = color[idx] + torch.where(has_obj[:, None], att[idx] * emission[obj.clamp(min=0)], torch.zeros_like(r[:, 0:3]))
        if patch_emission is not None:
            color[idx] = color[idx] + torch.where(on_patch[:, None], att[idx] * patch_emission[patch.clamp(min=0)],
                                                  torch.zeros_like(r[:, 0:3]))
        res = ctx.scatter(r, rec, s)   # (a record without an object is scatter()'s miss: nothing drawn, ray and state kept)
        work[idx], states[idx] = res.rays, res.rng
        scat = res.status == BOUNCE_SCATTERED
        on = idx[scat]
        att[on] = att[on] * res.attenuation[scat]
        p.live = on.int()
    return p.finish(color)


def trace_direct(ctx, rays, rng, emission, diffuse, max_depth=50, sky=None, mis=False, lamp_mask=None, time_range=None,
                 mode="auto", strategy="solid_angle", glossy=None, textures=False):
    """trace()'s loop with next-event estimation: after each bounce, the rays that hit a diffuse object sample one light of
    the table (sample_lights), ask occluded() whether the segment to the sampled surface point is free, and add
        att * albedo / pi * emission[light] * max(0, n . unit(dir)) / pdf
    where it is.  Emission FOUND by hitting an object counts only at step 0 or after a Metal / Dielectric bounce -- or, with
    mis=True, everywhere with balance-heuristic weights: light_pdf against the Lambertian density cos / pi, on both sides.
    Every emitter that diffuse surfaces are to see must be in the light table (set_lights).  The last of the max_depth steps
    samples no light, so both ways of finding a lamp follow paths of the same lengths, trace()'s.

    emission: (n_objects, 3) float64.  diffuse: (n_objects,) bool (diffuse_objects(scene)).  lamp_mask: the occluded() mask
    of the shadow segments; with one, their range is (0.001, 1.0) and the mask must leave the lamps' group out (set_groups);
    None: every group, and the range ends at 1 - 1e-9 instead, just short of the sampled surface.  rays, rng, sky,
    time_range, mode and the result (color, rng, mode) as for trace(); strategy as for sample_lights.

    glossy: None (the code path above, unchanged in every bit), or (n_objects,) bool (glossy_objects(scene): Metal with
    fuzz != 0).  With it the material is no longer restated here: a vertex on a diffuse OR a glossy object takes the light
    sample -- also one whose scattered ray Metal absorbed -- and is no longer booked specular; one bsdf() call gives value
    and density p_b of the sampled light direction, and the sample adds att * value * emission[light] / pdf where the
    segment is free and p_b > 0; with mis=True a second bsdf() call gives the density of the direction the path left in,
    the partner of light_pdf in the balance weights on both sides.

    The light draws come from a second state per path, derived from the path's entry state (splitmix64 finalisers over its
    words), not from the path state itself: the bounces see exactly the states trace() gives them.  So with an all-zero
    emission the colours are trace()'s, bit for bit, and the returned states are the path states, as trace() returns
    them.

    textures: False -- every launch and every bit as above; True -- as for trace(): albedo(result, the stepped list) after each
    step, att *= its colour for the rays that scattered (on the default path the throughput carries the albedo into the light
    sample, so nothing else changes), and on the `glossy=` path the light sample's value is colour * p_b in place of bsdf()'s
    albedo * p_b.  A ValueError without a texture table."""
    import torch
    if textures:
        _need_textures(ctx, "trace_direct")
    tex = None
    p = _Paths.from_rays(ctx, "trace_direct", rays, rng, time_range)
    n, dev, f64 = p.n, p.dev, torch.float64
    work, color, att, tr = p.work, p.color, p.att, p.tr
    emission, diffuse = _colours(emission, dev), _flags(diffuse, dev)
    lrng = _light_states(p.entry())
    lamb = _LambertianNee(p, diffuse)
    points, p_bsdf, specular = lamb.points, lamb.p_bsdf, lamb.specular
    t_range = torch.empty((n, 2), dtype=f64, device=dev)
    t_range[:, 0], t_range[:, 1] = 0.001, (1.0 if lamp_mask is not None else 1.0 - 1e-9)
    ls, occ = None, None
    nee_ok, win, ev, ev2 = None, None, None, None
    if glossy is not None:   # the objects whose vertices take a light sample, and the incoming rays of the step (bsdf's rays_in)
        nee_ok, win = diffuse | _flags(glossy, dev), torch.empty_like(work)
    for step in p.steps(max_depth):
        if nee_ok is not None:
            win.copy_(work)
        idx, st, res = p.step(mode)
        p.sky_on_miss(sky, idx, st)
        hit = idx[st != BOUNCE_MISS]
        obj = res.object[hit].long()
        # emission found by hitting it: the whole of it after a specular vertex; after a diffuse one nothing, or its MIS share
        wgt = specular[hit].to(f64)
        if mis and hit.numel():
            p_light = ctx.light_pdf(points, res.object, hit.int(), strategy)[hit]
            share = p_bsdf[hit] / (p_bsdf[hit] + p_light)
            wgt = torch.where(specular[hit], wgt, torch.where(torch.isfinite(share), share, torch.zeros_like(share)))
        color[hit] = color[hit] + att[hit] * emission[obj] * wgt[:, None]
        if nee_ok is not None:   # (before the attenuation moves on: the light sample is weighted by att * value)
            nee = hit[nee_ok[obj]]
            att_nee = att[nee]
        if textures:
            tex = ctx.albedo(res, p.live, out=tex)
            scat = p.advance(albedo=tex.color)
        else:
            scat = p.advance()
        if nee_ok is not None:
            # next-event estimation at every diffuse or glossy vertex, through bsdf(): also where Metal absorbed the
            # scattered ray -- the vertex reflects the lamp whatever became of the one direction the scatter drew
            specular[scat] = ~nee_ok[res.object[scat].long()]
            if nee.numel() == 0 or step == int(max_depth) - 1:
                continue
            points[nee, 0:3], points[nee, 3] = res.p[nee], win[nee, 6]
            lst = nee.int()
            ls = ctx.sample_lights(points, lrng, lst, strategy, out=ls)
            occ = ctx.occluded(ls.rays, t_range, lst, tr, mode, out=occ, mask=lamp_mask)
            ev = ctx.bsdf(win, res, ls.rays, lst, out=ev)
            p_b, pdf, lamp = ev.pdf[nee], ls.pdf[nee], ls.light[nee].long()
            ok = (~occ.occluded[nee]) & (lamp >= 0) & (pdf > 0) & torch.isfinite(pdf) & (p_b > 0) & torch.isfinite(p_b)
            share = pdf / (pdf + p_b) if mis else torch.ones_like(pdf)
            value = tex.color[nee] * ev.pdf[nee][:, None] if textures else ev.value[nee]
            add = att_nee * value * emission[lamp.clamp(min=0)] * (share / pdf)[:, None]
            color[nee] = color[nee] + torch.where(ok[:, None], add, torch.zeros_like(add))
            if mis:   # the density of the direction the path actually left in (0 for an absorbed ray: it found nothing)
                ev2 = ctx.bsdf(win, res, work, lst, out=ev2)
                p_bsdf[nee] = ev2.pdf[nee]
            continue
        # next-event estimation at the diffuse hits that go on
        at = lamb.vertices(scat, step == int(max_depth) - 1)
        if at is None:
            continue
        nee, lst, nrm = at
        ls = ctx.sample_lights(points, lrng, lst, strategy, out=ls)
        occ = ctx.occluded(ls.rays, t_range, lst, tr, mode, out=occ, mask=lamp_mask)
        sd = ls.rays[nee, 3:6]
        cos_l = (nrm * sd).sum(1) / torch.sqrt((sd * sd).sum(1))
        lamp = ls.light[nee].long()
        lamb.add(nee, cos_l, ls.pdf[nee], (~occ.occluded[nee]) & (lamp >= 0), emission[lamp.clamp(min=0)], mis)
    return p.finish(color)


def trace_light(ctx, cam: Camera, nrows: int, ncols: int, rng, emission, diffuse, max_depth=50, lamp_mask=None, time_range=None,
                mode="auto", splat=None):
    """A light tracer on top of emit_lights, bounce, connect_camera and occluded: one path per state starts on a lamp of the
    light table (set_lights) with beta = Le * pi / pdf_area, and every vertex the camera can see directly is splatted into
    the pixel it lands in.  The emission vertex itself adds Le * cos_y * factor / pdf_area where cos_y > 0.  Per step the
    live rays bounce; every hit on a `diffuse` object is connected (connect_camera), the segment to the lens point asked of
    occluded() with range (0.001, 1.0), and where it is free and cos_y > 0 (the face normal the step returned against the
    unit direction to the lens point) the vertex adds beta * albedo / pi * cos_y * factor; then beta *= attenuation for the
    rays that scattered, which stay live, for at most max_depth steps.

    Each batch goes to splat(pixels, colors, index): pixels (n,) int32 (-1 where nothing is added), colors (n, 3) float64
    already divided by nrows * ncols, index the int32 list of the entries of this batch -- Film.deposit's signature; with
    N paths in all, a pixel's radiance estimate is the sum of its splats times nrows * ncols / N.  splat None: nothing is
    kept.  Returns (the number of splats offered, rng after the paths' last draws, the mode that ran).

    emission: (n_objects, 3) float64, the radiance Le of every lamp.  diffuse: (n_objects,) bool (diffuse_objects(scene)).
    lamp_mask: the occluded() mask of the connection segments (None: every group).  time_range: the emission's (lo, hi);
    None: the camera's shutter interval.  rng: (n, 4) states, a contiguous CUDA tensor is updated in place; numpy states
    go through the device and come back as numpy.  The connection draws come from a second state per path, derived from
    the path's entry state (_derived_states with a constant of its own), so the bounces see the states they would see
    without connections.

    What a light tracer cannot see: surfaces the camera sees THROUGH a Metal or Dielectric vertex (a mirror image, the
    far side of a glass ball) -- no connection reaches the lens by way of a specular vertex; those need trace / trace_direct
    / trace_environment.  Mixing both estimators in one film counts the directly seen diffuse surfaces twice and is out of
    scope, as are multiple importance sampling between them and the sky (an environment is no lamp of the table)."""
    import torch
    p = _Paths.from_states(ctx, "trace_light", rng, (cam.shutter_open, cam.shutter_close) if time_range is None else time_range)
    n, dev, f64, tr = p.n, p.dev, torch.float64, p.tr
    emission, diffuse = _colours(emission, dev), _flags(diffuse, dev)
    inv_npix = 1.0 / float(int(nrows) * int(ncols))
    crng = _derived_states(p.entry(), _CAMERA_STREAM)
    if n == 0:
        return p.finish(0)
    em, lamp = p.emit(emission)
    work, beta, pdf_area = p.work, p.att, em.pdf_area
    points = torch.zeros((n, 4), dtype=f64, device=dev)
    t_range = torch.empty((n, 2), dtype=f64, device=dev)
    t_range[:, 0], t_range[:, 1] = 0.001, 1.0
    colors = torch.zeros((n, 3), dtype=f64, device=dev)
    offered = 0

    def connect(lst, nrm, weight, conn, occ):
        """Connect the listed vertices (their points are set): splat weight * cos_y * factor / npix where visible."""
        conn = ctx.connect_camera(cam, nrows, ncols, points, crng, lst, out=conn)
        occ = ctx.occluded(conn.rays, t_range, lst, tr, mode, out=occ, mask=lamp_mask)
        at = lst.long()
        d = conn.rays[at, 3:6]
        cos_y = (nrm * d).sum(1) / torch.sqrt((d * d).sum(1))
        ok = (conn.pixel[at] >= 0) & (~occ.occluded[at]) & (cos_y > 0)
        add = weight * (cos_y * conn.factor[at] * inv_npix)[:, None]
        colors[at] = torch.where(ok[:, None] & torch.isfinite(add), add, torch.zeros_like(add))
        pixels = torch.where(ok, conn.pixel[at], torch.full_like(conn.pixel[at], -1))
        conn.pixel[at] = pixels
        if splat is not None:
            splat(conn.pixel, colors, lst)
        return conn, occ, int(lst.numel())

    points[:, 0:3], points[:, 3] = work[:, 0:3], work[:, 6]
    conn, occ, k = connect(p.live, em.normal, emission[lamp] / pdf_area[:, None], None, None)
    offered += k
    for step in p.steps(max_depth):
        idx, st, res = p.step(mode)
        obj = res.object[idx].long().clamp(min=0)
        at = idx[(st != BOUNCE_MISS) & diffuse[obj]]
        if at.numel():
            points[at, 0:3], points[at, 3] = res.p[at], work[at, 6]
            conn, occ, k = connect(at.int(), res.normal[at], beta[at] * res.attenuation[at] / np.pi, conn, occ)
            offered += k
        p.advance()
    return p.finish(offered)


def trace_photons(ctx, rng, emission, diffuse, max_depth=50, caustic_only=False, lamp_mask=None, time_range=None, mode="auto") -> "Photons":
    """trace_light's loop without the connections: one light path per state starts on a lamp of the light table
    (set_lights, emit_lights) with beta = Le * pi / pdf_area; per step the live rays bounce, and every hit on a `diffuse`
    object stores a photon {p, beta as it ARRIVES (before the surface's albedo), the incoming ray's direction (not
    normalised: a gather uses only its sign against the normal)}; then beta *= attenuation for the rays that scattered,
    which stay live, for at most max_depth steps.

    caustic_only: keep a photon only if its path has taken at least one specular step (a hit on an object that is not
    `diffuse`) and no diffuse one; the path stops at its first diffuse hit.  emission, diffuse, time_range ((lo, hi) of the
    emission; None: (0, 0)), mode and rng as for trace_light; lamp_mask is accepted for symmetry and unused (there are no
    connection segments).  Returns Photons(position (m, 3), power (m, 3), direction (m, 3), paths = n, rng, mode): the
    operands of build_photons.  The powers are NOT divided by the path count: PhotonGather.irradiance(paths) does that, so
    the photons of several calls concatenate."""
    import torch
    p = _Paths.from_states(ctx, "trace_photons", rng, (0.0, 0.0) if time_range is None else time_range)
    n, dev = p.n, p.dev
    emission, diffuse = _colours(emission, dev), _flags(diffuse, dev)
    pos, pw, dr = [], [], []
    if n:
        em, lamp = p.emit(emission)
        p.att = torch.where((em.light >= 0)[:, None], p.att, torch.zeros_like(p.att))
        work, beta = p.work, p.att
        specular = torch.zeros(n, dtype=torch.bool, device=dev)   # the path has taken a specular step
        win = torch.empty_like(work)
        for step in p.steps(max_depth):
            win.copy_(work)   # the incoming rays of the step: bounce() writes the scattered ones over `work`
            idx, st, res = p.step(mode)
            obj = res.object[idx].long().clamp(min=0)
            hit = st != BOUNCE_MISS
            on_diffuse = hit & diffuse[obj]
            at = idx[on_diffuse & specular[idx]] if caustic_only else idx[on_diffuse]
            if at.numel():
                pos.append(res.p[at].clone()), pw.append(beta[at].clone()), dr.append(win[at, 3:6].clone())
            specular[idx[hit & ~diffuse[obj]]] = True
            p.advance(stop=diffuse if caustic_only else None)   # (caustic_only: the path stops at its first diffuse hit)
    cat = (lambda parts: torch.cat(parts) if parts else torch.zeros((0, 3), dtype=torch.float64, device=dev))
    position, power, direction, rng, ran = p.finish(cat(pos), cat(pw), cat(dr))
    return Photons(position, power, direction, n, rng, ran)


def trace_photon_map(ctx, rays, rng, emission, diffuse, paths, radius=None, kernel="epanechnikov", max_depth=50, time_range=None,
                     mode="auto"):
    """Direct visualisation of the context's photon map (build_photons from trace_photons' photons of `paths` light paths in
    all, caustic_only=False): every camera ray is followed through its specular steps, with trace()'s bookkeeping, to its
    first hit on a `diffuse` object, where the map is gathered (gather_photons with the face normal the step returned); the
    colour is
        sum over the hits on the way of att * emission[object]  +  att * albedo / pi * irradiance estimate
    with att the product of the attenuations of the steps before, and albedo the attenuation of the diffuse step.  A ray
    that misses is black: the sky is no source here (an environment is no lamp of the light table), and neither is it in
    trace_photons.  The estimator is complete on its own: emission is seen directly or through specular vertices only,
    every other light path of the scene is in the map once, so nothing is counted twice.  The path ends at that diffuse
    hit (the albedo is the step's attenuation; a step the material absorbed reflects nothing).  Mixing it with trace_direct
    is out of scope.

    rays, rng, time_range, mode, max_depth as for trace(); radius, kernel as for gather_photons.  Returns (color (n, 3),
    rng, the mode that ran)."""
    import torch
    p = _Paths.from_rays(ctx, "trace_photon_map", rays, rng, time_range)
    n, dev, color, att = p.n, p.dev, p.color, p.att
    emission, diffuse = _colours(emission, dev), _flags(diffuse, dev)
    points, normals = torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros((n, 3), dtype=torch.float64, device=dev)
    gat = None
    for step in p.steps(max_depth):
        idx, st, res = p.step(mode)
        hit = idx[st != BOUNCE_MISS]
        obj = res.object[hit].long()
        color[hit] = color[hit] + att[hit] * emission[obj]
        at = hit[diffuse[obj]]
        if at.numel():
            points[at], normals[at] = res.p[at], res.normal[at]
            gat = ctx.gather_photons(points, normals, radius, at.int(), kernel, out=gat)
            albedo = torch.where((res.status[at] == BOUNCE_SCATTERED)[:, None], res.attenuation[at], torch.zeros_like(att[at]))
            color[at] = color[at] + att[at] * albedo / np.pi * gat.irradiance(paths)[at]
        p.advance(stop=diffuse)   # (the path ends at its first diffuse hit)
    return p.finish(color)


def trace_environment(ctx, rays, rng, diffuse, max_depth=50, direct=True, mis=False, time_range=None, mode="auto"):
    """trace()'s loop with the environment map (set_environment) as the sky, and next-event estimation towards it: a ray
    that misses adds att * environment(ray) * w, and with `direct` every diffuse hit that goes on (except on the last of
    the max_depth steps) draws a direction from the map (sample_environment), asks occluded() with range (0.001, +inf)
    whether it is free, and adds att * color * (cos / pi / pdf * share) where it is.  w = 1 when `direct` is off or the
    ray left the camera, a Metal or a Dielectric; otherwise 0, or with mis=True the balance share
    p_bsdf / (p_bsdf + p_env) -- `share` is then p_env / (p_env + p_bsdf), else 1.  p_bsdf is the Lambertian density
    cos / pi, p_env the map's density of the direction (environment(pdf=True)).

    diffuse: (n_objects,) bool (diffuse_objects(scene)).  rays, rng, time_range, mode and the result (color, rng, mode) as
    for trace().  No step builds a list of the misses, so none synchronises with the host on their count.

    The environment draws come from a third state per path, derived from the path's entry state like trace_direct's light
    states but with the constant 0xd1342543de82ef95 in place of the golden ratio's 0x9e3779b97f4a7c15: the bounces see
    exactly the states trace() gives them.  So with direct=False the colours are those of
    trace(sky=lambda rays, idx: ctx.environment(rays, idx)[idx.long()]), bit for bit, and the returned states are the path
    states, as trace() returns them."""
    import torch
    p = _Paths.from_rays(ctx, "trace_environment", rays, rng, time_range)
    work, color, att, f64 = p.work, p.color, p.att, torch.float64
    diffuse = _flags(diffuse, p.dev)
    erng = _derived_states(p.entry(), _ENV_STREAM)
    lamb = _LambertianNee(p, diffuse)
    p_bsdf, specular = lamb.p_bsdf, lamb.specular
    es, occ, ev = None, None, None
    for step in p.steps(max_depth):
        idx, st, res = p.step(mode)
        # the map's colour (and density) of every stepped ray, kept where it missed: no list of the misses
        if direct and mis:
            ev = ctx.environment(work, p.live, out=ev, pdf=True)
            sky, p_env = ev.color[idx], ev.pdf[idx]
            share = p_bsdf[idx] / (p_bsdf[idx] + p_env)
            wgt = torch.where(specular[idx], torch.ones_like(share), torch.where(torch.isfinite(share), share, torch.zeros_like(share)))
            sky = sky * att[idx] * wgt[:, None]
        else:
            ev = ctx.environment(work, p.live, out=ev)
            sky = ev[idx] * att[idx]
            if direct:
                sky = sky * specular[idx].to(f64)[:, None]
        color[idx] = torch.where((st == BOUNCE_MISS)[:, None], color[idx] + sky, color[idx])
        scat = p.advance()
        if not direct:
            continue
        # next-event estimation at the diffuse hits that go on
        at = lamb.vertices(scat, step == int(max_depth) - 1)
        if at is None:
            continue
        nee, lst, nrm = at
        es = ctx.sample_environment(lamb.points, erng, lst, out=es)
        occ = ctx.occluded(es.rays, None, lst, p.tr, mode, out=occ)
        cos_l = (nrm * es.rays[nee, 3:6]).sum(1)              # (the sampled direction is unit)
        lamb.add(nee, cos_l, es.pdf[nee], ~occ.occluded[nee], es.color[nee], mis)
    return p.finish(color)


def trace_media(ctx, rays, rng, max_depth=50, sky=None, mask=None, free_flight=None, phase=False):
    """The volumetric twin of trace(): a wavefront path tracer through the surfaces of the scene and the media of the table.
    att = 1; per iteration, for the live rays, in this order: hit() with `mask` (the surfaces a ray sees; the media's
    boundary spheres belong to a group the mask leaves out); ONE uniform01 per live ray (uniform()); tau = free_flight(u),
    default -log1p(-u) (torch's: the library takes no logarithm); march_media() with range (0, the hit's t or +inf).  A ray
    that collided scatters isotropically (scatter_media(): two more outputs of its stream) and att *= the mixture's albedo;
    one that reached its surface scatters as the reference's material does (scatter(): that material's draws), att *= its
    attenuation, and an absorbed ray ends black; one that reached nothing ends with sky * att.  Rays still live after
    max_depth iterations are black.  So the draw order of a path is, per iteration, the free-flight uniform first, then
    the draws of whichever scatter it met.  Returns (color (n, 3), rng (n, 4) after the path's last draw).

    phase: False -- the isotropic scatter above; True -- a collision scatters by the media's Henyey-Greenstein phase functions
    (set_media_phase; sample_phase(): three outputs of the stream where scatter_media draws two, at the same place of the
    draw order) and att *= its attenuation.

    sky: None (Context.sky) or sky(rays, index) -> (len(index), 3), as for trace().  mask: as for hit(), or a callable
    mask(step).  free_flight: a callable on the (n,) tensor of uniforms giving tau (every entry is evaluated, the live ones
    are used).  hit() takes no list, so every iteration's closest-hit launch runs on all n rays and the hits of the rays
    that have ended are not read; uniform, march_media and the two scatters run on the live list.

    Density grids (set_media_grid): with K media that have one, ascending m_1 < .. < m_K, an iteration draws
    1 + K uniforms per live ray in ONE uniform() call -- u[0] for the table, u[j] for grid medium m_j --, so the draw order of
    a path is, per iteration, the table's free-flight uniform, the K grid uniforms in ascending medium order, then the draws
    of whichever scatter it met.  tau_j = free_flight(u[j]).  First the homogeneous march up to the hit; then
    march_media_grid of m_1 .. m_K in that order, each with t_max = the earliest collision so far (or the hit): a grid march
    that collides replaces the candidate (independent Poisson processes superpose: the earliest collision is the path's).
    The winner's (t, active) -- active = 1 << m for a grid medium -- feed the scatter.  K = 0: every launch as before.  rays are not modified; a contiguous CUDA rng tensor is updated in place; numpy operands go through the
    device and come back as numpy."""
    return _media_loop(ctx, "trace_media", rays, rng, max_depth, sky, mask, free_flight, phase, None)


def trace_media_direct(ctx, rays, rng, emission, lamp_mask, max_depth=50, sky=None, mask=None, free_flight=None, transmit=None,
                       strategy="solid_angle"):
    """trace_media(phase=True) plus lamps: the lamps of the light table (set_lights) light the fog.  Emission found by hitting
    an object adds att * emission[object] -- unless the path's previous vertex was a medium collision, where the light sample
    has already counted it.  At every collision that is not on the last of the max_depth steps, with the point the scattered
    ray's origin and time: sample_lights gives a segment to a lamp; occluded(segment, (0.001, 1.0), mask=lamp_mask) its
    visibility; march_media(segment, inf, (0.0, 1.0)) its optical depth; T = transmit(depth), default torch's exp(-depth) (a
    callable lets a test use defined bits, as free_flight does); phase(the incoming rays, the collision's active word, the
    segment) the value; and the collision adds
        att_before * value * emission[lamp] * (T / pdf)
    where the segment is free, lamp >= 0 and the light's pdf is finite and > 0.  lamp_mask is required (ValueError for
    None): without one the media's own boundary spheres would shadow every segment.

    The light draws come from _light_states of the paths' entry states, so path states and draw order are those of
    trace_media(phase=True), as trace_direct relates to trace: with an all-zero emission the colours and states are its,
    bit for bit.  With density grids the draw order is trace_media's (1 + K uniforms per iteration: the table's, then one per
    grid medium ascending), the winner's active word feeds phase(), and the shadow segment's depth is march_media's plus
    each grid medium's march_media_grid(segment, inf, m, (0.0, 1.0)) depth, added in ascending medium order, before transmit.  emission: (n_objects, 3) float64; strategy as for sample_lights; the rest as for trace_media.  Out of
    scope: light samples at surfaces through fog, MIS between phase and light sampling, chromatic extinction, phase
    functions other than Henyey-Greenstein.  (Heterogeneous density is DESIGN 4.26: set_media_grid.)"""
    if lamp_mask is None:
        raise ValueError("Context.trace_media_direct: lamp_mask is required (the media's boundary spheres would shadow every segment)")
    return _media_loop(ctx, "trace_media_direct", rays, rng, max_depth, sky, mask, free_flight, True,
                       (emission, lamp_mask, transmit, strategy))


def _media_loop(ctx, who, rays, rng, max_depth, sky, mask, free_flight, phase, direct):
    """The loop of trace_media and trace_media_direct; direct: None, or (emission, lamp_mask, transmit, strategy).  Without
    `phase` and `direct` every launch and every bit is trace_media's as it was before either existed, and without a density
    grid (K = len(ctx.media_grids()) == 0) every launch and every bit is as it was before grids existed."""
    import torch
    p = _Paths.from_rays(ctx, who, rays, rng, None)
    n, dev, work, color, att = p.n, p.dev, p.work, p.color, p.att
    inf = torch.full((n,), float("inf"), dtype=torch.float64, device=dev)
    t_range = torch.zeros((n, 2), dtype=torch.float64, device=dev)
    grids = ctx.media_grids()      # the media with a density grid (set_media_grid), ascending; none: every launch as it was
    K = len(grids)
    u = torch.zeros((n, 1 + K), dtype=torch.float64, device=dev)
    march, nxt = None, None
    flight = (lambda x: -torch.log1p(-x)) if free_flight is None else \
        (lambda x: torch.as_tensor(free_flight(x), dtype=torch.float64).to(dev).reshape(n))
    if K:
        grid_range = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        gm, gseg = [None] * K, [None] * K
    if direct is not None:
        emission, lamp_mask, transmit, strategy = direct
        emission = _colours(emission, dev)
        lrng = _light_states(p.entry())
        points = torch.zeros((n, 4), dtype=torch.float64, device=dev)
        shadow_range = torch.empty((n, 2), dtype=torch.float64, device=dev)
        shadow_range[:, 0], shadow_range[:, 1] = 0.001, 1.0
        seg_range = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        seg_range[:, 1] = 1.0
        after_collision = torch.zeros((n,), dtype=torch.bool, device=dev)   # the path's previous vertex was a medium collision
        ls, occ, seg, ev = None, None, None, None
    for step in p.steps(max_depth):
        live = p.live
        hit = ctx.hit(work, time_range=p.tr, mask=mask(step) if callable(mask) else mask)
        u, p.rng = ctx.uniform(p.rng, 1 + K, index=live, out=u)
        tau = flight(u[:, 0])
        t_range[:, 1] = torch.where(hit.object >= 0, hit.t, inf)
        march = ctx.march_media(work, tau, t_range, index=live, out=march)
        idx = live.long()
        if K:   # one budget per grid medium; each march runs up to the earliest collision so far (or the hit) and replaces it
            listed = torch.zeros((n,), dtype=torch.bool, device=dev)
            listed[idx] = True
            w_status, w_t, w_active = march.status.clone(), march.t.clone(), march.active.clone()
            for j, m in enumerate(grids):
                grid_range[:, 1] = torch.where(w_status == MEDIA_COLLIDED, w_t, t_range[:, 1])
                gm[j] = ctx.march_media_grid(work, flight(u[:, 1 + j].contiguous()), m, grid_range, index=live, out=gm[j])
                won = listed & (gm[j].status == MEDIA_COLLIDED)
                w_status = torch.where(won, gm[j].status, w_status)
                w_t = torch.where(won, gm[j].t, w_t)
                w_active = torch.where(won, gm[j].active, w_active)
            # (the winner's status, t and active -- all that is read below; depth and rho stay the HOMOGENEOUS march's, not the winner's)
            march_h, march = march, MediaMarch(w_status, w_t, march.depth, w_active, march.rho, "")
        st, obj = march.status[idx], hit.object[idx]
        collided = live[st == MEDIA_COLLIDED]
        surface = live[(st == MEDIA_ESCAPED) & (obj >= 0)]
        missed = idx[(st == MEDIA_ESCAPED) & (obj < 0)]
        alive = torch.zeros((n,), dtype=torch.bool, device=dev)
        lit = color[missed].clone() if direct is not None and missed.numel() else None   # what the light samples have added
        if sky is not None:
            p.caller_sky(sky, missed)
        elif missed.numel():   # (Context.sky on the list of the misses, not on every stepped ray as trace() asks it)
            color[missed] = ctx.sky(work, missed.int())[missed] * att[missed]
        if lit is not None:    # (a path's sky is its only colour without lamps, and is assigned; with them it is added)
            color[missed] = lit + color[missed]
        if surface.numel():
            if direct is not None:   # emission found by hitting it, unless the light sample at a collision has counted it
                si = surface.long()
                found = att[si] * emission[hit.object[si].long()]
                color[si] = color[si] + torch.where(after_collision[si][:, None], torch.zeros_like(found), found)
            res = ctx.scatter(work, hit, p.rng, index=surface)
            si = surface.long()
            sc = si[res.status[si] == BOUNCE_SCATTERED]
            att[sc] = att[sc] * res.attenuation[sc]
            alive[sc] = True
            if direct is not None:
                after_collision[sc] = False
        if collided.numel():
            nxt = (ctx.sample_phase if phase else ctx.scatter_media)(work, march, p.rng, index=collided, out=nxt)
            ci = collided.long()
            if direct is not None:
                after_collision[ci] = True
                if step != int(max_depth) - 1:   # the light sample at the collision; `work` still holds the incoming rays
                    points[ci, 0:3], points[ci, 3] = nxt.rays[ci, 0:3], nxt.rays[ci, 6]
                    ls = ctx.sample_lights(points, lrng, collided, strategy, out=ls)
                    occ = ctx.occluded(ls.rays, shadow_range, collided, p.tr, "auto", out=occ, mask=lamp_mask)
                    seg = ctx.march_media(ls.rays, inf, seg_range, index=collided, out=seg)
                    depth = seg.depth[ci]
                    for j, m in enumerate(grids):   # the depths of a shadow segment add, in ascending medium order
                        gseg[j] = ctx.march_media_grid(ls.rays, inf, m, seg_range, index=collided, out=gseg[j])
                        depth = depth + gseg[j].depth[ci]
                    T = torch.exp(-depth) if transmit is None else \
                        torch.as_tensor(transmit(depth), dtype=torch.float64).to(dev).reshape(-1)
                    ev = ctx.phase(work, march.active, ls.rays, collided, out=ev)
                    pdf, lamp = ls.pdf[ci], ls.light[ci].long()
                    ok = (~occ.occluded[ci]) & (lamp >= 0) & (pdf > 0) & torch.isfinite(pdf)
                    add = att[ci] * ev.value[ci] * emission[lamp.clamp(min=0)] * (T / pdf)[:, None]
                    color[ci] = color[ci] + torch.where(ok[:, None], add, torch.zeros_like(add))
            work[ci] = nxt.rays[ci]
            att[ci] = att[ci] * nxt.attenuation[ci]
            alive[ci] = True
        if K:
            march = march_h   # (the homogeneous march's buffers are written again next iteration)
        p.live = torch.nonzero(alive).reshape(-1).int()
    return p.finish(color)[:2]
