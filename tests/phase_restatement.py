"""An independent restatement of the phase-function queries (include/tor_phase.h): the Henyey-Greenstein sampler, its evaluation
twin, and the wavefront loops built from them (what Context.trace_media(phase=True) and Context.trace_media_direct run).

Every row is computed in scalar float64 (Python floats: single IEEE roundings, never fused; math.sqrt is correctly rounded), one
operation per line of the header, over ALL media of the table in a plain counted loop (no union of a wave: what the kernel skips
must not matter).  The uniforms come from the CPU oracle's exported generator (oracle_rng_uniform01) and the azimuth's sin / cos from
its portable pair (oracle_port_sincos), as media_restatement.scatter takes them.  It shares no code with the library.  `variant`
names a deliberately wrong restatement (VARIANTS): the CPU suite shows which named input tells each apart."""
import math

import numpy as np

import media_restatement as MR
import radiance_restatement as RR

PI = 3.141592653589793
FOUR_PI = 4.0 * PI
TWO_PI = 2.0 * PI
G_MAX, G_MIN = 0.99, 2.0 ** -20
INF = math.inf

VARIANTS = ("no_clamp", "x_le_acc", "no_fallback", "descending", "no_copysign", "mu_from_dot")


def clamp1(x):
    if x > 1.0:
        return 1.0
    if x < -1.0:
        return -1.0
    return x


def dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def hg(g, mu):
    g2 = g * g
    den = (1.0 + g2) - (2.0 * g) * mu
    return (1.0 - g2) / (FOUR_PI * (den * math.sqrt(den)))


def _bits_of(A, M, descending=False):
    ms = [m for m in range(M) if (A >> m) & 1]
    return ms[::-1] if descending else ms


def mixture(sigma, albedo, gs, A, mu, descending=False):
    """(rho, q, n): the header's mixture(active, mu) over the table of M = len(sigma) media."""
    rho, q, n = 0.0, 0.0, [0.0, 0.0, 0.0]
    for m in _bits_of(A, len(sigma), descending):
        p = hg(gs[m], mu)
        rho = rho + sigma[m]
        q = q + sigma[m] * p
        n = [n[c] + (sigma[m] * albedo[m][c]) * p for c in range(3)]
    return rho, q, n


def _usable(xx):
    return xx > 0 and xx != INF


def eval_row(sigma, albedo, gs, d_in, A, d_out, variant=None):
    """One item of tor_phase_eval_device: (value [3], pdf)."""
    M = len(sigma)
    ii, oo = dot(d_in, d_in), dot(d_out, d_out)
    if not _usable(ii) or not _usable(oo) or A == 0 or (A >> M) != 0:
        return [0.0, 0.0, 0.0], 0.0
    fi, fo = 1.0 / math.sqrt(ii), 1.0 / math.sqrt(oo)
    w = [d_in[c] * fi for c in range(3)]
    v = [d_out[c] * fo for c in range(3)]
    mu = dot(w, v)
    if variant != "no_clamp":
        mu = clamp1(mu)
    rho, q, n = mixture(sigma, albedo, gs, A, mu, variant == "descending")
    if not rho > 0:
        return [0.0, 0.0, 0.0], 0.0
    return [n[c] / rho for c in range(3)], q / rho


def cosine(g, u_cos, variant=None):
    """The header's cosine line: (mu after the clamp, mu before it)."""
    if g == 0:
        raw = 1.0 - 2.0 * u_cos
    else:
        gg = g * g
        s = (1.0 - gg) / ((1.0 - g) + (2.0 * g) * u_cos)
        raw = ((1.0 + gg) - s * s) / (2.0 * g)
    return (raw if variant == "no_clamp" else clamp1(raw)), raw


def select(sigma, A, u_sel, rho, variant=None):
    """The header's selection: (chosen, whether the fallback decided)."""
    x = u_sel * rho
    acc, chosen, last = 0.0, -1, -1
    for m in _bits_of(A, len(sigma), variant == "descending"):
        acc = acc + sigma[m]
        if sigma[m] > 0:
            last = m
        if chosen < 0 and (x <= acc if variant == "x_le_acc" else x < acc):
            chosen = m
    fell = chosen < 0
    if fell and variant != "no_fallback":
        chosen = last
    return chosen, fell


def frame(w, variant=None):
    sg = 1.0 if variant == "no_copysign" else math.copysign(1.0, w[2])
    a = -1.0 / (sg + w[2])
    b = (w[0] * w[1]) * a
    b1 = [1.0 + ((sg * w[0]) * w[0]) * a, sg * b, -(sg * w[0])]
    b2 = [b, sg + (w[1] * w[1]) * a, -w[1]]
    return b1, b2


ZERO_ROW = ([0.0] * 7, [0.0] * 3, 0.0)


def sample_row(sigma, albedo, gs, ray, t, A, u_sel, u_cos, u_phi, sincos, variant=None, detail=None):
    """One ray of tor_phase_sample_device from its three uniforms: (out ray [7], att [3], pdf).  sincos(phi) -> (sin, cos), the
    portable pair.  detail: a dict that receives chosen, fell, mu, raw (the cosine before the clamp) and b1."""
    M = len(sigma)
    o, d = ray[0:3], ray[3:6]
    ii = dot(d, d)
    desc = variant == "descending"
    rho = 0.0
    for m in _bits_of(A, M, desc):
        rho = rho + sigma[m]
    if A == 0 or (A >> M) != 0 or not rho > 0 or not _usable(ii):
        return ZERO_ROW
    chosen, fell = select(sigma, A, u_sel, rho, variant)
    if chosen < 0:                                                  # (only the no_fallback variant gets here)
        return ZERO_ROW
    mu, raw = cosine(gs[chosen], u_cos, variant)
    r2 = 1.0 - mu * mu
    if not r2 > 0:
        r2 = 0.0
    st = math.sqrt(r2)
    phi = u_phi * TWO_PI
    sp, cp = sincos(phi)
    f = 1.0 / math.sqrt(ii)
    w = [d[c] * f for c in range(3)]
    if variant == "no_copysign" and 1.0 + w[2] == 0.0:              # the frame of Frisvad without the sign: singular at -z
        return ZERO_ROW
    b1, b2 = frame(w, variant)
    v = [((st * cp) * b1[c] + (st * sp) * b2[c]) + mu * w[c] for c in range(3)]
    if variant == "mu_from_dot":
        mu = clamp1(dot(w, v))
    rho2, q, n = mixture(sigma, albedo, gs, A, mu, desc)
    if detail is not None:
        detail.update(chosen=chosen, fell=fell, mu=mu, raw=raw, b1=b1, w=w, v=v)
    if not q > 0:
        return ZERO_ROW
    return [o[c] + t * d[c] for c in range(3)] + v + [ray[6]], [n[c] / q for c in range(3)], q / rho


def _table(sigma, albedo, gs):
    sigma = [float(s) for s in np.asarray(sigma, dtype=np.float64).reshape(-1)]
    M = len(sigma)
    albedo = [[1.0] * 3] * M if albedo is None else np.asarray(albedo, dtype=np.float64).reshape(M, 3).tolist()
    gs = [0.0] * M if gs is None else [float(g) for g in np.asarray(gs, dtype=np.float64).reshape(-1)]
    assert len(gs) == M
    return sigma, albedo, gs


def _words(active, n):
    a = np.asarray(active)
    a = a.view(np.uint64) if a.dtype.itemsize == 8 and a.dtype.kind in "iu" else a.astype(np.uint64)
    return [int(v) for v in a.reshape(n)]


def sample(oracle, sigma, albedo, gs, rays, t, active, states, index=None, into=None, variant=None, details=None):
    """tor_phase_sample_device for the listed rays: a dict of rays (n, 7), attenuation (n, 3), pdf (n,) and states (n, 4) uint64;
    rays that are not listed keep what `into` holds (else 0) and their state."""
    L = oracle.lib()
    sigma, albedo, gs = _table(sigma, albedo, gs)
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = rays.shape[0]
    t = np.asarray(t, dtype=np.float64).reshape(n)
    A = _words(active, n)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    new = np.zeros((n, 7)) if into is None else np.array(into["rays"])
    att = np.zeros((n, 3)) if into is None else np.array(into["attenuation"])
    pdf = np.zeros(n) if into is None else np.array(into["pdf"])
    sincos = lambda phi: MR._sincos(L, phi)
    for i in MR._listed(index, n):
        g = RR._ptr(st, i)
        u_sel, u_cos, u_phi = L.oracle_rng_uniform01(g), L.oracle_rng_uniform01(g), L.oracle_rng_uniform01(g)   # always three
        detail = None if details is None else details.setdefault(int(i), dict(u=(u_sel, u_cos, u_phi)))
        new[i], att[i], pdf[i] = sample_row(sigma, albedo, gs, rays[i].tolist(), float(t[i]), A[i], u_sel, u_cos, u_phi, sincos,
                                            variant, detail)
    return {"rays": new, "attenuation": att, "pdf": pdf, "states": st}


def evaluate(sigma, albedo, gs, rays_in, active, rays_out, index=None, into=None, variant=None):
    """tor_phase_eval_device for the listed items: a dict of value (n, 3) and pdf (n,)."""
    sigma, albedo, gs = _table(sigma, albedo, gs)
    rays_in = np.asarray(rays_in, dtype=np.float64).reshape(-1, 7)
    rays_out = np.asarray(rays_out, dtype=np.float64).reshape(-1, 7)
    n = rays_in.shape[0]
    A = _words(active, n)
    value = np.zeros((n, 3)) if into is None else np.array(into["value"])
    pdf = np.zeros(n) if into is None else np.array(into["pdf"])
    for i in MR._listed(index, n):
        value[i], pdf[i] = eval_row(sigma, albedo, gs, rays_in[i, 3:6].tolist(), A[i], rays_out[i, 3:6].tolist(), variant)
    return {"value": value, "pdf": pdf}


def mismatches(got, want, rows=slice(None), keys=("rays", "attenuation", "pdf")):
    """What differs between two sample (or, with keys value / pdf, evaluation) results, bit for bit."""
    bad = []
    for k in keys:
        same = MR.same_bits(np.asarray(got[k])[rows], np.asarray(want[k])[rows])
        if not same.all():
            rows_bad = np.nonzero(~same.reshape(same.shape[0], -1).all(axis=1))[0]
            bad.append(f"{k}: {rows_bad.size} rows, first {int(rows_bad[0])}")
    if "states" in want and "states" in got:
        gs_ = np.ascontiguousarray(got["states"]).view(np.uint64).reshape(-1, 4)[rows]
        if not np.array_equal(gs_, want["states"][rows]):
            bad.append("states")
    return bad


def trace(oracle, recs, objects, sigma, albedo, gs, rays, states, max_depth, free_flight, direct=None):
    """The wavefront loop of Context.trace_media(phase=True) -- media_restatement.trace with the phase sampler at the collisions --
    and, with direct = dict(emission (n_objects, 3), lights = (objects, weights), groups, lamp_mask, transmit, strategy,
    light_sample, occluded), of Context.trace_media_direct.  light_sample(points (n, 4), light states, index) -> dict(rays, pdf,
    light, states) and occluded(rays (n, 7), t_range (n, 2), index) -> (n,) bool are the caller's restatements of sample_lights
    and of occluded() under the lamp mask.  Returns (color (n, 3), states (n, 4) uint64)."""
    import bounce_restatement as BR
    import hit_restatement as H
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays = np.array(rays, dtype=np.float64).reshape(-1, 7)
    st = np.ascontiguousarray(np.array(states).view(np.uint64).reshape(-1, 4)).copy()
    n = rays.shape[0]
    surf = np.array([j for j in range(len(recs)) if j not in set(int(o) for o in objects)], dtype=np.int64)
    color, att = np.zeros((n, 3)), np.ones((n, 3))
    live = np.arange(n)
    if direct is not None:
        emission = np.asarray(direct["emission"], dtype=np.float64).reshape(-1, 3)
        lst = direct["light_states"]
        after_collision = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for step in range(max_depth):
            if live.size == 0:
                break
            raw = np.zeros((n, 8))
            raw.view(np.int32)[:, 14] = -1
            if surf.size:
                sub = H.world_hit(recs[surf], rays[live])
                w = sub.view(np.int32)
                w[:, 14] = np.where(w[:, 14] >= 0, surf[np.maximum(w[:, 14], 0)], -1)
                raw[live] = sub
            hit = H.fields(raw)
            u, st = MR.uniforms(oracle, st, 1, live)
            tau = np.asarray(free_flight(u[:, 0]), dtype=np.float64)
            tr = np.zeros((n, 2))
            tr[:, 1] = np.where(hit["object"] >= 0, hit["t"], np.inf)
            m = MR.march(recs, objects, sigma, rays, tau, tr, live)
            status, obj = m["status"][live], hit["object"][live]
            collided = live[status == MR.COLLIDED]
            surface = live[(status == MR.ESCAPED) & (obj >= 0)]
            missed = live[(status == MR.ESCAPED) & (obj < 0)]
            alive = np.zeros(n, dtype=bool)
            if missed.size:
                sk = BR.sky(rays, missed)[missed] * att[missed]
                color[missed] = sk if direct is None else color[missed] + sk
            if surface.size:
                if direct is not None:
                    found = att[surface] * emission[hit["object"][surface]]
                    color[surface] = color[surface] + np.where(after_collision[surface][:, None], 0.0, found)
                res = BR.scatter(oracle, recs, rays, raw, st, surface)
                rays, st = res["rays"], res["states"]
                sc = surface[res["status"][surface] == BR.SCATTERED]
                att[sc] = att[sc] * res["attenuation"][sc]
                alive[sc] = True
                if direct is not None:
                    after_collision[sc] = False
            if collided.size:
                res = sample(oracle, sigma, albedo, gs, rays, m["t"], m["active"], st, collided)
                st = res["states"]
                if direct is not None:
                    after_collision[collided] = True
                    if step != max_depth - 1:
                        points = np.zeros((n, 4))
                        points[collided, 0:3], points[collided, 3] = res["rays"][collided, 0:3], res["rays"][collided, 6]
                        ls = direct["light_sample"](points, lst, collided)
                        lst = ls["states"]
                        sr = np.zeros((n, 2))
                        sr[:, 0], sr[:, 1] = 0.001, 1.0
                        blocked = direct["occluded"](ls["rays"], sr, collided)
                        zr = np.zeros((n, 2))
                        zr[:, 1] = 1.0
                        depth = MR.march(recs, objects, sigma, ls["rays"], np.inf, zr, collided)["depth"][collided]
                        T = np.asarray(direct["transmit"](depth), dtype=np.float64)
                        ev = evaluate(sigma, albedo, gs, rays, m["active"], ls["rays"], collided)
                        pdf, lamp = ls["pdf"][collided], ls["light"][collided].astype(np.int64)
                        ok = (~blocked[collided]) & (lamp >= 0) & (pdf > 0) & np.isfinite(pdf)
                        add = att[collided] * ev["value"][collided] * emission[np.maximum(lamp, 0)] * (T / pdf)[:, None]
                        color[collided] = color[collided] + np.where(ok[:, None], add, 0.0)
                rays[collided] = res["rays"][collided]
                att[collided] = att[collided] * res["attenuation"][collided]
                alive[collided] = True
            live = np.nonzero(alive)[0]
    return color, st
