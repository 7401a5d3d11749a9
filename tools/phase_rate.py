#!/usr/bin/env python3
"""Rates of the Henyey-Greenstein sampler (tor_phase_sample_device) against what a host does without it -- uniform(rng, 3) and the
definition of include/tor_phase.h written in torch -- on the same device arrays in one process: M rays/s per table size.  2^20
rays with seeded directions; tables of 1, 8 and 64 media (g cycling through 0.3, -0.7, 0.99, 0, ...), active words of one medium
(the table of 1) or of one to three seeded media (as overlapping boundaries give them).

The composition is timed for the table of one medium only, where torch needs no table walk: the mixture of one medium is that
medium.  Legs, interleaved per round between HIP events:
    compose    tor_rng_uniform_device (3 draws) -- of the library --parent-lib names (the parent commit's build, loaded next to
               this one with a context of its own), else of this build -- and the torch arithmetic: inversion, clamp, azimuth
               (torch.sin / torch.cos: not the library's bits), the frame of Duff et al., the direction, hg, attenuation, pdf
    sample_a   one tor_phase_sample_device launch into outputs allocated before the timing
    sample_b   sample_a again: the run-to-run spread
    scatter    tor_media_scatter_device of this build on the same operands (two draws, no phase function): the second reference
    eval       tor_phase_eval_device on the sampled rays
Every leg starts from the same states (copied back before each run, outside no leg: the copy is part of every leg alike).  WARM
warm-up runs, then ROUNDS timings of REPS back-to-back runs; the median over the rounds.  No ratio is fixed in advance: a win is
claimed only where sample / compose lies above 1 by more than the spread between repeated legs of either, a loss is said plainly.
The two answers must agree: directions within 1e-12, pdf within 1e-9 relative (torch's sin / cos are not the portable pair's
bits).  Each table runs in a child process under --step-timeout; the first that fails or runs past it ends the run.  Writes the
table to --out and prints one JSON line.

    python tools/phase_rate.py [--parent-lib /path/to/parent/libtor_mi355x.so] [--reps 2] [--rounds 5] [--warm 1]
                               [--step-timeout 180] [--out profiles/phase_rate.txt]
"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")
MEDIA = (1, 8, 64)
G_CYCLE = (0.3, -0.7, 0.99, 0.0, -0.99, 2.0 ** -20)
FOUR_PI, TWO_PI = 4.0 * 3.141592653589793, 2.0 * 3.141592653589793


class ParentUniform:
    """tor_rng_uniform_device of another build of the library (the parent commit's), on a context of its own."""

    def __init__(self, path):
        self.L = C.CDLL(os.path.abspath(path))
        self.L.tor_last_error.restype = C.c_char_p
        self.L.tor_context_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
        self.L.tor_context_destroy.argtypes = [C.c_void_p]
        tor._bind(self.L, ("tor_rng_uniform_device",))
        self.h = C.c_void_p()
        self._ok(self.L.tor_context_create(-1, C.byref(self.h)))

    def _ok(self, rc):
        if rc != 0:
            raise SystemExit("phase_rate: parent library: " + self.L.tor_last_error().decode("utf-8", "replace"))

    def uniform(self, rng, out):
        stream = torch.cuda.current_stream().cuda_stream
        self._ok(self.L.tor_rng_uniform_device(self.h, int(rng.shape[0]), C.c_void_p(rng.data_ptr()), C.c_void_p(0), int(rng.shape[0]), 3,
                                               C.c_void_p(out.data_ptr()), C.c_void_p(stream)))

    def close(self):
        self.L.tor_context_destroy(self.h)


def table(n_media):
    """One surface sphere and n_media boundary spheres; (records, objects, sigma, albedo, g)."""
    g = np.random.default_rng(20261020 + n_media)
    recs = np.zeros((n_media + 1, 16))
    recs[:, 8], recs[:, 9], recs[:, 11:14] = 1.0, 1.0, 0.5
    c = g.uniform(-3, 3, (n_media + 1, 3))
    recs[:, 1:4], recs[:, 4:7] = c, c
    return (recs, np.arange(1, n_media + 1, dtype=np.int32), g.uniform(0.05, 0.5, n_media), g.uniform(0.2, 1.0, (n_media, 3)),
            np.asarray([G_CYCLE[m % len(G_CYCLE)] for m in range(n_media)]))


def compose_one(u, rays, t, g, sigma, albedo):
    """The definition for a table of ONE medium, in torch: (rays_out (n, 7), att (n, 3), pdf (n,))."""
    d = rays[:, 3:6]
    ii = (d * d).sum(dim=1)
    if g == 0.0:
        mu = 1.0 - 2.0 * u[:, 1]
    else:
        gg = g * g
        s = (1.0 - gg) / ((1.0 - g) + (2.0 * g) * u[:, 1])
        mu = ((1.0 + gg) - s * s) / (2.0 * g)
    mu = mu.clamp(-1.0, 1.0)
    st = torch.sqrt((1.0 - mu * mu).clamp(min=0.0))
    phi = u[:, 2] * TWO_PI
    sp, cp = torch.sin(phi), torch.cos(phi)
    w = d * (1.0 / torch.sqrt(ii))[:, None]
    sg = torch.copysign(torch.ones_like(ii), w[:, 2])
    a = -1.0 / (sg + w[:, 2])
    b = (w[:, 0] * w[:, 1]) * a
    b1 = torch.stack([1.0 + ((sg * w[:, 0]) * w[:, 0]) * a, sg * b, -(sg * w[:, 0])], dim=1)
    b2 = torch.stack([b, sg + (w[:, 1] * w[:, 1]) * a, -w[:, 1]], dim=1)
    v = ((st * cp)[:, None] * b1 + (st * sp)[:, None] * b2) + mu[:, None] * w
    den = (1.0 + g * g) - (2.0 * g) * mu
    p = (1.0 - g * g) / (FOUR_PI * (den * torch.sqrt(den)))
    out = torch.empty_like(rays)
    out[:, 0:3], out[:, 3:6], out[:, 6] = rays[:, 0:3] + t[:, None] * d, v, rays[:, 6]
    q = sigma * p
    att = (sigma * albedo)[None, :] * p[:, None] / q[:, None]
    return out, att, q / sigma


def rate_rows(a, n_media):
    """The row of one table size: runs in a child process (main's --row) and prints it as one ROW line."""
    if not torch.cuda.is_available():
        sys.exit("phase_rate: no GPU -- a rate is measured on the device or not at all")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261020 + n_media)
    recs, objects, sigma, albedo, gs = table(n_media)
    ctx = tor.Context()
    ctx.upload(tor.Scene.from_records(recs).list())
    ctx.set_media(objects, sigma, albedo)
    ctx.set_media_phase(gs)
    n = a.rays
    rays = torch.randn((n, 7), dtype=torch.float64, device="cuda", generator=gen)
    t = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    if n_media == 1:
        active = torch.ones(n, dtype=torch.int64, device="cuda")
    else:
        bits = torch.randint(0, n_media, (n, 3), device="cuda", generator=gen)
        keep = torch.rand((n, 3), device="cuda", generator=gen) < torch.tensor([1.0, 0.5, 0.25], device="cuda")
        active = torch.zeros(n, dtype=torch.int64, device="cuda")
        for k in range(3):
            active |= torch.where(keep[:, k], torch.ones_like(active) << bits[:, k], torch.zeros_like(active))
    states0 = torch.from_numpy(tor.rng_seed2(np.arange(n) // 1024, np.arange(n) % 1024).view(np.int64)).cuda()
    states = states0.clone()
    parent = ParentUniform(a.parent_lib) if a.parent_lib and n_media == 1 else None
    u = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    s1, al1 = float(sigma[0]), torch.from_numpy(albedo[0]).cuda()

    def compose():
        states.copy_(states0)
        if parent is not None:
            parent.uniform(states, u)
        else:
            ctx.uniform(states, 3, out=u)
        return compose_one(u, rays, t, float(gs[0]), s1, al1)

    states.copy_(states0)
    ps = ctx.sample_phase(rays, (t, active), states)
    states.copy_(states0)
    sc = ctx.scatter_media(rays, (t, active), states)
    ev = ctx.phase(rays, active, ps.rays)

    def sample():
        states.copy_(states0)
        return ctx.sample_phase(rays, (t, active), states, out=ps)

    def scatter():
        states.copy_(states0)
        return ctx.scatter_media(rays, (t, active), states, out=sc)

    legs = {"sample_a": sample, "sample_b": sample, "scatter": scatter, "eval": lambda: ctx.phase(rays, active, ps.rays, out=ev)}
    if n_media == 1:
        legs = {"compose_a": compose, "compose_b": compose, **legs}
    order = list(legs)
    for leg in order:
        for _ in range(a.warm):
            legs[leg]()
    dir_err = pdf_err = None
    if n_media == 1:
        want = sample()
        got = compose()
        torch.cuda.synchronize()
        dir_err = float((got[0][:, 3:6] - want.rays[:, 3:6]).abs().max())
        pdf_err = float(((got[2] - want.pdf).abs() / want.pdf).max())
    ms = {leg: [] for leg in order}
    for _ in range(a.rounds):
        for leg in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                legs[leg]()
            e1.record()
            torch.cuda.synchronize()
            ms[leg].append(e0.elapsed_time(e1) / a.reps)
    rate = {leg: n / (statistics.median(ms[leg]) * 1e-3) / 1e6 for leg in order}
    spread = abs(rate["sample_a"] - rate["sample_b"]) / max(rate["sample_a"], rate["sample_b"])
    row = {"device": torch.cuda.get_device_name(0), "media": n_media, "rays": n,
           "active_per_ray": round(float(sum(((active >> m) & 1).double().mean() for m in range(n_media))), 3),
           "mrays_s": {k: round(v, 1) for k, v in rate.items()}, "sample_spread": round(spread, 4)}
    if n_media == 1:
        cspread = abs(rate["compose_a"] - rate["compose_b"]) / max(rate["compose_a"], rate["compose_b"])
        ratio = min(rate["sample_a"], rate["sample_b"]) / max(rate["compose_a"], rate["compose_b"])
        both = max(spread, cspread)
        row.update(compose_spread=round(cspread, 4), sample_vs_compose=round(ratio, 2), dir_err=dir_err, pdf_rel_err=pdf_err,
                   verdict="win" if ratio > 1.0 + both else ("LOSS" if ratio < 1.0 - both else "within the spread"))
    if parent is not None:
        parent.close()
    ctx.close()
    print("ROW " + json.dumps([row]))
    return 0


def child(args, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"phase_rate: {what} ran past {limit} s -- stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"phase_rate: {what} failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="libtor_mi355x.so built from the parent commit: the compose leg's uniforms run on it")
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds the row of one table size may take")
    ap.add_argument("--row", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_rate.txt"))
    a = ap.parse_args()
    if a.row:
        return rate_rows(a, a.row)
    common = ["--rays", str(a.rays), "--reps", str(a.reps), "--rounds", str(a.rounds), "--warm", str(a.warm)]
    if a.parent_lib:
        common += ["--parent-lib", a.parent_lib]
    rows = []
    for n_media in MEDIA:   # each GPU step under its own limit; stop at the first that fails
        rc, got = child(["--row", str(n_media)] + common, a.step_timeout, f"the table of {n_media} media")
        if rc:
            return rc
        rows += got
    lines = [f"phase_rate: M rays/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events; {rows[0]['rays']} rays; "
             f"{rows[0]['device']}; the compose leg's uniforms: {'the parent build' if a.parent_lib else 'this build'}",
             f"{'media':>5}{'active':>8}{'compose':>9}{'again':>9}{'sample':>9}{'again':>9}{'spread':>8}{'s/c':>7}{'scatter':>9}{'eval':>9}"
             f"  verdict            dir err   pdf rel err"]
    for r in rows:
        g = r["mrays_s"]
        one = r["media"] == 1
        lines.append(f"{r['media']:>5}{r['active_per_ray']:>8.2f}" + (f"{g['compose_a']:>9.1f}{g['compose_b']:>9.1f}" if one else f"{'-':>9}{'-':>9}")
                     + f"{g['sample_a']:>9.1f}{g['sample_b']:>9.1f}{r['sample_spread']:>8.3f}" + (f"{r['sample_vs_compose']:>7.2f}" if one else f"{'-':>7}")
                     + f"{g['scatter']:>9.1f}{g['eval']:>9.1f}" + (f"  {r['verdict']:<18} {r['dir_err']:.2e}  {r['pdf_rel_err']:.2e}" if one else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "phase_rate", "unit": "M rays/s", "reps": a.reps, "rounds": a.rounds, "warm": a.warm,
                      "parent_lib": bool(a.parent_lib), "rows": rows}))
    ok = all(r["media"] != 1 or (r["dir_err"] <= 1e-12 and r["pdf_rel_err"] <= 1e-9) for r in rows)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
