#!/usr/bin/env python3
"""Rates of the direct-light sampling query (tor_light_sample_device) against what a host does without it -- the same arithmetic
as a batched torch float64 computation over n_points x n_lights on the same device (the generator's three draws in int64 tensor
arithmetic, centres, solid-angle measures, a cumulative sum per point, the pick, the cone sample), chunked to fit memory: M points/s
for 1, 16, 256 and 4096 lights and both strategies.  Scene: that many spheres in a box, every eighth one moving, random weights;
points uniform in the box.  Legs, interleaved per round between HIP events: the library (one launch into outputs allocated before
the timing; the states are written again and again) and torch.  Every leg: WARM warm-up runs, then ROUNDS timings of REPS
back-to-back runs; the median over the rounds.  The torch leg's cumulative sum is not sequential, so its total may differ from the
library's in the last bits: the tool counts the points whose pick or density differ and reports them; where the pick agrees the
densities are compared to 1e-12 relative.  Nothing here fixes a ratio: the expectation printed with the table is arithmetic.

Each light count runs in a child process of its own under a time limit; the run stops at the first child that fails.

    python tools/light_sample_rate.py [--points 1048576] [--reps 2] [--rounds 5] [--warm 1] [--out profiles/light_sample_rate.txt]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

LIGHTS = (1, 16, 256, 4096)
STRATEGIES = ("weight", "solid_angle")
PAIRS_PER_CHUNK = 1 << 24        # n x L float64 temporaries of 128 MiB
TWO_PI = 2.0 * 3.141592653589793


def scene_records(n_lights, rs):
    recs = np.zeros((n_lights, 16))
    recs[:, 1:4] = rs.uniform(-8.0, 8.0, size=(n_lights, 3))
    recs[:, 4:7] = recs[:, 1:4]
    moving = np.arange(n_lights) % 8 == 3
    recs[moving, 0] = 1.0
    recs[moving, 5] += 0.5
    recs[:, 8] = 1.0
    recs[:, 9] = rs.uniform(0.1, 0.5, size=n_lights)
    recs[:, 11:14] = 0.5
    recs[:, 15] = 1.5
    return recs


def torch_draws(torch, st):
    """Three uniform01 of xoshiro256+ (support/rng.nim:58-74, 129-133) per row of the (n, 4) int64 states, in tensor arithmetic."""
    def lsr(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)

    s0, s1, s2, s3 = (st[:, k].clone() for k in range(4))
    us = []
    for _ in range(3):
        out = s0 + s3
        t = s1 << 17
        s2 = s2 ^ s0
        s3 = s3 ^ s1
        s1 = s1 ^ s2
        s0 = s0 ^ s3
        s2 = s2 ^ t
        s3 = (s3 << 45) | lsr(s3, 19)
        us.append((lsr(out, 12) | 0x3FF0000000000000).view(torch.float64) - 1.0)
    return us, torch.stack((s0, s1, s2, s3), dim=1)


def torch_sample(torch, recs, weights, pts, st, solid):
    """The n x L matrix a host writes today: (pick (n,), pdf (n,), rays (n, 7), states)."""
    kind, c0, c1, t0, t1 = recs[None, :, 0], recs[None, :, 1:4], recs[None, :, 4:7], recs[None, :, 7], recs[None, :, 8]
    R2 = (recs[:, 9].abs() * recs[:, 9].abs())[None, :]
    nl = recs.shape[0]
    chunk = max(1, PAIRS_PER_CHUNK // nl)
    (u0, u1, u2), st2 = torch_draws(torch, st)
    picks, pdfs, rays = [], [], []
    for lo in range(0, int(pts.shape[0]), chunk):
        p, time = pts[lo:lo + chunk, None, 0:3], pts[lo:lo + chunk, None, 3]
        f = (time - t0) / (t1 - t0)
        c = torch.where((kind != 0)[:, :, None], c0 + (c1 - c0) * f[:, :, None], c0)
        w = c - p
        d2 = w[:, :, 0] * w[:, :, 0] + w[:, :, 1] * w[:, :, 1] + w[:, :, 2] * w[:, :, 2]
        inside = ~(d2 > R2)
        s2 = R2 / d2
        m = torch.where(inside, torch.full_like(s2, 2.0), s2 / (1.0 + torch.sqrt(1.0 - s2)))
        imp = weights[None, :] * m if solid else weights[None, :].expand_as(m)
        runs = torch.cumsum(imp, dim=1)
        T = runs[:, -1]
        x = u0[lo:lo + chunk] * T
        above = (imp > 0) & (runs > x[:, None])
        pick = torch.argmax(above.to(torch.int8), dim=1)
        rows = torch.arange(pick.shape[0], device=pick.device)
        mp, d2p, wp, ins = m[rows, pick], d2[rows, pick], w[rows, pick], inside[rows, pick]
        P = imp[rows, pick] / T
        k = u1[lo:lo + chunk] * mp
        cos_t, sin2 = 1.0 - k, k * (2.0 - k)
        sin_t = torch.sqrt(sin2)
        ang = u2[lo:lo + chunk] * TWO_PI
        s, cs = torch.sin(ang), torch.cos(ang)
        sd = torch.sqrt(d2p)
        a = wp * (1.0 / sd)[:, None]
        sg = torch.copysign(torch.ones_like(sd), a[:, 2])
        aa = -1.0 / (sg + a[:, 2])
        bb = a[:, 0] * a[:, 1] * aa
        b1 = torch.stack((1.0 + sg * a[:, 0] * a[:, 0] * aa, sg * bb, -sg * a[:, 0]), dim=1)
        b2 = torch.stack((bb, sg + a[:, 1] * a[:, 1] * aa, -a[:, 1]), dim=1)
        d = b1 * (sin_t * cs)[:, None] + b2 * (sin_t * s)[:, None] + a * cos_t[:, None]
        h = torch.clamp(R2[0, pick] - d2p * sin2, min=0.0)
        t = torch.where(ins, sd * cos_t + torch.sqrt(h), sd * cos_t - torch.sqrt(h))
        ray = torch.empty((pick.shape[0], 7), dtype=torch.float64, device=pick.device)
        ray[:, 0:3], ray[:, 3:6], ray[:, 6] = pts[lo:lo + chunk, 0:3], d * t[:, None], pts[lo:lo + chunk, 3]
        picks.append(pick)
        pdfs.append(P / (TWO_PI * mp))
        rays.append(ray)
    return torch.cat(picks), torch.cat(pdfs), torch.cat(rays), st2


def one_row(a, n_lights):
    """The child: one light count, both strategies; prints one JSON line."""
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    if not torch.cuda.is_available():
        sys.exit("light_sample_rate: no GPU -- a rate is measured on the device or not at all")
    rs = np.random.RandomState(n_lights)
    recs_np = scene_records(n_lights, rs)
    weights_np = rs.uniform(0.1, 3.0, size=n_lights)
    n = max(1 << 14, min(a.points, (1 << 30) // n_lights))              # the library leg: at most 2^30 pairs a launch
    nt = max(1 << 12, min(n, (1 << 26) // n_lights))                     # the torch leg: at most 2^26 pairs a run
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019 + n_lights)
    pts = torch.rand((n, 4), dtype=torch.float64, device="cuda", generator=gen)
    pts[:, 0:3] = pts[:, 0:3] * 20.0 - 10.0
    st0 = torch.randint(-(1 << 62), 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=gen) * 2 + 1
    ctx = tor.Context()
    ctx.upload(tor.Scene.from_records(recs_np).list())
    objects = np.arange(n_lights, dtype=np.int32)
    ctx.set_lights(objects, weights_np)
    recs, weights = torch.from_numpy(recs_np).cuda(), torch.from_numpy(weights_np).cuda()
    lamp = torch.from_numpy(objects).cuda()
    rows = []
    for strategy in STRATEGIES:
        solid = strategy == "solid_angle"
        st = st0.clone()
        out = ctx.sample_lights(pts, st, strategy=strategy)
        legs = {"library": lambda: ctx.sample_lights(pts, st, strategy=strategy, out=out),
                "torch": lambda: torch_sample(torch, recs, weights, pts[:nt], st0[:nt], solid)}
        size = {"library": n, "torch": nt}
        # the check, from the same states
        st = st0.clone()
        got = ctx.sample_lights(pts, st, strategy=strategy)
        pick, pdf, _rays, st2 = torch_sample(torch, recs, weights, pts[:nt], st0[:nt], solid)
        torch.cuda.synchronize()
        same_pick = lamp[pick] == got.light[:nt].long()
        rel = ((pdf - got.pdf[:nt]).abs() / got.pdf[:nt].abs())[same_pick]
        check = {"states_equal": bool(torch.equal(st2, st[:nt])), "picks_differ": int((~same_pick).sum()),
                 "pdf_differ_where_pick_agrees": int((rel > 1e-12).sum()), "n_checked": nt}
        for leg in legs:
            for _ in range(a.warm):
                legs[leg]()
        torch.cuda.synchronize()
        ms = {leg: [] for leg in legs}
        for _ in range(a.rounds):
            for leg in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    legs[leg]()
                e1.record()
                torch.cuda.synchronize()
                ms[leg].append(e0.elapsed_time(e1) / a.reps)
        rate = {leg: size[leg] / (statistics.median(ms[leg]) * 1e-3) / 1e6 for leg in legs}
        rows.append({"lights": n_lights, "strategy": strategy, "n": n, "n_torch": nt,
                     "mpoints_s": {k: round(v, 3) for k, v in rate.items()},
                     "gpairs_s": round(rate["library"] * n_lights / 1e3, 3), "library_vs_torch": round(rate["library"] / rate["torch"], 1),
                     "check": check, "device": torch.cuda.get_device_name(0)})
    ctx.close()
    print("ROW " + json.dumps(rows))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a light count may take")
    ap.add_argument("--row", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_sample_rate.txt"))
    a = ap.parse_args()
    if a.row:
        return one_row(a, a.row)
    rows = []
    for n_lights in LIGHTS:                                               # each GPU step under its own limit; stop at the first that fails
        cmd = [sys.executable, os.path.abspath(__file__), "--row", str(n_lights), "--points", str(a.points), "--reps", str(a.reps),
               "--rounds", str(a.rounds), "--warm", str(a.warm)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"light_sample_rate: {n_lights} lights ran past {a.step_timeout} s -- stopping", file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f"light_sample_rate: {n_lights} lights failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}",
                  file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        rows += json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])
    lines = [f"light_sample_rate: M points/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events; "
             f"{rows[0]['device']}",
             "expectation: by solid angle a (point, light) pair costs one `/`, one sqrt and about 15 float64 operations, twice (the total, "
             "then the walk); by weight one compare",
             f"{'lights':>7}  {'strategy':<12}{'points':>9}{'library':>12}{'G pairs/s':>11}{'torch':>12}{'(points)':>10}{'lib/torch':>11}"
             f"  states=  picks differ  pdf differ (pick agrees)"]
    for r in rows:
        g, c = r["mpoints_s"], r["check"]
        lines.append(f"{r['lights']:>7}  {r['strategy']:<12}{r['n']:>9}{g['library']:>12.2f}{r['gpairs_s']:>11.2f}{g['torch']:>12.3f}"
                     f"{r['n_torch']:>10}{r['library_vs_torch']:>11.1f}  {c['states_equal']!s:<7}  {c['picks_differ']:>6} of {c['n_checked']:<8}"
                     f"{c['pdf_differ_where_pick_agrees']:>6}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "light_sample_rate", "unit": "M points/s", "rows": rows}))
    return 0 if all(r["check"]["states_equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
