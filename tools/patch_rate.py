#!/usr/bin/env python3
"""Rates of the planar patch queries (tor_patch_hit_device, tor_patch_occluded_device; include/tor_patches.h) on the device: M rays/s
at --rays rays for tables of 12, 64, 1024 and 16384 patches, closest hit and any-hit, and beside them, from the same run,
tor_hit_device in TOR_HIT_BRUTE on a scene of as many spheres -- a yardstick per ray x primitive (46 float64 operations per ray and
patch against 17 per ray and sphere, both walks wave-uniform with scalar record loads), not a bar.

The patches are random quads and triangles (half each) with edges of about one unit, corners uniform in a cube of side 20; the
spheres have radius 0.5 and centres uniform in the same cube; the rays start uniformly in the cube with uniform directions, so a
ray meets more primitives as the table grows and the any-hit query stops earlier.  Each table size runs in a child process under
--step-timeout (the first that fails or runs past it ends the run).  Every leg: --warm warm-up windows, then --rounds timed windows
between HIP events, each of `reps` back-to-back launches (chosen per size so that a window is some tens of milliseconds), legs
interleaved per round; the median over the rounds and the spread (max - min) / median.  Outputs are allocated before the timing.
Writes the table to --out and prints one JSON line.

    python tools/patch_rate.py [--rays 1048576] [--sizes 12,64,1024,16384] [--rounds 5] [--warm 1] [--out profiles/patch_rate.txt]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")
PAIR_FLOPS = {"patch": 46, "sphere": 17}


def timed(legs, order, warm, rounds, reps):
    """{leg: (median ms, spread)}: warm-up runs of every leg, then rounds of interleaved timings between HIP events."""
    for leg in order:
        for _ in range(warm * reps):
            legs[leg]()
    ms = {leg: [] for leg in order}
    for _ in range(rounds):
        for leg in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                legs[leg]()
            e1.record()
            torch.cuda.synchronize()
            ms[leg].append(e0.elapsed_time(e1) / reps)
    return {leg: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for leg, v in ms.items()}


def leg(a):
    n_p, n = a.leg, a.rays
    g = np.random.default_rng(1234 + n_p)
    patches = []
    for j in range(n_p):
        q, u, v = g.uniform(-10, 10, 3), g.normal(0, 1, 3), g.normal(0, 1, 3)
        patches.append(tor.Patch.quad(q, u, v, 0) if j % 2 == 0 else tor.Patch.triangle(q, q + u, q + v, 0))
    recs = np.zeros((n_p, 16))
    recs[:, 1:4] = recs[:, 4:7] = g.uniform(-10, 10, (n_p, 3))
    recs[:, 8], recs[:, 9], recs[:, 11:14] = 1.0, 0.5, 0.5
    ctx = tor.Context()
    ctx.upload(tor.Scene.from_records(recs).list())
    ctx.set_patches(patches)
    d = g.normal(size=(n, 3))
    rays = torch.from_numpy(np.concatenate([g.uniform(-10, 10, (n, 3)), d / np.linalg.norm(d, axis=1, keepdims=True), np.zeros((n, 1))], axis=1)).cuda()
    ph, oc = ctx.hit_patches(rays), ctx.occluded_patches(rays)
    sp = ctx.hit(rays, None, (0.0, 0.0), "brute")
    L, h, stream = tor.lib(), ctx._h, torch.cuda.current_stream().cuda_stream
    raw = sp.raw
    legs = {"patch_hit": lambda: ctx.hit_patches(rays, out=ph), "patch_any": lambda: ctx.occluded_patches(rays, out=oc),
            "sphere_brute": lambda: L.tor_hit_device(h, n, rays.data_ptr(), None, 0.0, 0.0, tor.HIT_BRUTE, raw.data_ptr(), stream)}
    reps = max(1, min(50, 8192 // n_p))
    t = timed(legs, ["patch_hit", "patch_any", "sphere_brute"], a.warm, a.rounds, reps)
    torch.cuda.synchronize()
    row = {"device": torch.cuda.get_device_name(0), "n_patches": n_p, "rays": n, "reps": reps,
           "patch_hit_share": round(float((ph.patch >= 0).double().mean()), 4), "sphere_hit_share": round(float((sp.object >= 0).double().mean()), 4),
           "ms": {k: round(v[0], 4) for k, v in t.items()}, "spread": {k: round(v[1], 3) for k, v in t.items()}}
    print("ROW " + json.dumps(row))
    return 0


def child(args, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"patch_rate: {what} ran past {limit} s -- stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"patch_rate: {what} failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--sizes", default="12,64,1024,16384")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one child process may take")
    ap.add_argument("--leg", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_rate.txt"))
    a = ap.parse_args()
    if a.leg:
        if not torch.cuda.is_available():
            sys.exit("patch_rate: no GPU -- a rate is measured on the device or not at all")
        return leg(a)
    rows = []
    for n_p in (int(s) for s in a.sizes.split(",")):
        rc, row = child(["--leg", str(n_p), "--rays", str(a.rays), "--rounds", str(a.rounds), "--warm", str(a.warm)], a.step_timeout,
                        f"the table of {n_p}")
        if rc:
            return rc
        rows.append(row)
    lines = [f"patch_rate: {a.rays} rays; median of {a.rounds} timed windows after {a.warm} warm-up window(s), HIP events, legs interleaved; "
             f"{rows[0]['device']}",
             "M rays/s, and G (ray x primitive) pairs/s = rays * primitives / time -- for the any-hit query an upper bound on the pairs walked "
             "(a lane stops at its first accepted patch)", "",
             f"{'prims':>6}{'reps':>6}{'patch hit':>11}{'patch any':>11}{'sphere brute':>14}{'Gpair/s hit':>13}{'Gpair/s sph':>13}{'hit/sph time':>14}"
             f"{'by flops':>10}{'spread h':>10}{'spread s':>10}{'hits p':>8}{'hits s':>8}"]
    for r in rows:
        m, s, n, k = r["ms"], r["spread"], r["rays"], r["n_patches"]
        rate = {key: n / (v * 1e-3) / 1e6 for key, v in m.items()}
        lines.append(f"{k:>6}{r['reps']:>6}{rate['patch_hit']:>11.1f}{rate['patch_any']:>11.1f}{rate['sphere_brute']:>14.1f}"
                     f"{rate['patch_hit'] * k / 1e3:>13.1f}{rate['sphere_brute'] * k / 1e3:>13.1f}{m['patch_hit'] / m['sphere_brute']:>14.2f}"
                     f"{PAIR_FLOPS['patch'] / PAIR_FLOPS['sphere']:>10.2f}{s['patch_hit']:>10.3f}{s['sphere_brute']:>10.3f}"
                     f"{r['patch_hit_share']:>8.3f}{r['sphere_hit_share']:>8.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "patch_rate", "rows": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
