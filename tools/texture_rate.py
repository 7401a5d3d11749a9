#!/usr/bin/env python3
"""Rates of the surface-texture query (tor_texture_eval_device, include/tor_texture.h) and what it costs a host integrator, on the
device, in child processes that each run under --step-timeout (the first that fails or runs past it ends the run):
    eval       M records/s of Context.albedo on the 2^20 hit records of one bounce of random_scene's camera rays (1024 x 1024), every
               object bound to ONE texture of the kind: unbound (the attenuation), constant, checker world / normal, a 256 x 256
               image nearest / bilinear; beside Context.bsdf (tor_bsdf_eval_device) on the same records, the query family's
               nearest relative (one record per lane, the cold record gathered by object).  Outputs allocated before the timing.
    trace      ms of trace(textures=True) against trace() on random_scene, --trace-rays camera rays, depth 50, every object bound to
               a CONSTANT equal to its albedo (the same paths, bit for bit -- checked), legs interleaved per round.
    parent     with --parent-lib: ms of trace() on this build against the library of the parent commit, each in a process of its own
               (TOR_AB_LIB), alternating parent / this for --parent-rounds rounds in this one run.  No figure is fixed in advance;
               the expectation is that they differ by no more than the 1-2.5 % by which these kernels answer to unrelated edits.
Every leg: --warm warm-up windows, then --rounds timed windows between HIP events, each of --eval-reps back-to-back launches (eval:
1000 launches of 27 to 40 us, so a window is tens of milliseconds and the launches queue behind each other) or --trace-reps
back-to-back trace() calls (20 calls of about 8 ms); the median over the rounds and the spread (max - min) / median.  Writes the
table to --out and prints one JSON line.

    python tools/texture_rate.py [--parent-lib /path/to/parent/libtor_mi355x.so] [--eval-reps 1000] [--trace-reps 20] [--rounds 7]
                                 [--warm 2] [--out profiles/texture_rate.txt]
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
KINDS = ("unbound", "constant", "checker world", "checker normal", "image nearest", "image bilinear")


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


def scene_and_rays(side):
    scene = tor.random_scene()
    ctx = tor.Context()
    ctx.upload(scene.list())
    rays, rng = ctx.camera_rays(tor.camera(), side, side, 0, 1, tor.SEED_SAMPLE)
    return scene, ctx, rays, rng


def texture_of(kind, side=256):
    g = np.random.default_rng(7)
    if kind == "constant":
        return tor.Texture.constant((0.5, 0.4, 0.3))
    if kind.startswith("checker"):
        return tor.Texture.checker((0.9, 0.9, 0.9), (0.1, 0.2, 0.1), 3.0, kind.split()[1])
    return tor.Texture.image(g.random((side, side, 3)), kind.split()[1])


def leg_eval(a):
    scene, ctx, rays, rng = scene_and_rays(1024)
    n_obj = len(scene)
    win = rays.clone()
    res = ctx.bounce(rays, rng)
    n = int(res.raw.shape[0])
    rows = []
    ev_b = ctx.bsdf(win, res, res.rays)
    for kind in KINDS:
        if kind == "unbound":
            ctx.set_textures([tor.Texture.constant((1, 1, 1))], np.full(n_obj, -1))
        else:
            ctx.set_textures([texture_of(kind)], np.zeros(n_obj, dtype=np.int32))
        ev = ctx.albedo(res)
        legs = {"albedo": lambda: ctx.albedo(res, out=ev), "albedo_again": lambda: ctx.albedo(res, out=ev),
                "bsdf": lambda: ctx.bsdf(win, res, res.rays, out=ev_b)}
        t = timed(legs, ["albedo", "bsdf", "albedo_again"], a.warm, a.rounds, a.eval_reps)
        rate = {k: n / (v[0] * 1e-3) / 1e6 for k, v in t.items()}
        rows.append({"kind": kind, "n": n, "hit_share": round(float((res.object >= 0).double().mean()), 4),
                     "mrec_s": {k: round(v, 1) for k, v in rate.items()}, "spread": {k: round(v[1], 3) for k, v in t.items()},
                     "albedo_vs_bsdf": round(min(rate["albedo"], rate["albedo_again"]) / rate["bsdf"], 3)})
    print("ROW " + json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}))
    return 0


def leg_trace(a, textured):
    side = int(round(a.trace_rays ** 0.5))
    scene, ctx, rays, rng = scene_and_rays(side)
    legs = {"trace": lambda: ctx.trace(rays, rng.clone(), 50)}
    order = ["trace"]
    same = None
    if textured:
        recs = scene.to_records()
        albedo = np.where((recs[:, 10] == 2)[:, None], 1.0, recs[:, 11:14])
        ctx.set_textures([tor.Texture.constant(c) for c in albedo], np.arange(len(recs)))
        legs["trace_textures"] = lambda: ctx.trace(rays, rng.clone(), 50, textures=True)
        order.append("trace_textures")
        c0, s0, _ = legs["trace"]()
        c1, s1, _ = legs["trace_textures"]()
        torch.cuda.synchronize()
        same = bool(torch.equal(c0.view(torch.int64), c1.view(torch.int64)) and torch.equal(s0, s1))
    t = timed(legs, order, a.warm, a.rounds, a.trace_reps)
    print("ROW " + json.dumps({"device": torch.cuda.get_device_name(0), "n": int(rays.shape[0]), "same_bits": same,
                               "ms": {k: round(v[0], 3) for k, v in t.items()}, "spread": {k: round(v[1], 3) for k, v in t.items()}}))
    return 0


def child(args, limit, what, env=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env)
    except subprocess.TimeoutExpired:
        print(f"texture_rate: {what} ran past {limit} s -- stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"texture_rate: {what} failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-rays", type=int, default=1 << 18)
    ap.add_argument("--eval-reps", type=int, default=1000, help="back-to-back query launches per timed window")
    ap.add_argument("--trace-reps", type=int, default=20, help="back-to-back trace() calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libtor_mi355x.so built from the parent commit: adds the parent legs")
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_rate.txt"))
    a = ap.parse_args()
    if a.leg:
        if not torch.cuda.is_available():
            sys.exit("texture_rate: no GPU -- a rate is measured on the device or not at all")
        return leg_eval(a) if a.leg == "eval" else leg_trace(a, a.leg == "trace_textures")
    common = ["--trace-rays", str(a.trace_rays), "--eval-reps", str(a.eval_reps), "--trace-reps", str(a.trace_reps), "--rounds", str(a.rounds), "--warm", str(a.warm)]
    rc, ev = child(["--leg", "eval"] + common, a.step_timeout, "the eval leg")
    if rc:
        return rc
    rc, tr = child(["--leg", "trace_textures"] + common, a.step_timeout, "the trace leg")
    if rc:
        return rc
    pairs = []
    if a.parent_lib:
        for k in range(a.parent_rounds):   # alternating processes: the parent's library, then this build's
            rc, p = child(["--leg", "trace"] + common, a.step_timeout, f"parent round {k}", dict(os.environ, TOR_AB_LIB=os.path.abspath(a.parent_lib)))
            if rc:
                return rc
            rc, t = child(["--leg", "trace"] + common, a.step_timeout, f"this build, round {k}")
            if rc:
                return rc
            pairs.append((p["ms"]["trace"], t["ms"]["trace"], p["spread"]["trace"], t["spread"]["trace"]))
    lines = [f"texture_rate: median of {a.rounds} timed windows of {a.eval_reps} launches (eval) / {a.trace_reps} calls (trace) after {a.warm} warm-up windows, HIP events, legs interleaved; "
             f"{ev['device']}",
             "", f"eval: M records/s on {ev['rows'][0]['n']} hit records of random_scene (hit share {ev['rows'][0]['hit_share']})",
             f"{'kind':<16}{'albedo':>9}{'again':>9}{'bsdf':>9}{'albedo/bsdf':>13}{'spread a':>10}{'spread b':>10}"]
    for r in ev["rows"]:
        g, s = r["mrec_s"], r["spread"]
        lines.append(f"{r['kind']:<16}{g['albedo']:>9.1f}{g['albedo_again']:>9.1f}{g['bsdf']:>9.1f}{r['albedo_vs_bsdf']:>13.3f}"
                     f"{s['albedo']:>10.3f}{s['bsdf']:>10.3f}")
    m, s = tr["ms"], tr["spread"]
    lines += ["", f"trace: ms for {tr['n']} camera rays of random_scene, depth 50, every object bound to a CONSTANT equal to its albedo "
                  f"(same bits as trace(): {tr['same_bits']})",
              f"trace() {m['trace']:.3f} (spread {s['trace']:.3f})   trace(textures=True) {m['trace_textures']:.3f} (spread {s['trace_textures']:.3f})   "
              f"ratio {m['trace_textures'] / m['trace']:.3f}"]
    if pairs:
        lines += ["", f"parent: ms of trace() on {tr['n']} rays, the parent commit's library against this build, a process each, alternating"]
        for k, (p, t, sp, st) in enumerate(pairs):
            lines.append(f"round {k}: parent {p:.3f} (spread {sp:.3f})   this {t:.3f} (spread {st:.3f})   this / parent {t / p:.4f}")
        mp, mt = statistics.median(x[0] for x in pairs), statistics.median(x[1] for x in pairs)
        lines.append(f"median: parent {mp:.3f}   this {mt:.3f}   this / parent {mt / mp:.4f}")
    else:
        lines += ["", "parent: not run (no --parent-lib)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "texture_rate", "eval": ev, "trace": tr, "parent": pairs}))
    return 0 if tr["same_bits"] else 1


if __name__ == "__main__":
    sys.exit(main())
