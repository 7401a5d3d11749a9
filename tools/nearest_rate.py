#!/usr/bin/env python3
"""Rates of the nearest-surface point queries (tor_nearest_device) against what a host does without them -- the same definition as
a batched torch float64 computation over n_points x n_objects on the same device, min (K = 1) or topk (K > 1) per point, chunked to
fit memory -- in one process: G points/s per (workload, K, leg).  Workloads:
    random      random_scene (485 objects), uniform points in the scene's box, time in (0, 1), no limit
    random d1   the same points with d_max = 1.0
    anim120     frame 120 of the animation (1601 spheres, the two-level culling layout), uniform points in its box
Legs, interleaved per round between HIP events: brute, blocks, auto (one tor_nearest_device launch each, into outputs allocated
before the timing) and torch (the yardstick, on the first --torch-points points).  Every leg: WARM warm-up runs, then ROUNDS timings
of REPS back-to-back runs; the median over the rounds.  The expectation under test: auto is never slower than brute, and faster than
torch at every K; rows where it is not are marked.  The three library legs must agree bit for bit, and K = 1 with torch's minimum.
Writes the table to --out and prints one JSON line.

    python tools/nearest_rate.py [--points 4194304] [--torch-points 1048576] [--reps 2] [--rounds 5] [--warm 1]
                                 [--out profiles/nearest_rate.txt]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")
MODES = ("brute", "blocks", "auto")
KS = (1, 4, tor.NEAREST_MAX)
CHUNK = 1 << 16


def scene_box(recs):
    """The 2nd .. 98th percentile box of the spheres (the ground sphere's top is what matters)."""
    r = np.abs(recs[:, 9:10])
    lo = np.minimum(recs[:, 1:4], recs[:, 4:7]) - r
    hi = np.maximum(recs[:, 1:4], recs[:, 4:7]) + r
    return np.percentile(lo, 2, axis=0), np.percentile(hi, 98, axis=0)


def torch_nearest(recs, pts, k, d_max):
    """The definition in plain torch float64, chunk by chunk: (distance (n, k), object (n, k)), +inf / -1 where there is none."""
    kind, c0, c1, t0, t1, r = recs[None, :, 0], recs[None, :, 1:4], recs[None, :, 4:7], recs[None, :, 7], recs[None, :, 8], recs[None, :, 9]
    dist, obj = [], []
    for lo in range(0, int(pts.shape[0]), CHUNK):
        p, time = pts[lo:lo + CHUNK, None, 0:3], pts[lo:lo + CHUNK, None, 3]
        f = (time - t0) / (t1 - t0)
        c = torch.where((kind != 0)[:, :, None], c0 + (c1 - c0) * f[:, :, None], c0)
        oc = p - c
        x, y, z = oc[:, :, 0], oc[:, :, 1], oc[:, :, 2]
        d = torch.sqrt(x * x + y * y + z * z) - r.abs()
        ok = torch.isfinite(d) if d_max is None else torch.isfinite(d) & (d < d_max)
        d = torch.where(ok, d, torch.full_like(d, float("inf")))
        if k == 1:
            best, arg = d.min(dim=1, keepdim=True)
        else:
            best, arg = torch.topk(d, k, dim=1, largest=False, sorted=True)
        dist.append(best)
        obj.append(torch.where(torch.isfinite(best), arg, torch.full_like(arg, -1)))
    return torch.cat(dist), torch.cat(obj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--torch-points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_rate.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nearest_rate: no GPU -- a rate is measured on the device or not at all")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261018)
    it = iter(tor.Animation(1080, 1920, 0.005, 0.0, 7.2).scenes(6))
    for _ in range(121):
        _cam, ascene, _t = next(it)
    rows = []
    for wname, scene, d_max in (("random", tor.random_scene(0xFACADE), None), ("random d1", tor.random_scene(0xFACADE), 1.0),
                                ("anim120", ascene, None)):
        recs_np = scene.to_records()
        lo, hi = scene_box(recs_np)
        recs = torch.from_numpy(recs_np).cuda()
        n, nt = a.points, min(a.torch_points, a.points)
        pts = torch.rand((n, 4), dtype=torch.float64, device="cuda", generator=gen)
        pts[:, 0:3] = torch.from_numpy(lo).cuda() + pts[:, 0:3] * torch.from_numpy(hi - lo).cuda()
        ctx = tor.Context()
        ctx.upload(scene.list())
        for k in KS:
            outs = {m: ctx.nearest(pts, k, d_max, None, (0.0, 1.0), m) for m in MODES}   # written again by every timed call
            legs = {m: (lambda m=m: ctx.nearest(pts, k, d_max, None, (0.0, 1.0), m, out=outs[m])) for m in MODES}
            legs["torch"] = lambda: torch_nearest(recs, pts[:nt], k, d_max)
            size = {m: n for m in MODES}
            size["torch"] = nt
            order = list(MODES) + ["torch"]
            for leg in order:
                for _ in range(a.warm):
                    legs[leg]()
            torch.cuda.synchronize()
            ran = {m: outs[m].mode for m in MODES}
            equal = all(torch.equal(outs[m].raw.view(torch.int64), outs["brute"].raw.view(torch.int64))
                        and torch.equal(outs[m].count, outs["brute"].count) for m in MODES)
            td, _to = torch_nearest(recs, pts[:nt], k, d_max)
            has = torch.isfinite(td)
            got = outs["auto"].distance[:nt]
            equal_torch = bool(torch.equal(outs["auto"].count[:nt], has.sum(dim=1).int())
                               and torch.equal(got[has].view(torch.int64), td[has].view(torch.int64)))
            mean_count = float(outs["auto"].count.double().mean())
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
            rate = {leg: size[leg] / (statistics.median(ms[leg]) * 1e-3) / 1e9 for leg in order}
            rows.append({"workload": wname, "objects": len(scene), "n": n, "n_torch": nt, "k": k, "d_max": d_max, "ran": ran,
                         "mean_count": round(mean_count, 3), "gpoints_s": {leg: round(v, 4) for leg, v in rate.items()},
                         "auto_vs_brute": round(rate["auto"] / rate["brute"], 3), "auto_vs_torch": round(rate["auto"] / rate["torch"], 1),
                         "holds": bool(rate["auto"] >= 0.97 * rate["brute"] and rate["auto"] > rate["torch"]),
                         "equal": bool(equal), "equal_torch": equal_torch})
        ctx.close()
    lines = [f"nearest_rate: G points/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events; "
             f"{torch.cuda.get_device_name(0)}; {a.points} points per library leg, {min(a.torch_points, a.points)} per torch leg",
             f"{'workload':<11}{'objects':>8}{'K':>4}{'count':>8}{'brute':>10}{'blocks':>10}{'auto':>10}{'torch':>10}{'auto/brute':>12}"
             f"{'auto/torch':>12}  auto ran                expectation  equal  =torch"]
    for r in rows:
        g = r["gpoints_s"]
        lines.append(f"{r['workload']:<11}{r['objects']:>8}{r['k']:>4}{r['mean_count']:>8.2f}{g['brute']:>10.3f}{g['blocks']:>10.3f}"
                     f"{g['auto']:>10.3f}{g['torch']:>10.4f}{r['auto_vs_brute']:>12.2f}{r['auto_vs_torch']:>12.1f}  {r['ran']['auto']:<22}  "
                     f"{'holds' if r['holds'] else 'FAILS':<11}  {r['equal']!s:<5}  {r['equal_torch']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "nearest_rate", "unit": "G points/s", "reps": a.reps, "rounds": a.rounds, "warm": a.warm, "rows": rows}))
    return 0 if all(r["equal"] and r["equal_torch"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
