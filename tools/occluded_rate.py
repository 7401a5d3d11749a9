#!/usr/bin/env python3
"""Rates of the any-hit queries (tor_occluded_device) against the closest-hit queries (tor_hit_device) on the same device arrays
in one process: M rays/s per (scene, ray set, mode), with the `hit` leg run twice so the table shows the run-to-run spread.
    scenes     random_scene (485 objects) and frame 120 of the animation (1601 spheres, the two-level culling layout)
    ray sets   camera      the library's 108x192 camera rays (sample 0), tiled to at least 2^20 rays, range (0.001, +inf)
               incoherent  2^20 rays, seeded origins in the scene's box, uniform directions, range (0.001, +inf)
               segments    2^20 shadow segments p -> q, p in the scene's box, |q - p| uniform in (0.5, 3), range (0.001, 1.0)
    modes      brute, blocks
Every leg: WARM warm-up launches, then ROUNDS timings of REPS back-to-back launches between HIP events, the legs interleaved per
round (hit, occluded, hit again); the median over the rounds.  occluded must equal `hit().object >= 0` on every row.  Writes the
table to --out and prints one JSON line.

    python tools/occluded_rate.py [--reps 3] [--rounds 7] [--warm 2] [--out profiles/occluded_rate.txt]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")
MODES = ("brute", "blocks")
LEGS = ("hit_a", "occluded", "hit_b")


def scene_box(recs):
    r = torch.tensor(recs[:, 9:10], device="cuda").abs()
    c0, c1 = torch.tensor(recs[:, 1:4], device="cuda"), torch.tensor(recs[:, 4:7], device="cuda")
    return torch.quantile(torch.minimum(c0, c1) - r, 0.02, dim=0), torch.quantile(torch.maximum(c0, c1) + r, 0.98, dim=0)


def unit_vectors(n, gen):
    d = torch.randn((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    return d / d.norm(dim=1, keepdim=True)


def ray_sets(ctx, cam, recs, n, gen):
    """[(name, rays (m, 7), t_range (m, 2) or None)]"""
    cam_rays, _ = ctx.camera_rays(cam, 108, 192)
    tiled = cam_rays.repeat(((n + cam_rays.shape[0] - 1) // cam_rays.shape[0], 1)).contiguous()
    lo, hi = scene_box(recs)
    shutter = (float(cam.as_array()[22]), float(cam.as_array()[23]))
    times = lambda: shutter[0] + (shutter[1] - shutter[0]) * torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    inc = torch.empty((n, 7), dtype=torch.float64, device="cuda")
    inc[:, 0:3] = lo + (hi - lo) * torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    inc[:, 3:6] = unit_vectors(n, gen)
    inc[:, 6] = times()
    p = lo + (hi - lo) * torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    length = 0.5 + 2.5 * torch.rand((n, 1), dtype=torch.float64, device="cuda", generator=gen)
    seg, seg_range = tor.Context.shadow_segments(p, p + length * unit_vectors(n, gen), time=times())
    return [("camera", tiled, None), ("incoherent", inc, None), ("segments", seg, seg_range)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occluded_rate.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("occluded_rate: no GPU -- a rate is measured on the device or not at all")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261017)
    it = iter(tor.Animation(1080, 1920, 0.005, 0.0, 7.2).scenes(6))
    for _ in range(121):
        acam, ascene, _t = next(it)
    rows = []
    for sname, scene, cam in (("random_scene", tor.random_scene(0xFACADE), tor.camera()), ("anim120", ascene, acam)):
        ctx = tor.Context()
        ctx.upload(scene.list())
        for rname, rays, t_range in ray_sets(ctx, cam, scene.to_records(), a.rays, gen):
            n = int(rays.shape[0])
            tr = tuple(float(v) for v in torch.aminmax(rays[:, 6]))
            for m in MODES:
                legs = {"hit_a": lambda: ctx.hit(rays, t_range, tr, m), "hit_b": lambda: ctx.hit(rays, t_range, tr, m),
                        "occluded": lambda: ctx.occluded(rays, t_range, None, tr, m)}
                for leg in LEGS:
                    for _ in range(a.warm):
                        legs[leg]()
                h, o = legs["hit_a"](), legs["occluded"]()
                torch.cuda.synchronize()
                equal = bool(torch.equal(o.raw, (h.object >= 0).to(torch.int32)))
                share = float(o.occluded.double().mean())
                ms = {leg: [] for leg in LEGS}
                for _ in range(a.rounds):
                    for leg in LEGS:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.reps):
                            legs[leg]()
                        e1.record()
                        torch.cuda.synchronize()
                        ms[leg].append(e0.elapsed_time(e1) / a.reps)
                rate = {leg: n / (statistics.median(ms[leg]) * 1e-3) / 1e6 for leg in LEGS}
                rows.append({"scene": sname, "objects": len(scene), "rays": rname, "n": n, "mode": m, "ran": o.mode,
                             "occluded_share": round(share, 4), "mrays_s": {k: round(v, 1) for k, v in rate.items()},
                             "hit_spread": round(abs(rate["hit_a"] - rate["hit_b"]) / max(rate["hit_a"], rate["hit_b"]), 4),
                             "occluded_vs_hit": round(rate["occluded"] / max(rate["hit_a"], rate["hit_b"]), 3), "equal": equal})
        ctx.close()
    lines = [f"occluded_rate: M rays/s, median of {a.rounds} rounds of {a.reps} launches after {a.warm} warm-up launches, HIP events; "
             f"{torch.cuda.get_device_name(0)}",
             f"{'scene':<13}{'rays':<11}{'n':>9} {'mode':<7}{'occl.share':>10}{'hit':>10}{'occluded':>10}{'hit again':>10}"
             f"{'hit spread':>11}{'occl/hit':>9}  equal"]
    for r in rows:
        g = r["mrays_s"]
        lines.append(f"{r['scene']:<13}{r['rays']:<11}{r['n']:>9} {r['mode']:<7}{r['occluded_share']:>10.3f}{g['hit_a']:>10.1f}"
                     f"{g['occluded']:>10.1f}{g['hit_b']:>10.1f}{r['hit_spread']:>11.3f}{r['occluded_vs_hit']:>9.2f}  {r['equal']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "occluded_rate", "unit": "M rays/s", "reps": a.reps, "rounds": a.rounds, "warm": a.warm, "rows": rows}))
    return 0 if all(r["equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
