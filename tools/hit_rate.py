#!/usr/bin/env python3
"""Rates of the closest-hit queries (tor_hit_device): G rays/s of the brute force, the blocks and auto, and the mode auto chose, on
three workloads:
    camera      one pinhole ray per pixel of BASELINE configs[2]'s 1920x1080 view of random_scene
    incoherent  16 M rays, seeded origins in random_scene's box, uniform directions
    anim120     frame 120 of the animation (1601 spheres, the two-level culling layout): one pinhole ray per pixel at 1920x1080
Device events around REPS back-to-back launches after a warm-up, best of ROUNDS (modes interleaved per round).  The outputs are
hashed: every mode must give the same bytes.  Prints a table and one JSON line.

    python tools/hit_rate.py [--reps 5] [--rounds 3] [--out FILE.json]
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")
MODES = ("brute", "blocks", "auto")


def pinhole_rays(cam, h, w, gen):
    """Ray through the centre of projection and each pixel (cameras.nim:47-57 without the lens), times uniform in the shutter."""
    c = torch.tensor(cam.as_array(), dtype=torch.float64, device="cuda")
    origin, llc, horiz, vert = c[0:3], c[3:6], c[6:9], c[9:12]
    s = torch.arange(w, dtype=torch.float64, device="cuda") / (w - 1)
    t = torch.arange(h, dtype=torch.float64, device="cuda") / (h - 1)
    d = llc + s[None, :, None] * horiz + t[:, None, None] * vert - origin
    rays = torch.empty((h * w, 7), dtype=torch.float64, device="cuda")
    rays[:, 0:3] = origin
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 6] = c[22] + (c[23] - c[22]) * torch.rand(h * w, dtype=torch.float64, device="cuda", generator=gen)
    return rays


def incoherent_rays(recs, n, gen):
    r = torch.tensor(recs[:, 9:10], device="cuda").abs()
    c0, c1 = torch.tensor(recs[:, 1:4], device="cuda"), torch.tensor(recs[:, 4:7], device="cuda")
    lo = torch.quantile(torch.minimum(c0, c1) - r, 0.02, dim=0)
    hi = torch.quantile(torch.maximum(c0, c1) + r, 0.98, dim=0)
    rays = torch.empty((n, 7), dtype=torch.float64, device="cuda")
    rays[:, 0:3] = lo + (hi - lo) * torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    d = torch.randn((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    rays[:, 3:6] = d / d.norm(dim=1, keepdim=True)
    rays[:, 6] = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--incoherent", type=int, default=16 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261016)
    rscene, rcam = tor.random_scene(0xFACADE), tor.camera()
    it = iter(tor.Animation(1080, 1920, 0.005, 0.0, 7.2).scenes(6))
    for _ in range(121):
        acam, ascene, _t = next(it)
    work = [("camera", rscene, pinhole_rays(rcam, 1080, 1920, gen)),
            ("incoherent", rscene, incoherent_rays(rscene.to_records(), a.incoherent, gen)),
            ("anim120", ascene, pinhole_rays(acam, 1080, 1920, gen))]
    rows = []
    for name, scene, rays in work:
        ctx = tor.Context()
        ctx.upload(scene.list())
        n = rays.shape[0]
        times = rays[:, 6]
        tr = (float(times.min()), float(times.max()))
        best, chose, digest = {}, {}, {}
        for m in MODES:  # warm-up: layouts, bounds, code objects; the outputs' hashes
            res = ctx.hit(rays, None, tr, m)
            torch.cuda.synchronize()
            chose[m] = res.mode
            digest[m] = hashlib.sha256(res.raw.cpu().numpy().tobytes()).hexdigest()[:16]
            best[m] = 0.0
        for _ in range(a.rounds):
            for m in MODES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    ctx.hit(rays, None, tr, m)
                e1.record()
                torch.cuda.synchronize()
                best[m] = max(best[m], n * a.reps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
        fastest = max(best["brute"], best["blocks"])
        rows.append({"workload": name, "objects": len(scene), "rays": n, "grays_s": {m: round(best[m], 4) for m in MODES},
                     "auto_chose": chose["auto"], "auto_vs_fastest": round(best["auto"] / fastest, 4),
                     "hashes": digest, "hashes_equal": len(set(digest.values())) == 1})
        ctx.close()
    print(f"{'workload':<12}{'objects':>8}{'rays':>10}{'brute':>10}{'blocks':>10}{'auto':>10}  auto chose    auto/fastest  hashes equal")
    for r in rows:
        g = r["grays_s"]
        print(f"{r['workload']:<12}{r['objects']:>8}{r['rays']:>10}{g['brute']:>10.3f}{g['blocks']:>10.3f}{g['auto']:>10.3f}  "
              f"{r['auto_chose']:<13}{r['auto_vs_fastest']:>12.3f}  {r['hashes_equal']}")
    line = json.dumps({"tool": "hit_rate", "unit": "G rays/s", "reps": a.reps, "rounds": a.rounds, "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["hashes_equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
