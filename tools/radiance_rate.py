#!/usr/bin/env python3
"""Rates of the radiance queries (tor_radiance_device): M paths/s of the brute force, the blocks and auto, and the mode auto chose, on
three workloads at depth 50:
    camera      the camera paths of random_scene at 1920x1080, samples [0, 16) (tor_camera_rays_device, TOR_SEED_SAMPLE)
    incoherent  as many rays with seeded origins in random_scene's box, uniform directions and seed1 states
    anim120     frame 120 of the animation (1601 spheres, the two-level culling layout): its camera paths at 1920x1080, one sample
Device events around REPS back-to-back launches after a warm-up, best of ROUNDS (modes interleaved per round).  The outputs (colours
and states) are hashed: every mode must give the same bytes.  On the camera workload the rate of tor_render_accumulate_device over
the same sample range stands beside it -- the same paths plus camera generation: accel 0 against brute, accel 3 against
blocks / auto.  Prints a table and one JSON line.

    python tools/radiance_rate.py [--reps 3] [--rounds 3] [--samples 16] [--out FILE.json]
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")
MODES = ("brute", "blocks", "auto")
H, W, DEPTH = 1080, 1920, 50


def incoherent(recs, n, gen):
    r = torch.tensor(recs[:, 9:10], device="cuda").abs()
    c0, c1 = torch.tensor(recs[:, 1:4], device="cuda"), torch.tensor(recs[:, 4:7], device="cuda")
    lo = torch.quantile(torch.minimum(c0, c1) - r, 0.02, dim=0)
    hi = torch.quantile(torch.maximum(c0, c1) + r, 0.98, dim=0)
    rays = torch.empty((n, 7), dtype=torch.float64, device="cuda")
    rays[:, 0:3] = lo + (hi - lo) * torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    d = torch.randn((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    rays[:, 3:6] = d / d.norm(dim=1, keepdim=True)
    rays[:, 6] = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    st = torch.from_numpy(tor.rng_seed1(np.arange(n, dtype=np.uint64)).view(np.int64)).cuda()
    return rays, st


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261016)
    rscene, rcam = tor.random_scene(0xFACADE), tor.camera()
    it = iter(tor.Animation(H, W, 0.005, 0.0, 7.2).scenes(6))
    for _ in range(121):
        acam, ascene, _t = next(it)
    rows = []
    for name, scene, cam, ns in (("camera", rscene, rcam, a.samples), ("incoherent", rscene, None, a.samples),
                                 ("anim120", ascene, acam, 1)):
        ctx = tor.Context()
        ctx.upload(scene.list())
        if cam is not None:
            rays, st0 = ctx.camera_rays(cam, H, W, 0, ns, tor.SEED_SAMPLE)
        else:
            rays, st0 = incoherent(scene.to_records(), H * W * ns, gen)
        n = rays.shape[0]
        times = rays[:, 6]
        tr = (float(times.min()), float(times.max()))
        st = st0.clone()
        best, chose, digest = {}, {}, {}
        for m in MODES:  # warm-up: layouts, bounds, code objects; the outputs' hashes
            st.copy_(st0)
            color, st, chose[m] = ctx.radiance(rays, st, DEPTH, tr, m)
            torch.cuda.synchronize()
            digest[m] = hashlib.sha256(color.cpu().numpy().tobytes() + st.cpu().numpy().tobytes()).hexdigest()[:16]
            best[m] = 0.0
        for _ in range(a.rounds):
            for m in MODES:  # (the states advance from launch to launch: same work per launch, other draws)
                best[m] = max(best[m], n / timed(lambda: ctx.radiance(rays, st, DEPTH, tr, m), a.reps) / 1e6)
        row = {"workload": name, "objects": len(scene), "paths": n, "mpaths_s": {m: round(best[m], 1) for m in MODES},
               "auto_chose": chose["auto"], "hashes": digest, "hashes_equal": len(set(digest.values())) == 1}
        if name == "camera":  # the integrator over the same sample range: the same paths, plus camera generation
            sums = torch.zeros((H * W, 3), dtype=torch.float64, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            acc = {}
            for accel in (0, 3):
                opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel)
                ctx.accumulate_device(cam, H, W, 0, ns, DEPTH, opt, sums.data_ptr(), 0, s)
                torch.cuda.synchronize()
                acc[accel] = 0.0
                for _ in range(a.rounds):
                    acc[accel] = max(acc[accel], n / timed(lambda: ctx.accumulate_device(cam, H, W, 0, ns, DEPTH, opt, sums.data_ptr(), 0, s),
                                                           a.reps) / 1e6)
            row["accumulate_mpaths_s"] = {"accel0": round(acc[0], 1), "accel3": round(acc[3], 1)}
        rows.append(row)
        ctx.close()
    print(f"{'workload':<12}{'objects':>8}{'paths':>11}{'brute':>9}{'blocks':>9}{'auto':>9}  auto chose   hashes equal  accumulate (accel 0 / 3)")
    for r in rows:
        g = r["mpaths_s"]
        accs = r.get("accumulate_mpaths_s")
        print(f"{r['workload']:<12}{r['objects']:>8}{r['paths']:>11}{g['brute']:>9.1f}{g['blocks']:>9.1f}{g['auto']:>9.1f}  "
              f"{r['auto_chose']:<12}{str(r['hashes_equal']):<14}" + (f"{accs['accel0']:.1f} / {accs['accel3']:.1f}" if accs else "-"))
    line = json.dumps({"tool": "radiance_rate", "unit": "M paths/s", "depth": DEPTH, "reps": a.reps, "rounds": a.rounds, "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["hashes_equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
