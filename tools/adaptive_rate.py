#!/usr/bin/env python3
"""Adaptive sampling (tor_render_accumulate_list_device + tor_adaptive_select_device) on random_scene.

1. Cost of the list indirection: at 1920x1080 x SPP (default 256), one full-frame list pass against one tor_render_accumulate_device
   pass with moments, for accel 0 and 3.  Kernel time (tor_last_kernel_ms) and wall time, best of REPS, interleaved; the resolved
   canvases must hash the same.
2. Adaptive against uniform at 1080p (accel --cmp-accel, default 3) for a few tolerances: samples spent, wall time, the final frame's
   mean / max standard error (each pixel at its own count) and the count histogram.  Uniform references: Progressive.render_until
   to the adaptive frame's max standard error (same pass size, same cap), and a uniform render with the same sample budget.

Prints tables and one JSON line.

    python tools/adaptive_rate.py [--spp 256] [--accel 0,3] [--tols rel:0.2,rel:0.1,rel:0.05,abs:0.004,abs:0.002] [--max-samples 1024]
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")


def frame_se(sums, moments, counts):
    """(mean, max) over the pixels of the largest per-channel standard error, each pixel at its own sample count."""
    n = counts.to(torch.float64).unsqueeze(-1)
    var = torch.clamp((moments - sums * sums / n) / (n - 1.0), min=0.0)
    se = torch.sqrt(var / n).amax(dim=-1)
    return float(se.mean()), float(se.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--accel", default="0,3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--cmp-accel", type=int, default=3)
    ap.add_argument("--tols", default="rel:0.2,rel:0.1,rel:0.05,abs:0.004,abs:0.002")
    ap.add_argument("--pass-samples", type=int, default=16)
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--max-samples", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W, N = a.height, a.width, a.spp
    npix = H * W
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context()
    ctx.upload(scene.list())
    stream = torch.cuda.current_stream().cuda_stream
    sums = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
    mom = torch.empty_like(sums)
    img = torch.empty_like(sums)
    full = torch.arange(npix, dtype=torch.int32, device="cuda")

    # ---- 1. the list indirection ----
    cost = []
    ok = True
    for accel in [int(x) for x in a.accel.split(",")]:
        opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel)

        def plain():
            ctx.accumulate_device(cam, H, W, 0, N, a.depth, opt, sums.data_ptr(), mom.data_ptr(), stream)

        def listed():
            ctx.accumulate_list_device(cam, H, W, full.data_ptr(), npix, 0, N, a.depth, opt, sums.data_ptr(), mom.data_ptr(), stream)

        runs = {"moments": plain, "full list": listed}
        best_wall = {k: 1e30 for k in runs}
        best_kern = {k: 1e30 for k in runs}
        digest = {}
        for fn in runs.values():  # warm-up: layouts, code objects
            sums.zero_(); mom.zero_(); fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, fn in runs.items():
                sums.zero_(); mom.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                best_wall[name] = min(best_wall[name], time.perf_counter() - t0)
                best_kern[name] = min(best_kern[name], ctx.last_kernel_ms()[0] / 1e3)
                ctx.resolve_device(sums.data_ptr(), sums.numel(), N, 2.2, img.data_ptr(), stream)
                torch.cuda.synchronize()
                digest[name] = hashlib.sha256(img.cpu().numpy().tobytes()).hexdigest()[:12] + \
                    hashlib.sha256(mom.cpu().numpy().tobytes()).hexdigest()[:4]
        same = digest["moments"] == digest["full list"]
        ok = ok and same
        for name in runs:
            cost.append({"accel": accel, "launch": name, "kernel_ms": round(best_kern[name] * 1e3, 2), "wall_ms": round(best_wall[name] * 1e3, 2),
                         "msamples_s": round(npix * N / best_wall[name] / 1e6, 1),
                         "overhead_pct": round((best_wall[name] / best_wall["moments"] - 1) * 100, 2),
                         "kernel_overhead_pct": round((best_kern[name] / best_kern["moments"] - 1) * 100, 2),
                         "hash": digest[name], "same": same})

    # ---- 2. adaptive against uniform ----
    opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=a.cmp_accel)
    cmp_rows = []
    for spec in a.tols.split(","):
        kind, val = spec.split(":")
        tol = dict(abs_tol=float(val), rel_tol=0.0) if kind == "abs" else dict(abs_tol=0.0, rel_tol=float(val))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ad = tor.Adaptive(ctx, cam, H, W, a.depth, opt, min_samples=a.min_samples, pass_samples=a.pass_samples, max_samples=a.max_samples, **tol)
        ad.run()
        torch.cuda.synchronize()
        t_ad = time.perf_counter() - t0
        counts = ad.counts()
        ad_mean, ad_max = frame_se(ad.sums, ad.moments, counts)
        spent = ad.total_samples()
        hist = {int(k): int(v) for k, v in zip(*np.unique(counts.cpu().numpy(), return_counts=True))}
        # uniform to the same frame max standard error
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pg = tor.Progressive(ctx, cam, H, W, a.depth, opt, moments=True)
        n_u = pg.render_until(max_se=ad_max, max_samples=a.max_samples, pass_samples=a.pass_samples)
        torch.cuda.synchronize()
        t_u = time.perf_counter() - t0
        u_mean, u_max = pg.noise()
        del pg
        # uniform with the adaptive sample budget (rounded down to a pass)
        n_b = max(a.pass_samples, spent // npix // a.pass_samples * a.pass_samples)
        pb = tor.Progressive(ctx, cam, H, W, a.depth, opt, moments=True)
        pb.add(n_b)
        b_mean, b_max = pb.noise()
        del pb
        del ad
        cmp_rows.append({"tol": spec, "adaptive": {"samples": spent, "spp_avg": round(spent / npix, 2), "wall_s": round(t_ad, 3),
                                                   "se_mean": ad_mean, "se_max": ad_max, "hist": hist},
                         "uniform_same_max_se": {"spp": n_u, "samples": n_u * npix, "wall_s": round(t_u, 3), "se_mean": u_mean, "se_max": u_max,
                                                 "reached": u_max <= ad_max},
                         "uniform_same_budget": {"spp": n_b, "samples": n_b * npix, "se_mean": b_mean, "se_max": b_max},
                         "sample_ratio": round(spent / (n_u * npix), 4)})
    ctx.close()

    print(f"list indirection, {W}x{H} x {N} spp (one pass, best of {a.reps}):")
    print(f"{'accel':>5} {'launch':>10} {'kernel ms':>10} {'wall ms':>9} {'Msamples/s':>11} {'wall vs mom':>12} {'kernel vs mom':>14}  hash")
    for r in cost:
        print(f"{r['accel']:>5} {r['launch']:>10} {r['kernel_ms']:>10.2f} {r['wall_ms']:>9.2f} {r['msamples_s']:>11.1f} {r['overhead_pct']:>+11.2f}% "
              f"{r['kernel_overhead_pct']:>+13.2f}%  {r['hash']}" + ("" if r["same"] else "  DIFFERS"))
    print(f"\nadaptive vs uniform, {W}x{H}, accel {a.cmp_accel}, passes of {a.pass_samples}, min {a.min_samples}, max {a.max_samples}:")
    print(f"{'tol':>10} {'ad spp':>7} {'ad s':>6} {'ad se mean':>11} {'ad se max':>10} | {'uni spp':>7} {'uni s':>6} {'uni se max':>10} "
          f"{'ratio':>6} | {'budget spp':>10} {'b se mean':>10} {'b se max':>10}")
    for r in cmp_rows:
        ad, u, b = r["adaptive"], r["uniform_same_max_se"], r["uniform_same_budget"]
        print(f"{r['tol']:>10} {ad['spp_avg']:>7.1f} {ad['wall_s']:>6.2f} {ad['se_mean']:>11.3e} {ad['se_max']:>10.3e} | {u['spp']:>7} "
              f"{u['wall_s']:>6.2f} {u['se_max']:>10.3e} {r['sample_ratio']:>6.3f} | {b['spp']:>10} {b['se_mean']:>10.3e} {b['se_max']:>10.3e}")
        print(f"{'':>10} counts: " + " ".join(f"{k}:{v}" for k, v in ad["hist"].items()))
    line = {"tool": "adaptive_rate", "size": f"{W}x{H}", "spp": N, "depth": a.depth, "reps": a.reps, "list_cost": cost,
            "cmp_accel": a.cmp_accel, "pass_samples": a.pass_samples, "min_samples": a.min_samples, "max_samples": a.max_samples,
            "adaptive_vs_uniform": cmp_rows}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
