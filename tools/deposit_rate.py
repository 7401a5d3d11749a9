#!/usr/bin/env python3
"""Rates of the exact sample deposit (tor_deposit_device) in one process: G samples/s per leg, 2^24 samples on a 1920x1080 film, k
samples per pixel for k in {1, 16, 64, 1000} (entry e belongs to pixel (e // k) mod npix: camera order, runs of k).  Legs,
interleaved per round between HIP events:
    camera      (a) the deposit in camera order, sums and moments
    camera S    (a) the same into the sums alone (what index_add_ computes)
    random      (b) the same samples after torch.randperm: every run has length 1 -- prices the in-wave reduction
    index_add   (c) torch.index_add_ on float64 sums: the yardstick, what a host falls back to without this entry
and, on the whole film at --pass-samples samples per pixel (random_scene, depth 50):
    radiance    (d) the tor_radiance_device launch that produced the colours, next to the deposit of those colours
    open pass   (e) camera_rays + radiance + deposit against tor_render_accumulate_device (with moments) for the same sample range
Every leg: WARM warm-up runs, then ROUNDS timings of REPS back-to-back runs; the median over the rounds.  The expectations under
test: (a) is not slower than (c) at any k, and (a) is a small share of (d); rows where one fails are marked, not hidden.  Camera and
random order must give the same bits, and the open pass the bits of the closed one.  Writes the table to --out and prints one JSON line.

    python tools/deposit_rate.py [--samples 16777216] [--pass-samples 8] [--reps 2] [--rounds 5] [--warm 1]
                                 [--out profiles/deposit_rate.txt]
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
NROWS, NCOLS = 1080, 1920
KS = (1, 16, 64, 1000)


def timed(legs, order, warm, rounds, reps):
    """{leg: median ms per run}: the legs interleaved per round, each between two HIP events."""
    for leg in order:
        for _ in range(warm):
            legs[leg]()
    torch.cuda.synchronize()
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
    return {leg: statistics.median(v) for leg, v in ms.items()}


def same_bits(a, b):
    return bool(torch.equal(a.reshape(-1).view(torch.int64), b.reshape(-1).view(torch.int64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 24)
    ap.add_argument("--pass-samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deposit_rate.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("deposit_rate: no GPU -- a rate is measured on the device or not at all")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261018)
    npix, n = NROWS * NCOLS, a.samples
    ctx = tor.Context()
    scene = tor.random_scene(0xFACADE)
    ctx.upload(scene.list())
    colors = torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    perm = torch.randperm(n, device="cuda", generator=gen)
    colors_r = colors[perm].contiguous()
    sums, moments = (torch.zeros((npix, 3), dtype=torch.float64, device="cuda") for _ in range(2))
    yard = torch.zeros((npix, 3), dtype=torch.float64, device="cuda")
    rows = []
    for k in KS:
        pixels = ((torch.arange(n, dtype=torch.int64, device="cuda") // k) % npix).int()
        pixels_r = pixels[perm].contiguous()
        pixels_l = pixels.long()
        # the two orders give the same bits (a film of its own each; the timed legs below only add to scratch films)
        fa, fb = (torch.zeros((2, npix, 3), dtype=torch.float64, device="cuda") for _ in range(2))
        ctx.deposit(colors, pixels, fa[0], fa[1])
        ctx.deposit(colors_r, pixels_r, fb[0], fb[1])
        torch.cuda.synchronize()
        equal = same_bits(fa, fb)
        del fa, fb
        legs = {"camera": lambda: ctx.deposit(colors, pixels, sums, moments),
                "camera S": lambda: ctx.deposit(colors, pixels, sums),
                "random": lambda: ctx.deposit(colors_r, pixels_r, sums, moments),
                "index_add": lambda: yard.index_add_(0, pixels_l, colors)}
        order = list(legs)
        ms = timed(legs, order, a.warm, a.rounds, a.reps)
        rate = {leg: n / (ms[leg] * 1e-3) / 1e9 for leg in order}
        rows.append({"k": k, "n": n, "ms": {leg: round(v, 4) for leg, v in ms.items()}, "gsamples_s": {leg: round(v, 3) for leg, v in rate.items()},
                     "camera_vs_index_add": round(rate["camera"] / rate["index_add"], 2),
                     "random_vs_camera": round(rate["random"] / rate["camera"], 2),
                     "holds": bool(rate["camera"] >= 0.97 * rate["index_add"]), "equal": equal})
        sums.zero_()
        moments.zero_()
        yard.zero_()
    del colors, colors_r, perm
    # (d), (e): one open pass over the whole film
    cam, kp = tor.camera(), a.pass_samples
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    rays, rng0 = ctx.camera_rays(cam, NROWS, NCOLS, 0, kp)
    rng = rng0.clone()
    pcol = ctx.radiance(rays, rng, 50, (0.0, 1.0))[0]
    ppix = torch.arange(npix, dtype=torch.int32, device="cuda").repeat_interleave(kp)
    closed = torch.zeros((2, npix, 3), dtype=torch.float64, device="cuda")
    ctx.accumulate_device(cam, NROWS, NCOLS, 0, kp, 50, opt, closed[0].data_ptr(), closed[1].data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    opened = torch.zeros_like(closed)
    ctx.deposit(pcol, ppix, opened[0], opened[1])
    torch.cuda.synchronize()
    pass_equal = same_bits(opened, closed)

    def open_pass():
        r, g = ctx.camera_rays(cam, NROWS, NCOLS, 0, kp)
        ctx.deposit(ctx.radiance(r, g, 50, (0.0, 1.0))[0], ppix, sums, moments)

    def radiance():
        rng.copy_(rng0)
        ctx.radiance(rays, rng, 50, (0.0, 1.0))
    legs = {"radiance": radiance, "copy": lambda: rng.copy_(rng0), "deposit": lambda: ctx.deposit(pcol, ppix, sums, moments),
            "open pass": open_pass,
            "closed pass": lambda: ctx.accumulate_device(cam, NROWS, NCOLS, 0, kp, 50, opt, sums.data_ptr(), moments.data_ptr(),
                                                         torch.cuda.current_stream().cuda_stream)}
    pm = timed(legs, list(legs), a.warm, a.rounds, a.reps)
    rad_ms = pm["radiance"] - pm["copy"]     # (the leg restores the generator states first: that copy is timed on its own)
    share = pm["deposit"] / rad_ms
    cost = pm["open pass"] / pm["closed pass"]
    pass_row = {"samples_per_pixel": kp, "n": npix * kp, "ms": {k_: round(v, 3) for k_, v in pm.items()}, "radiance_ms": round(rad_ms, 3),
                "deposit_share_of_radiance": round(share, 4), "open_vs_closed": round(cost, 2), "holds": bool(share < 0.1),
                "equal": pass_equal}
    lines = [f"deposit_rate: G samples/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events; "
             f"{torch.cuda.get_device_name(0)}; {n} samples per leg on a {NCOLS}x{NROWS} film, float64",
             f"{'k':>6}{'camera':>10}{'camera S':>10}{'random':>10}{'index_add':>11}{'camera/index_add':>18}{'random/camera':>15}"
             f"  expectation  orders equal"]
    for r in rows:
        g = r["gsamples_s"]
        lines.append(f"{r['k']:>6}{g['camera']:>10.3f}{g['camera S']:>10.3f}{g['random']:>10.3f}{g['index_add']:>11.3f}"
                     f"{r['camera_vs_index_add']:>18.2f}{r['random_vs_camera']:>15.2f}  {'holds' if r['holds'] else 'FAILS':<11}  {r['equal']}")
    lines.append(f"open pass, random_scene, depth 50, {kp} samples per pixel ({npix * kp} samples): radiance {rad_ms:.2f} ms, deposit "
                 f"{pm['deposit']:.3f} ms = {100 * share:.2f} % of it ({'holds' if pass_row['holds'] else 'FAILS'}: expected below 10 %); "
                 f"camera_rays + radiance + deposit {pm['open pass']:.2f} ms against tor_render_accumulate_device {pm['closed pass']:.2f} ms "
                 f"= {cost:.2f} x; same bits: {pass_equal}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "deposit_rate", "unit": "G samples/s", "reps": a.reps, "rounds": a.rounds, "warm": a.warm, "rows": rows,
                      "pass": pass_row}))
    return 0 if all(r["equal"] for r in rows) and pass_equal else 1


if __name__ == "__main__":
    sys.exit(main())
