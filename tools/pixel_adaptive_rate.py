#!/usr/bin/env python3
"""Adaptive sampling on the reference's pixel streams (tor_render_resume_list_device, PixelAdaptive) on random_scene at 1920x1080.

1. List overhead: one listed pass over the FULL list against one tor_render_resume_device pass (with moments) of the same samples
   (--spp, default 128), TOR_PIXEL_KERNEL_LANE, accel 0 and 3.  Four legs, each repetition of each in a fresh child process that warms
   up with one 16-sample pass of its own kind: (a) the resume pass in ANOTHER build (--parent-lib: the parent commit's), (b) the resume
   pass in this build, (c) the listed pass in this build, (d) the resume pass in this build with the cost probe and the tile order off
   (TOR_LPT_MIN_SPP=0) -- a listed pass runs neither, so (c) against (d) is the cost of the list indirection alone and (d) against (b)
   what the tile order is worth at this pass size.  Kernel time (tor_last_kernel_ms: the pass's kernel, the probe not included), median of
   REPS, legs interleaved; the differences stand next to the run-to-run spread (max - min over median) of (a).  All must leave the same
   state, sums and moments.
2. Kernel crossover: cost per listed sample over ascending random sub-lists of 100 / 25 / 5 / 4 / 1 / 0.1 % of the frame under LANE,
   WAVE and AUTO, for passes of 16 and of 128 (accel --cmp-accel): STARTING passes (first_sample = 0, the same samples in every
   repetition) and, for the two forced kernels, CONTINUED passes (first_sample > 0: state, sums and moments are loaded per pixel; every
   repetition runs the streams' next samples).  Kernel time, median of REPS.  The kernel AUTO ran is read from the library
   (tor_debug_last_variant after a sentinel launch); AUTO is flagged when it is slower than the faster forced kernel by more than the
   spread seen at that point.
3. End to end: PixelAdaptive.run() (rel_tol 0.05, max_samples 1024) for passes of 16 and of 128 against a uniform PixelProgressive to
   max_samples: samples spent, wall time, count histogram.

    python tools/pixel_adaptive_rate.py --parent-lib /path/to/parent/libtor_mi355x.so [--spp 128] [--reps 5] [--skip 1,2,3] [--out FILE.txt]
"""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:12]


def child(a):
    """one leg of section 1 in a process of its own: prints one JSON line {kernel ms, wall s, hash of (rng, sums, moments)}"""
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    H, W = a.height, a.width
    ctx = tor.Context()
    ctx.upload(tor.random_scene(0xFACADE).list())
    stream = torch.cuda.current_stream().cuda_stream
    opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=a.child_accel, pixel_kernel=tor.PIXEL_KERNEL_LANE)
    cam = tor.camera()
    rng = torch.zeros((H, W, 4), dtype=torch.int64, device="cuda")
    sums = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
    mom = torch.zeros_like(sums)
    full = torch.arange(H * W, dtype=torch.int32, device="cuda")

    def run(n):
        if a.child_leg == "listed":
            ctx.resume_list_device(cam, H, W, full.data_ptr(), H * W, 0, n, a.depth, opt, rng.data_ptr(), sums.data_ptr(), mom.data_ptr(), stream)
        else:
            ctx.resume_device(cam, H, W, 0, n, a.depth, opt, rng.data_ptr(), sums.data_ptr(), mom.data_ptr(), stream)

    run(16)  # warm-up: layouts, code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(a.spp)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    try:  # (tor_last_pixel_cost refuses when the last launch ran no cost probe)
        probe = ctx.last_pixel_cost(H * W).size > 0
    except tor.TorError:
        probe = False
    print(json.dumps({"kernel_ms": ctx.last_kernel_ms()[0], "probe": probe, "wall_s": wall, "variant": ctx.last_variant()[0], "hash": _digest(rng, sums, mom)}))
    ctx.close()


def run_child(a, accel, lib, leg):
    env = dict(os.environ)
    env.pop("TOR_AB_LIB", None)  # (this build unless the leg names another)
    env.pop("TOR_LPT_MIN_SPP", None)
    if lib:
        env["TOR_AB_LIB"] = lib
    if leg == "resume-unordered":
        env["TOR_LPT_MIN_SPP"] = "0"
    cmd = [sys.executable, os.path.abspath(__file__), "--child-accel", str(accel), "--child-leg", leg, "--spp", str(a.spp),
           "--width", str(a.width), "--height", str(a.height), "--depth", str(a.depth)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=128, help="samples of the passes of section 1")
    ap.add_argument("--accel", default="3,0")
    ap.add_argument("--cmp-accel", type=int, default=3)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fractions", default="1,0.25,0.05,0.04,0.01,0.001")
    ap.add_argument("--passes", default="16,128")
    ap.add_argument("--rel-tol", type=float, default=0.05)
    ap.add_argument("--run-passes", default="16,128", help="pass sizes of section 3")
    ap.add_argument("--max-samples", type=int, default=1024)
    ap.add_argument("--skip", default="", help="sections to leave out, e.g. 1,3")
    ap.add_argument("--parent-lib", default=None, help="libtor_mi355x.so built from the parent commit (leg a); without it leg (a) is this build")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-accel", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-leg", default="resume", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_accel is not None:
        return child(a)
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    H, W = a.height, a.width
    npix = H * W
    skip = {int(x) for x in a.skip.split(",") if x}
    lines, ok = [], True

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"pixel_adaptive_rate: {W}x{H}, depth {a.depth}, random_scene, {a.reps} repetitions; parent build: {a.parent_lib or '(this build)'}")

    # ---- 1. the list indirection ----
    if 1 not in skip:
        emit(f"\n1. list overhead: one pass of {a.spp} samples, TOR_PIXEL_KERNEL_LANE, kernel ms (median of {a.reps}, legs interleaved, a process per run)")
        legs = (("a resume, parent build", a.parent_lib, "resume"), ("b resume, this build", None, "resume"), ("c full list, this build", None, "listed"),
                ("d resume, no tile order", None, "resume-unordered"))
        for accel in [int(x) for x in a.accel.split(",")]:
            ms = {name: [] for name, _, _ in legs}
            digest, variant, probe = {}, {}, {}
            for _ in range(a.reps):
                for name, lib, leg in legs:
                    c = run_child(a, accel, lib, leg)
                    ms[name].append(c["kernel_ms"])
                    digest[name], variant[name], probe[name] = c["hash"], c["variant"], c["probe"]
            med = {k: statistics.median(v) for k, v in ms.items()}
            base = med[legs[0][0]]
            spread = (max(ms[legs[0][0]]) - min(ms[legs[0][0]])) / base
            emit(f"  accel {accel}: spread of (a) over {a.reps} runs = {spread * 100:.2f} %")
            emit(f"  {'leg':>26} {'variant':>7} {'probe':>5} {'median ms':>10} {'min ms':>9} {'max ms':>9} {'Msamples/s':>11} {'vs (a)':>8} {'vs (b)':>8}  hash")
            for name, _, _ in legs:
                v = ms[name]
                same = digest[name] == digest[legs[1][0]]
                ok = ok and same
                emit(f"  {name:>26} {variant[name]:>7} {'yes' if probe[name] else 'no':>5} {med[name]:>10.2f} {min(v):>9.2f} {max(v):>9.2f} {npix * a.spp / med[name] / 1e3:>11.1f} "
                     f"{(med[name] / base - 1) * 100:>+7.2f}% {(med[name] / med[legs[1][0]] - 1) * 100:>+7.2f}%  {digest[name]}" + ("" if same else "  DIFFERS"))
            d_name = legs[3][0]
            emit(f"  the list indirection alone, (c) against (d): {(med[legs[2][0]] / med[d_name] - 1) * 100:+.2f} %; the tile order at this pass size, (d) against (b): "
                 f"{(med[d_name] / med[legs[1][0]] - 1) * 100:+.2f} %")

    ctx = tor.Context()
    ctx.upload(tor.random_scene(0xFACADE).list())
    cam = tor.camera()
    stream = torch.cuda.current_stream().cuda_stream

    # ---- 2. the kernel crossover ----
    if 2 not in skip:
        names = {tor.PIXEL_KERNEL_LANE: "LANE", tor.PIXEL_KERNEL_WAVE: "WAVE", tor.PIXEL_KERNEL_AUTO: "AUTO"}
        forced = (tor.PIXEL_KERNEL_LANE, tor.PIXEL_KERNEL_WAVE)
        emit(f"\n2. kernel crossover: passes over ascending random sub-lists, accel {a.cmp_accel}; ns of kernel time per listed sample (median of "
             f"{a.reps}; start = first_sample 0, cont. = first_sample > 0; spread = (max - min) / median of the point's widest starting leg)")
        emit(f"  {'pass':>5} {'list':>9} {'share':>7} {'LANE start':>11} {'WAVE start':>11} {'AUTO start':>11} {'AUTO ran':>9} {'LANE cont.':>11} {'WAVE cont.':>11} "
             f"{'spread':>7}  verdict")
        rng = torch.zeros((H, W, 4), dtype=torch.int64, device="cuda")
        sums = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        mom = torch.zeros_like(sums)
        tiny = [torch.zeros((2, 2, c), dtype=t, device="cuda") for c, t in ((4, torch.int64), (3, torch.float64), (3, torch.float64))]
        lane_opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=a.cmp_accel, pixel_kernel=tor.PIXEL_KERNEL_LANE)
        gen = np.random.default_rng(20261017)

        def launch(pk, lst, n, first, k):
            opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=a.cmp_accel, pixel_kernel=pk)
            ctx.resume_list_device(cam, H, W, lst.data_ptr(), n, first, k, a.depth, opt, rng.data_ptr(), sums.data_ptr(), mom.data_ptr(), stream)
            torch.cuda.synchronize()
            return ctx.last_kernel_ms()[0]

        for k in [int(x) for x in a.passes.split(",")]:
            for frac in [float(x) for x in a.fractions.split(",")]:
                n = npix if frac >= 1.0 else max(1, int(round(npix * frac)))
                lst = torch.from_numpy(np.sort(gen.choice(npix, size=n, replace=False)).astype(np.int32)).cuda()
                # which kernel AUTO runs, from the library: a 2 x 2 whole-frame lane launch leaves variant 6; a listed lane launch then says 7,
                # a wave launch leaves the 6
                ctx.resume_device(cam, 2, 2, 0, 1, a.depth, lane_opt, tiny[0].data_ptr(), tiny[1].data_ptr(), tiny[2].data_ptr(), stream)
                launch(tor.PIXEL_KERNEL_AUTO, lst, n, 0, k)
                ran = "LANE" if ctx.last_variant()[0] == 7 else "WAVE"
                ms = {pk: [] for pk in names}
                for rep_i in range(a.reps + 1):  # (the first round warms up)
                    for pk in names:
                        t = launch(pk, lst, n, 0, k)
                        if rep_i:
                            ms[pk].append(t)
                cont = {pk: [] for pk in forced}
                for pk in forced:  # continued passes: the listed pixels hold k samples from the last starting pass and go on from there
                    launch(pk, lst, n, 0, k)
                    for rep_i in range(a.reps):
                        cont[pk].append(launch(pk, lst, n, k * (rep_i + 1), k))
                med = {pk: statistics.median(v) for pk, v in ms.items()}
                spread = max((max(v) - min(v)) / med[pk] for pk, v in ms.items())
                ns = {pk: med[pk] * 1e6 / (n * k) for pk in names}
                cns = {pk: statistics.median(cont[pk]) * 1e6 / (n * k) for pk in forced}
                best = min(ns[tor.PIXEL_KERNEL_LANE], ns[tor.PIXEL_KERNEL_WAVE])
                good = ns[tor.PIXEL_KERNEL_AUTO] <= best * (1 + spread)
                ok = ok and good
                emit(f"  {k:>5} {n:>9} {frac * 100:>6.1f}% {ns[tor.PIXEL_KERNEL_LANE]:>11.3f} {ns[tor.PIXEL_KERNEL_WAVE]:>11.3f} {ns[tor.PIXEL_KERNEL_AUTO]:>11.3f} "
                     f"{ran:>9} {cns[tor.PIXEL_KERNEL_LANE]:>11.3f} {cns[tor.PIXEL_KERNEL_WAVE]:>11.3f} {spread * 100:>6.2f}%  "
                     f"{'ok' if good else 'AUTO IS NOT THE FASTER KERNEL'}")

    # ---- 3. end to end ----
    if 3 not in skip:
        opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=a.cmp_accel)
        warm = tor.PixelAdaptive(ctx, cam, H, W, a.depth, opt, rel_tol=a.rel_tol, max_samples=32)
        warm.run()
        tor.PixelProgressive(ctx, cam, H, W, a.depth, opt).add(32)
        torch.cuda.synchronize()
        del warm
        t0 = time.perf_counter()
        pp = tor.PixelProgressive(ctx, cam, H, W, a.depth, opt)
        pp.add(a.max_samples)
        uimg = pp.image()
        torch.cuda.synchronize()
        t_u = time.perf_counter() - t0
        emit(f"\n3. end to end, accel {a.cmp_accel}, rel_tol {a.rel_tol}, max {a.max_samples}, TOR_PIXEL_KERNEL_AUTO")
        emit(f"  uniform PixelProgressive, one pass of {a.max_samples}: {npix * a.max_samples} samples, {t_u:.3f} s wall, {npix * a.max_samples / t_u / 1e6:.1f} Msamples/s")
        for ps in [int(x) for x in a.run_passes.split(",")]:
            t0 = time.perf_counter()
            ad = tor.PixelAdaptive(ctx, cam, H, W, a.depth, opt, rel_tol=a.rel_tol, min_samples=ps, pass_samples=ps, max_samples=a.max_samples)
            sizes = []
            while ad.active > 0 and ad.samples < ad.max_samples:
                sizes.append(ad.active)
                ad.step()
            img = ad.image()
            torch.cuda.synchronize()
            t_ad = time.perf_counter() - t0
            spent = ad.total_samples()
            hist = {int(k): int(v) for k, v in zip(*np.unique(ad.counts().cpu().numpy(), return_counts=True))}
            at_max = ad.counts() == a.max_samples
            same = bool(torch.equal(img[at_max], uimg[at_max]))
            ok = ok and same
            emit(f"  PixelAdaptive.run(), passes of {ps} (min_samples {ps}): {len(sizes)} passes, {spent} samples ({spent / npix:.1f} per pixel), {t_ad:.3f} s wall, "
                 f"{spent / t_ad / 1e6:.1f} Msamples/s")
            emit(f"    samples {spent / (npix * a.max_samples) * 100:.1f} % and time {t_ad / t_u * 100:.1f} % of the uniform frame's; the {int(at_max.sum())} pixels at "
                 f"{a.max_samples} {'equal' if same else 'DIFFER FROM'} the uniform frame's bit for bit")
            emit("    list lengths per pass: " + " ".join(str(x) for x in sizes[:8]) + (" ... " + " ".join(str(x) for x in sizes[-3:]) if len(sizes) > 8 else ""))
            emit("    counts: " + " ".join(f"{k}:{v}" for k, v in hist.items()))
            del ad
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
