#!/usr/bin/env python3
"""Cost of resume passes on the reference's pixel streams (tor_render_resume_device) against one launch: random_scene at 1920x1080,
TOTAL samples per pixel (default 1000), accel 3 and accel 0, TOR_PIXEL_KERNEL_AUTO.  Legs:
  (a) tor_render_device(SEED_PIXEL) of ANOTHER build of the library (--parent-lib: the parent commit's)
  (b) the same call on this build
  (c) one resume pass of TOTAL          (d) 10 passes of TOTAL / 10          (e) passes of 16 (the last one shorter)
The gated legs (a), (b), (c) run like for like: each repetition of each in a fresh child process that warms up with one 64-spp launch
of its own kind and times one run; (d) and (e), recorded only, run in this process on one long-lived context.  Wall time from the
first enqueue to the finished canvas (resolve included for c-e), REPS repetitions (default 5) with the legs interleaved per
repetition; reports every leg's median time and Msamples/s, its time against (a)'s, and the run-to-run spread (max - min over
median) of (a).
Conditions (exit status 1 when one fails): (b) within (a)'s spread; (c) below (a) by no more than that spread plus the share of the
state traffic -- bytes in and out per pixel and pass over the device's HBM bandwidth, against the leg's kernel time.  (d) and (e) are
recorded.  Every leg must show leg (b)'s canvas hash.

    python tools/resume_rate.py --parent-lib /path/to/parent/libtor_mi355x.so [--total 1000] [--accel 3,0] [--reps 5] [--out FILE.txt]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_BYTES_PER_S = 8.0e12  # MI355X peak; the state traffic's share is an upper bound of what it can cost at that rate


def one_shot_child(a):
    """a gated leg -- one launch, or one resume pass -- in a process of its own: prints one JSON line {seconds and kernel ms per repetition, hash}"""
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context()
    ctx.upload(scene.list())
    stream = torch.cuda.current_stream().cuda_stream
    img = torch.empty((a.height, a.width, 3), dtype=torch.float64, device="cuda")
    opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=a.child_accel)
    pp = tor.PixelProgressive(ctx, cam, a.height, a.width, a.depth, opt) if a.child_leg == "resume" else None

    def run(n):
        if pp is None:
            ctx.render_device(cam, a.height, a.width, n, 2.2, a.depth, opt, img.data_ptr(), stream)
        else:
            pp.samples = 0
            pp.add(n)
            ctx.resolve_device(pp.sums.data_ptr(), pp.sums.numel(), n, 2.2, img.data_ptr(), stream)

    run(64)  # warm-up: layouts, code objects
    torch.cuda.synchronize()
    secs, kernel_ms = [], []
    for _ in range(a.child_reps):
        t0 = time.perf_counter()
        run(a.total)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        kernel_ms.append(ctx.last_kernel_ms()[0] if pp is not None else 0.0)
    print(json.dumps({"secs": secs, "kernel_ms": kernel_ms, "hash": hashlib.sha256(img.cpu().numpy().tobytes()).hexdigest()[:12]}))
    ctx.close()


def run_child(a, accel, lib, leg="oneshot"):
    env = dict(os.environ)
    env.pop("TOR_AB_LIB", None)  # (this build unless the leg names another)
    if lib:
        env["TOR_AB_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child-accel", str(accel), "--child-reps", "1", "--child-leg", leg, "--total", str(a.total),
           "--width", str(a.width), "--height", str(a.height), "--depth", str(a.depth)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--total", type=int, default=1000)
    ap.add_argument("--accel", default="3,0")
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libtor_mi355x.so built from the parent commit (leg a); without it leg (a) is this build in a child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-accel", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-reps", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--child-leg", default="oneshot", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_accel is not None:
        return one_shot_child(a)
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    H, W, N = a.height, a.width, a.total
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context()
    ctx.upload(scene.list())
    stream = torch.cuda.current_stream().cuda_stream
    img = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
    lines, ok = [], True

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"resume_rate: {W}x{H}, {N} spp, depth {a.depth}, random_scene, {a.reps} repetitions, legs interleaved; parent build: {a.parent_lib or '(this build, child process)'}")
    for accel in [int(x) for x in a.accel.split(",")]:
        opt = tor.make_options(seeding=tor.SEED_PIXEL, accel=accel)
        pp = tor.PixelProgressive(ctx, cam, H, W, a.depth, opt)
        kernel_ms = {}

        def one_shot():
            ctx.render_device(cam, H, W, N, 2.2, a.depth, opt, img.data_ptr(), stream)

        def resume(sizes, name):
            pp.samples = 0
            ms = 0.0
            for k in sizes:
                pp.add(k)
                if len(sizes) == 1:
                    ms += ctx.last_kernel_ms()[0]
            ctx.resolve_device(pp.sums.data_ptr(), pp.sums.numel(), N, 2.2, img.data_ptr(), stream)
            if len(sizes) == 1:
                kernel_ms[name] = ms

        p16 = [16] * (N // 16) + ([N % 16] if N % 16 else [])
        name_c = f"c 1 x {N}"
        legs = [(f"d 10 x {N // 10}", lambda: resume([N // 10] * 9 + [N - 9 * (N // 10)], "d"), 10), (f"e {len(p16)} x 16", lambda: resume(p16, "e"), len(p16))]
        one_shot()
        resume([64, 16], "warm")  # warm-up: layouts, code objects of both pass shapes
        torch.cuda.synchronize()
        secs = {name: [] for name, _, _ in legs}
        for name in ("a parent build", "b one launch", name_c):
            secs[name] = []
        digest = {}
        for _ in range(a.reps):
            for name, lib, leg in (("a parent build", a.parent_lib, "oneshot"), ("b one launch", None, "oneshot"), (name_c, None, "resume")):
                c = run_child(a, accel, lib, leg)
                secs[name] += c["secs"]
                digest[name] = c["hash"]
                if leg == "resume":
                    kernel_ms["c"] = c["kernel_ms"][-1]
            for name, fn, _ in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                secs[name].append(time.perf_counter() - t0)
                digest[name] = hashlib.sha256(img.cpu().numpy().tobytes()).hexdigest()[:12]
        rate = lambda s: H * W * N / s / 1e6
        med = {k: statistics.median(v) for k, v in secs.items()}
        sa = secs["a parent build"]
        spread = (max(sa) - min(sa)) / med["a parent build"]
        # state traffic of one pass: 32 B state + 24 B sums per pixel, loaded (first_sample > 0) and stored
        state_bytes = H * W * 56 * 2
        share = (state_bytes / HBM_BYTES_PER_S) / (kernel_ms["c"] / 1e3)
        emit(f"accel {accel}: spread of (a) over {len(sa)} runs = {spread * 100:.2f} %; state traffic of a pass {state_bytes / 1e6:.0f} MB = {share * 100:.4f} % of leg (c)'s kernel time at {HBM_BYTES_PER_S / 1e12:.0f} TB/s")
        emit(f"  {'leg':>16} {'median ms':>10} {'min ms':>9} {'max ms':>9} {'Msamples/s':>11} {'time vs (a)':>12}  hash")
        for name in ["a parent build", "b one launch", name_c] + [n for n, _, _ in legs]:
            v = secs[name]
            emit(f"  {name:>16} {med[name] * 1e3:>10.1f} {min(v) * 1e3:>9.1f} {max(v) * 1e3:>9.1f} {rate(med[name]):>11.1f} {(med[name] / med['a parent build'] - 1) * 100:>+11.2f}%  {digest[name]}"
                 + ("" if digest[name] == digest["b one launch"] else "  DIFFERS"))
            ok = ok and digest[name] == digest["b one launch"]
        b_ok = med["b one launch"] <= med["a parent build"] * (1 + spread)
        c_ok = med[name_c] <= med["a parent build"] * (1 + spread + share)
        emit(f"  condition (b) within (a)'s spread: {'met' if b_ok else 'NOT MET'}; condition (c) within spread + state share: {'met' if c_ok else 'NOT MET'}")
        ok = ok and b_ok and c_ok
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
