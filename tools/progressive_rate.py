#!/usr/bin/env python3
"""Cost of progressive passes (tor_render_accumulate_device) against one launch: random_scene at 1920x1080, TOTAL samples per pixel
(default 1000) rendered as one tor_render_device launch and as passes of 1000 / 500 / 250 / 100 / 25 / 10 samples, for accel 0 and 3,
with and without second moments.  Wall time from the first enqueue to the resolved canvas (host launch overhead and every pass's tail included), best
of REPS (default 2), schedules interleaved per repetition.  Prints a table (Msamples/s, overhead against the one-shot launch, canvas
hash -- every schedule must show the one-shot hash) and one JSON line.

    python tools/progressive_rate.py [--total 1000] [--passes 1,2,4,10,40,100] [--accel 0,3] [--reps 2] [--out FILE.json]
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--total", type=int, default=1000)
    ap.add_argument("--passes", default="1,2,4,10,40,100", help="pass counts (each divides --total)")
    ap.add_argument("--accel", default="0,3")
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W, N = a.height, a.width, a.total
    passes = [int(x) for x in a.passes.split(",")]
    assert all(N % k == 0 for k in passes), "every pass count must divide --total"
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context()
    ctx.upload(scene.list())
    stream = torch.cuda.current_stream().cuda_stream
    sums = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
    mom = torch.empty_like(sums)
    img = torch.empty_like(sums)

    def one_shot(accel):
        ctx.render_device(cam, H, W, N, 2.2, a.depth, tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel), img.data_ptr(), stream)

    def progressive(accel, k, moments):
        opt = tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel)
        sums.zero_()
        if moments:
            mom.zero_()
        step = N // k
        for i in range(k):
            ctx.accumulate_device(cam, H, W, i * step, step, a.depth, opt, sums.data_ptr(), mom.data_ptr() if moments else 0, stream)
        ctx.resolve_device(sums.data_ptr(), sums.numel(), N, 2.2, img.data_ptr(), stream)

    rows = []
    for accel in [int(x) for x in a.accel.split(",")]:
        runs = [("one launch", 1, False, lambda acc=accel: one_shot(acc))]
        for k in passes:
            for moments in (False, True):
                if k == 1 and not moments:
                    runs.append((f"1 x {N} pass", 1, False, lambda acc=accel: progressive(acc, 1, False)))
                else:
                    runs.append((f"{k} x {N // k}" + (" +mom" if moments else ""), k, moments,
                                 lambda acc=accel, kk=k, m=moments: progressive(acc, kk, m)))
        one_shot(accel)  # warm-up: layouts, code objects
        progressive(accel, 2, True)
        torch.cuda.synchronize()
        best = {r[0]: 1e30 for r in runs}
        digest = {}
        for _ in range(a.reps):
            for name, _k, _m, fn in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                best[name] = min(best[name], time.perf_counter() - t0)
                digest[name] = hashlib.sha256(img.cpu().numpy().tobytes()).hexdigest()[:12]
        base = best["one launch"]
        for name, k, moments, _fn in runs:
            rows.append({"accel": accel, "schedule": name, "passes": k, "moments": moments, "ms": round(best[name] * 1e3, 2),
                         "msamples_s": round(H * W * N / best[name] / 1e6, 1), "overhead_pct": round((best[name] / base - 1) * 100, 2),
                         "hash": digest[name], "same_as_one_shot": digest[name] == digest["one launch"]})
    ctx.close()
    print(f"{'accel':>5} {'schedule':>16} {'ms':>9} {'Msamples/s':>11} {'vs one launch':>14}  hash")
    for r in rows:
        print(f"{r['accel']:>5} {r['schedule']:>16} {r['ms']:>9.2f} {r['msamples_s']:>11.1f} {r['overhead_pct']:>+13.2f}%  {r['hash']}"
              + ("" if r["same_as_one_shot"] else "  DIFFERS"))
    line = {"tool": "progressive_rate", "size": f"{W}x{H}", "total_spp": N, "depth": a.depth, "reps": a.reps, "rows": rows}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)
    sys.exit(0 if all(r["same_as_one_shot"] for r in rows) else 1)


if __name__ == "__main__":
    main()
