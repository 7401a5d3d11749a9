#!/usr/bin/env python3
"""Rate of the photon-map queries (tor_photons_build_device, tor_photons_gather_device) against what a host does without them: the
chunked float64 brute force over every (query, photon) pair in torch on the same device -- cdist-style arithmetic, the accept test,
the Epanechnikov weight, the clamp and the rounding to 2^-36, summed per query.  There is no parent-commit figure: the entries are new.

The workload is a photon map as a renderer makes it: n photons uniform on the unit square of the plane z = 0 (a jitter of 1e-3 R in
z), gathered from a square grid of queries on the same plane -- in camera order (row-major: neighbouring lanes walk the same
buckets) and shuffled -- with the radius chosen for an occupancy of about 1, 8 and 64 photons per radius disc
(R = sqrt(occupancy / (pi n))).  Measured per row: the build (the C entry, all six launches) and the gather, HIP events, the legs of
a row interleaved per round, WARM warm-up runs, the median of ROUNDS timings.  The torch leg is linear in the number of queries by
construction (a loop over chunks of queries against all photons), so it is TIMED on 2^10 queries and scaled to the row's count;
the tool says so in its output.  It also checks the library's sums against the torch leg's on those queries, bit for bit.

Expectation (stated before the first run): the gather is not slower than the brute force at any row, and its time grows with
queries x occupancy, not with the photon count.  Rows that miss either are marked.

A last child records, not asserts, the per-pixel variance of trace_photon_map against trace_direct on the caustic frame of
tests/camera_inputs.py with a mirror ball added behind it, and the frame means.

Each photon count runs in a child process of its own under a time limit; the run stops at the first child that fails.

    python tools/photon_rate.py [--photons 65536,524288,4194304] [--queries 65536,1048576] [--rounds 5] [--warm 1] [--out F.txt]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

OCCUPANCIES = (1, 8, 64)
TORCH_QUERIES = 1 << 10


def torch_gather(torch, pos, pw, pts, r2, max_value=1.0):
    """The brute force a host writes today: (sums, count), the queries in chunks of at most 512 and at most 2^26 pairs (512 MiB
    per float64 temporary)."""
    n = pts.shape[0]
    chunk = max(1, min(512, (1 << 26) // max(int(pos.shape[0]), 1)))
    sums = torch.zeros((n, 3), dtype=torch.float64, device=pts.device)
    count = torch.zeros(n, dtype=torch.int32, device=pts.device)
    for lo in range(0, n, chunk):
        x = pts[lo:lo + chunk]
        e0, e1, e2 = (pos[None, :, k] - x[:, None, k] for k in range(3))
        d2 = (e0 * e0 + e1 * e1) + e2 * e2
        acc = d2 < r2
        w = torch.where(acc, 1.0 - d2 / r2, torch.zeros_like(d2))
        for ch in range(3):
            a = pw[None, :, ch] * w
            a = torch.where(a < max_value, a, torch.full_like(a, max_value))
            sums[lo:lo + chunk, ch] = ((a + 98304.0) - 98304.0).sum(dim=1)
        count[lo:lo + chunk] = acc.sum(dim=1)
    return sums, count


def timed(torch, legs, rounds, warm):
    """Median milliseconds per leg: warm-up, then `rounds` rounds with the legs interleaved, each between two HIP events."""
    for _ in range(warm):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, f in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in ms.items()}


def rate_rows(a, n_photons):
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    if not torch.cuda.is_available():
        sys.exit("photon_rate: no GPU -- a rate is measured on the device or not at all")
    ctx = tor.Context()
    L = tor.lib()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261020)
    rows = []
    for occ in OCCUPANCIES:
        radius = float(np.sqrt(occ / (np.pi * n_photons)))
        pos = torch.rand((n_photons, 3), dtype=torch.float64, device="cuda", generator=gen)
        pos[:, 2] = (pos[:, 2] - 0.5) * 1e-3 * radius
        pw = torch.rand((n_photons, 3), dtype=torch.float64, device="cuda", generator=gen)
        stream = torch.cuda.current_stream().cuda_stream

        def build():
            rc = L.tor_photons_build_device(ctx._h, n_photons, pos.data_ptr(), pw.data_ptr(), None, None, n_photons, radius, stream)
            if rc != 0:
                raise RuntimeError(L.tor_last_error().decode())
        build()
        ctx._photon_scale, ctx._photon_radius = 1.0, radius   # (the C entry was called directly: the powers are unscaled)
        info = ctx.photons_info()
        legs = {"build": build}
        sets = {}
        for nq in a.queries:
            side = int(round(np.sqrt(nq)))
            g = (torch.arange(side, dtype=torch.float64, device="cuda") + 0.5) / side
            cam = torch.stack([g[None, :].expand(side, side), g[:, None].expand(side, side), torch.zeros((side, side), dtype=torch.float64,
                                                                                                       device="cuda")], dim=2).reshape(-1, 3).contiguous()
            shuf = cam[torch.randperm(cam.shape[0], device="cuda", generator=gen)].contiguous()
            for order, pts in (("camera", cam), ("shuffled", shuf)):
                out = ctx.gather_photons(pts)
                sets[(nq, order)] = (pts, out)
                legs[f"gather {nq} {order}"] = (lambda pts=pts, out=out: ctx.gather_photons(pts, out=out))
        sub = sets[(a.queries[0], "shuffled")][0][:TORCH_QUERIES].contiguous()
        r2 = radius * radius
        legs["torch"] = lambda: torch_gather(torch, pos, pw, sub, r2)
        med = timed(torch, legs, a.rounds, a.warm)
        want_s, want_c = torch_gather(torch, pos, pw, sub, r2)
        got = ctx.gather_photons(sub)
        torch.cuda.synchronize()
        differ = int((got.sums.view(torch.int64) != want_s.view(torch.int64)).any(dim=1).sum()) + int((got.count != want_c).sum())
        for (nq, order), (pts, out) in sets.items():
            t = med[f"gather {nq} {order}"]
            brute = med["torch"] * pts.shape[0] / TORCH_QUERIES
            rows.append({"photons": n_photons, "occupancy": occ, "radius": radius, "queries": int(pts.shape[0]), "order": order,
                         "build_ms": round(med["build"], 4), "gather_ms": round(t, 4), "torch_ms_scaled": round(brute, 2),
                         "torch_ms_timed": round(med["torch"], 3), "mean_count": float(out.count.double().mean()),
                         "largest_bucket": info["largest_bucket"], "n_buckets": info["n_buckets"], "differ": differ,
                         "mqueries_s": round(pts.shape[0] / t / 1e3, 2), "device": torch.cuda.get_device_name(0)})
    ctx.close()
    print("ROW " + json.dumps(rows))
    return 0


def variances():
    """The child of the variance record: the caustic frame of tests/camera_inputs.py with a mirror ball behind the caustic."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import camera_inputs as I
    import light_inputs as LI
    tor = importlib.import_module("trace-of-radiance_amd")
    side, runs, depth, paths, radius = 16, 16, 8, 1 << 17, 0.08
    recs, emission, lamp = I.caustic_scene()
    recs = np.vstack([recs, np.array([LI._sphere((0.9, -0.2, -2.5), 1.5, LI.METAL, (0.9, 0.9, 0.9), 0.0)])])
    emission = np.vstack([emission, np.zeros((1, 3))])
    scene = tor.Scene.from_records(recs)
    ctx = tor.Context()
    ctx.upload(scene.list())
    ctx.set_lights([lamp])
    cam = I.frame_camera(tor)
    diffuse = tor.diffuse_objects(scene)
    rays, rng = ctx.camera_rays(cam, side, side, 0, runs)
    lum = ctx.trace_direct(rays, rng.clone(), emission, diffuse, depth)[0].mean(dim=1).reshape(side * side, runs).cpu().numpy()
    var = lum.var(axis=1, ddof=1)
    rows = [{"estimator": "trace_direct", "frame_mean": float(lum.mean()), "mean_pixel_variance": float(var.mean()),
             "max_pixel_variance": float(var.max()), "note": f"{runs} samples per pixel"}]
    est = []
    for b in range(runs):     # one camera sample per pixel against a photon map of its own: independent estimates
        st = torch.from_numpy(tor.rng_seed2(np.full(paths, 1000 + b, dtype=np.uint64), np.arange(paths, dtype=np.uint64)).view(np.int64)).cuda()
        ph = ctx.trace_photons(st, emission, diffuse, depth)
        ctx.build_photons(ph.position, ph.power, ph.direction, radius=radius)
        r1, g1 = ctx.camera_rays(cam, side, side, b, 1)
        est.append(ctx.trace_photon_map(r1, g1, emission, diffuse, ph.paths, max_depth=depth)[0].mean(dim=1).cpu().numpy())
    est = np.array(est)
    var = est.var(axis=0, ddof=1)
    rows.append({"estimator": "trace_photon_map", "frame_mean": float(est.mean()), "mean_pixel_variance": float(var.mean()),
                 "max_pixel_variance": float(var.max()), "note": f"{runs} runs of one sample per pixel, each with a map of {paths} light paths, "
                                                                 f"radius {radius} (biased by the kernel's blur; a miss is black in both)"})
    ctx.close()
    print("ROW " + json.dumps(rows))
    return 0


def child(args, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"photon_rate: {what} ran past {limit} s -- stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"photon_rate: {what} failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", default="65536,524288,4194304")
    ap.add_argument("--queries", default="65536,1048576")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a photon count may take")
    ap.add_argument("--row", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photon_rate.txt"))
    a = ap.parse_args()
    a.queries = [int(v) for v in a.queries.split(",")]
    if a.row == "variances":
        return variances()
    if a.row:
        return rate_rows(a, int(a.row))
    common = ["--queries", ",".join(str(q) for q in a.queries), "--rounds", str(a.rounds), "--warm", str(a.warm)]
    rows = []
    for n in [int(v) for v in a.photons.split(",")]:   # each GPU step under its own limit; stop at the first that fails
        rc, got = child(["--row", str(n)] + common, a.step_timeout, f"{n} photons")
        if rc:
            return rc
        rows += got
    rc, var = child(["--row", "variances"], a.step_timeout, "the variance record")
    if rc:
        return rc
    lines = [f"photon_rate: milliseconds, median of {a.rounds} rounds after {a.warm} warm-up, HIP events, legs interleaved; {rows[0]['device']}",
             f"torch = the chunked float64 brute force over all pairs, timed on {TORCH_QUERIES} queries and scaled linearly to the row's count",
             "photons uniform on the unit square, R = sqrt(occupancy / (pi n)); count = mean accepted photons per query; differ = queries of "
             "the timed torch leg whose bits differ from the library's (none expected)",
             f"{'photons':>9}{'occ':>5}{'queries':>9} {'order':<9}{'build ms':>10}{'gather ms':>11}{'Mq/s':>9}{'torch ms':>12}{'torch/lib':>11}"
             f"{'count':>8}{'max bucket':>11}{'differ':>8}  marks"]
    base = {}
    for r in rows:
        key = (r["occupancy"], r["queries"], r["order"])
        base.setdefault(key, r["gather_ms"])      # the smallest photon count's time for the same queries x occupancy
        marks = []
        if r["gather_ms"] > r["torch_ms_scaled"]:
            marks.append("SLOWER THAN TORCH")
        if r["gather_ms"] > 2.0 * base[key]:
            marks.append(f"{r['gather_ms'] / base[key]:.1f}x the time at {rows[0]['photons']} photons")
        lines.append(f"{r['photons']:>9}{r['occupancy']:>5}{r['queries']:>9} {r['order']:<9}{r['build_ms']:>10.3f}{r['gather_ms']:>11.3f}"
                     f"{r['mqueries_s']:>9.1f}{r['torch_ms_scaled']:>12.1f}{r['torch_ms_scaled'] / r['gather_ms']:>11.0f}{r['mean_count']:>8.1f}"
                     f"{r['largest_bucket']:>11}{r['differ']:>8}  {'; '.join(marks)}")
    lines += ["", "per-pixel variance on the caustic frame of tests/camera_inputs.py with a mirror ball behind the caustic (16 x 16 pixels, depth 8): "
              "recorded, not asserted", f"{'estimator':<18}{'frame mean':>12}{'mean pixel variance':>22}{'max pixel variance':>21}  note"]
    for v in var:
        lines.append(f"{v['estimator']:<18}{v['frame_mean']:>12.5f}{v['mean_pixel_variance']:>22.5g}{v['max_pixel_variance']:>21.5g}  {v['note']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "photon_rate", "unit": "ms", "rows": rows, "variances": var}))
    return 1 if any(r["differ"] for r in rows) else 0


if __name__ == "__main__":
    sys.exit(main())
