#!/usr/bin/env python3
"""Rates of the environment-light sampler (tor_env_sample_device) against what a host does without it -- the same tables and the
same states in batched torch float64 arithmetic on the same device: the generator's four draws in int64 tensor arithmetic,
torch.searchsorted over the marginal sums, a binary search of gathers over the picked row's running sums, the octahedral decode and
the density, elementwise in the header's order.  M points/s for n in 16, 256, 1024, 2048 and two maps: `uniform` (random texels:
the picks spread over every row) and `sun` (the same with one texel holding 99 % of the importance: one hot row).  Legs,
interleaved per round between HIP events: the library (one launch into outputs allocated before the timing; the states are written
again and again) and torch.  Every leg: WARM warm-up runs, then ROUNDS timings of REPS back-to-back runs; the median over the
rounds.  Both legs read the same running sums (summed sequentially on the host), so the tool counts the points whose texel or
density differ in any bit and expects none.  No rate is fixed in advance; the library is expected not to be slower than the torch
leg in any row, and a row under 1x is reported as it is.

A last child records the per-pixel sample variances of the three estimators of tests/test_gpu_env_query.py's frame (scattered rays
alone, next-event estimation, MIS): recorded, not asserted.

Each row runs in a child process of its own under a time limit; the run stops at the first child that fails.

    python tools/env_sample_rate.py [--points 1048576] [--reps 10] [--rounds 5] [--warm 2] [--out profiles/env_sample_rate.txt]
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

SIDES = (16, 256, 1024, 2048)
KINDS = ("uniform", "sun")
BYTES_PER_POINT = 32 + 32 + 32 + 56 + 8 + 4 + 24     # point and state in; state, ray, pdf, texel and colour out


def make_map(n, kind):
    rs = np.random.RandomState(n)
    rgb = rs.uniform(0.05, 1.0, size=(n, n, 3))
    if kind == "sun":
        lum = (0.2126 * rgb[:, :, 0] + 0.7152 * rgb[:, :, 1]) + 0.0722 * rgb[:, :, 2]
        rgb[(2 * n) // 3, n // 3] = np.array([1.0, 0.9, 0.7]) * (99.0 * lum.sum() / 0.9)
    return rgb


def host_tables(rgb):
    """The header's tables in numpy: I (n, n), cum (n, n) and M (n,), every running sum sequential."""
    n = rgb.shape[0]
    h = 2.0 / n
    s = ((np.arange(n) + 0.5) * h - 1.0)[None, :] * np.ones((n, 1))
    t = ((np.arange(n) + 0.5) * h - 1.0)[:, None] * np.ones((1, n))
    py = (1.0 - np.abs(s)) - np.abs(t)
    px = np.where(py >= 0, s, np.copysign(1.0 - np.abs(t), s))
    pz = np.where(py >= 0, t, np.copysign(1.0 - np.abs(s), t))
    ln = np.sqrt(px * px + py * py + pz * pz)
    lum = (0.2126 * rgb[:, :, 0] + 0.7152 * rgb[:, :, 1]) + 0.0722 * rgb[:, :, 2]
    imp = lum * (1.0 / ((ln * ln) * ln))
    cum = np.add.accumulate(imp, axis=1)                                  # (ufunc.accumulate adds in order)
    marg = np.add.accumulate(cum[:, -1].copy())
    return imp, cum, marg


def torch_draws(torch, st, count=4):
    """uniform01 of xoshiro256+ (support/rng.nim:58-74, 129-133) per row of the (n, 4) int64 states, in tensor arithmetic."""
    def lsr(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)

    s0, s1, s2, s3 = (st[:, k].clone() for k in range(4))
    us = []
    for _ in range(count):
        out = s0 + s3
        t = s1 << 17
        s2 = s2 ^ s0
        s3 = s3 ^ s1
        s1 = s1 ^ s2
        s0 = s0 ^ s3
        s2 = s2 ^ t
        s3 = (s3 << 45) | lsr(s3, 19)
        us.append((lsr(out, 12) | 0x3FF0000000000000).view(torch.float64) - 1.0)
    return us, torch.stack((s0, s1, s2, s3), dim=1)


def torch_sample(torch, tabs, pts, st):
    """What a host writes today, on the library's own tables: (texel (m,), pdf (m,), rays (m, 7), colour (m, 3), states)."""
    n, imp, cum, marg, rgb = tabs
    (u0, u1, u2, u3), st2 = torch_draws(torch, st)
    T = marg[n - 1]
    row = torch.searchsorted(marg, u0 * T, right=True).clamp(max=n - 1)   # the first r with M_r > x
    base = row * n
    y = u1 * cum[base + (n - 1)]
    lo, hi = torch.zeros_like(row), torch.full_like(row, n - 1)           # the first c with cum[row][c] > y: it exists, y < S_row
    for _ in range(max(1, (n - 1).bit_length())):
        mid = (lo + hi) >> 1
        above = cum[base + mid] > y
        hi = torch.where(above, mid, hi)
        lo = torch.where(above, lo, torch.clamp(mid + 1, max=n - 1))
    col = hi
    cell = base + col
    h = 2.0 / float(n)
    s = (col.to(torch.float64) + u2) * h - 1.0
    t = (row.to(torch.float64) + u3) * h - 1.0
    py = (1.0 - s.abs()) - t.abs()
    up = py >= 0
    px = torch.where(up, s, torch.copysign(1.0 - t.abs(), s))
    pz = torch.where(up, t, torch.copysign(1.0 - s.abs(), t))
    ln = torch.sqrt(px * px + py * py + pz * pz)
    inv = 1.0 / ln
    ray = torch.empty((row.shape[0], 7), dtype=torch.float64, device=row.device)
    ray[:, 0:3], ray[:, 6] = pts[:, 0:3], pts[:, 3]
    ray[:, 3], ray[:, 4], ray[:, 5] = px * inv, py * inv, pz * inv
    pdf = ((imp[cell] / T) * ((float(n) * float(n)) * 0.25)) * ((ln * ln) * ln)
    return cell, pdf, ray, rgb[cell], st2


def one_row(a, n, kind):
    """The child: one map; prints one JSON line."""
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    if not torch.cuda.is_available():
        sys.exit("env_sample_rate: no GPU -- a rate is measured on the device or not at all")
    rgb_np = make_map(n, kind)
    imp_np, cum_np, marg_np = host_tables(rgb_np)
    m = a.points
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019 + n)
    pts = torch.rand((m, 4), dtype=torch.float64, device="cuda", generator=gen)
    st0 = torch.randint(-(1 << 62), 1 << 62, (m, 4), dtype=torch.int64, device="cuda", generator=gen) * 2 + 1
    ctx = tor.Context()
    ctx.set_environment(rgb_np)
    tabs = (n, torch.from_numpy(imp_np.reshape(-1)).cuda(), torch.from_numpy(cum_np.reshape(-1)).cuda(), torch.from_numpy(marg_np).cuda(),
            torch.from_numpy(rgb_np.reshape(-1, 3)).cuda())
    # the check, from the same states
    st = st0.clone()
    got = ctx.sample_environment(pts, st)
    cell, pdf, ray, color, st2 = torch_sample(torch, tabs, pts, st0)
    torch.cuda.synchronize()
    check = {"states_equal": bool(torch.equal(st2, st)), "texels_differ": int((cell != got.texel.long()).sum()),
             "pdf_differ": int((pdf.view(torch.int64) != got.pdf.view(torch.int64)).sum()),
             "rays_differ": int((ray.view(torch.int64) != got.rays.view(torch.int64)).any(dim=1).sum()),
             "colors_differ": int((color != got.color).any(dim=1).sum()), "rows_picked": int(torch.unique(got.texel // n).numel())}
    st = st0.clone()
    out = ctx.sample_environment(pts, st)
    legs = {"library": lambda: ctx.sample_environment(pts, st, out=out), "torch": lambda: torch_sample(torch, tabs, pts, st0)}
    for leg in legs:
        for _ in range(a.warm):
            legs[leg]()
    torch.cuda.synchronize()
    ms = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                legs[leg]()
            e1.record()
            torch.cuda.synchronize()
            ms[leg].append(e0.elapsed_time(e1) / a.reps)
    med = {leg: statistics.median(ms[leg]) for leg in legs}
    rate = {leg: m / (med[leg] * 1e-3) / 1e6 for leg in legs}
    ctx.close()
    print("ROW " + json.dumps({"n": n, "map": kind, "points": m, "ms": {k: round(v, 4) for k, v in med.items()},
                               "mpoints_s": {k: round(v, 2) for k, v in rate.items()},
                               "gb_s": round(rate["library"] * 1e6 * BYTES_PER_POINT / 1e9, 1),
                               "library_vs_torch": round(rate["library"] / rate["torch"], 1), "check": check,
                               "device": torch.cuda.get_device_name(0)}))
    return 0


def variances():
    """The child of the variance record: the frame of tests/test_gpu_env_query.py, the three estimators."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import env_inputs as I
    tor = importlib.import_module("trace-of-radiance_amd")
    side, spp, depth, map_n = 8, 64, 8, 64
    scene = tor.Scene.from_records(I.open_scene())
    ctx = tor.Context()
    ctx.upload(scene.list())
    ctx.set_environment(I.sun_sky(tor.environment_directions(map_n)))
    cam = tor.camera(look_from=(0.0, 1.0, 3.0), look_at=(0.0, 0.0, -1.0), vertical_field_of_view=40.0, aspect_ratio=1.0,
                     aperture=0.0, focus_distance=1.0, shutter_open=0.0, shutter_close=0.0)
    rays, rng = ctx.camera_rays(cam, side, side, 0, spp)
    diffuse = tor.diffuse_objects(scene)
    rows = []
    for name, kw in (("direct=False", dict(direct=False)), ("direct=True", dict()), ("mis=True", dict(mis=True))):
        color = ctx.trace_environment(rays, rng.clone(), diffuse, depth, **kw)[0]
        torch.cuda.synchronize()
        lum = color.cpu().numpy().mean(axis=1).reshape(side * side, spp)
        var = lum.var(axis=1, ddof=1)
        rows.append({"estimator": name, "frame_mean": float(lum.mean()), "standard_error": float(np.sqrt((var / spp).sum()) / (side * side)),
                     "mean_pixel_variance": float(var.mean()), "max_pixel_variance": float(var.max())})
    ctx.close()
    print("ROW " + json.dumps(rows))
    return 0


def child(args, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"env_sample_rate: {what} ran past {limit} s -- stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"env_sample_rate: {what} failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a row may take")
    ap.add_argument("--row", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_sample_rate.txt"))
    a = ap.parse_args()
    if a.row == "variances":
        return variances()
    if a.row:
        n, kind = a.row.split(":")
        return one_row(a, int(n), kind)
    rows = []
    for n in SIDES:                                                       # each GPU step under its own limit; stop at the first that fails
        for kind in KINDS:
            rc, row = child(["--row", f"{n}:{kind}", "--points", str(a.points), "--reps", str(a.reps), "--rounds", str(a.rounds),
                             "--warm", str(a.warm)], a.step_timeout, f"n = {n} ({kind})")
            if rc:
                return rc
            rows.append(row)
    rc, var = child(["--row", "variances"], a.step_timeout, "the variance record")
    if rc:
        return rc
    lines = [f"env_sample_rate: M points/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events; "
             f"{rows[0]['device']}",
             f"accounting: a sampled point moves {BYTES_PER_POINT} bytes (32 point + 32 state in; 32 state + 56 ray + 8 pdf + 4 texel + "
             f"24 colour out) besides the table reads; GB/s = library rate x {BYTES_PER_POINT} B",
             f"{'n':>6}  {'map':<9}{'points':>9}{'library':>11}{'GB/s':>9}{'torch':>11}{'lib/torch':>11}  states=  texels differ  pdf differ  "
             f"rays differ  rows picked"]
    for r in rows:
        g, c = r["mpoints_s"], r["check"]
        lines.append(f"{r['n']:>6}  {r['map']:<9}{r['points']:>9}{g['library']:>11.1f}{r['gb_s']:>9.1f}{g['torch']:>11.2f}"
                     f"{r['library_vs_torch']:>11.1f}  {c['states_equal']!s:<7}  {c['texels_differ']:>13}  {c['pdf_differ']:>10}  "
                     f"{c['rays_differ']:>11}  {c['rows_picked']:>11}")
    lines += ["", "per-pixel sample variance of the three estimators of tests/test_gpu_env_query.py's frame (8 x 8 pixels, 64 samples, depth 8, "
              "the 64 x 64 gradient-plus-sun map): recorded, not asserted",
              f"{'estimator':<14}{'frame mean':>12}{'std error':>12}{'mean pixel variance':>22}{'max pixel variance':>21}"]
    for v in var:
        lines.append(f"{v['estimator']:<14}{v['frame_mean']:>12.5f}{v['standard_error']:>12.5f}{v['mean_pixel_variance']:>22.5g}"
                     f"{v['max_pixel_variance']:>21.5g}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "env_sample_rate", "unit": "M points/s", "rows": rows, "variances": var}))
    ok = all(r["check"]["states_equal"] and not r["check"]["texels_differ"] and not r["check"]["pdf_differ"] for r in rows)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
