#!/usr/bin/env python3
"""Rate of the BSDF query (tor_bsdf_eval_device) against what a host does without it -- the same arithmetic in batched torch float64
on the same device: the gather of the material by object, unit_vector, reflect, the cross product, the two closed forms and the
selects, elementwise in include/tor_bsdf.h's order.  M items/s for 2^20 items on an all-Lambertian scene, an all-Metal one
(fuzz 0.3) and random_scene's mix of materials (objects drawn uniformly per item).  Legs, interleaved per round between HIP
events: the library (one launch into outputs allocated before the timing) and torch.  Every leg: WARM warm-up runs, then ROUNDS
timings of REPS back-to-back runs; the median over the rounds.  torch fuses nothing either, but its division by a constant need
not be the correctly rounded one, so the legs agree to rounding; the tool counts the items whose bits differ.  No rate is fixed
in advance; a row in which the library is slower than the torch leg is reported as it is.

A last child records the per-pixel variance of trace_direct with and without glossy= (and of trace) on the glossy-floor frame of
tests/bsdf_inputs.py: recorded, not asserted.

Each row runs in a child process of its own under a time limit; the run stops at the first child that fails.

    python tools/bsdf_rate.py [--items 1048576] [--reps 10] [--rounds 5] [--warm 2] [--out profiles/bsdf_rate.txt]
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

ROWS = ("lambertian", "metal", "random_scene")
# the words the kernel touches: direction of `in` (Metal alone) and of `out`, normal and word 7 of the record; value, pdf and kind
# out; plus the gathered cold record (word 13, then 9..12), which a scene of a few hundred objects keeps in the cache
IN_BYTES, HIT_BYTES, OUT_BYTES, COLD_BYTES, RESULT_BYTES = 24, 32, 24, 40, 24 + 8 + 4
PI = 3.141592653589793


def torch_bsdf(torch, mats, rin, raw, rout):
    """include/tor_bsdf.h in torch: (value, pdf, kind).  mats: (n_objects, 5) float64 {kind, albedo rgb, fuzz}."""
    obj = raw.view(torch.int32)[:, 14].long()
    n_obj = mats.shape[0]
    known = (obj >= 0) & (obj < n_obj)
    m = mats[obj.clamp(0, n_obj - 1)]
    mat, albedo, fuzz = m[:, 0], m[:, 1:4], m[:, 4]
    dense = known & ((mat == 0.0) | ((mat == 1.0) & (fuzz != 0.0)))
    dot = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]
    d_in, nrm, out = rin[:, 3:6], raw[:, 3:6], rout[:, 3:6]
    oo = dot(out, out)
    w = out * (1.0 / torch.sqrt(oo))[:, None]
    gate = dot(out, nrm) > 0
    c = dot(w, nrm)
    zero = torch.zeros_like(c)
    lam = torch.where(c > 0, c / PI, zero)
    ud = d_in * (1.0 / torch.sqrt(dot(d_in, d_in)))[:, None]
    r = ud - nrm * (2.0 * dot(ud, nrm))[:, None]
    f = fuzz.abs()
    b = dot(w, r)
    x = torch.stack((w[:, 1] * r[:, 2] - w[:, 2] * r[:, 1], w[:, 2] * r[:, 0] - w[:, 0] * r[:, 2],
                     w[:, 0] * r[:, 1] - w[:, 1] * r[:, 0]), dim=1)
    h = f * f - dot(x, x)
    q = torch.sqrt(h)
    lo, hi = b - q, b + q
    f3 = f * f * f
    met = torch.where(h > 0, torch.where(lo > 0, (q * (3.0 * b * b + h)) / (2.0 * PI * f3),
                                         torch.where(hi > 0, (hi * hi * hi) / (4.0 * PI * f3), zero)), zero)
    p = torch.where(dense & (oo > 0) & (oo < float("inf")) & gate, torch.where(mat == 0.0, lam, met), zero)
    value = torch.where(dense[:, None], albedo * p[:, None], torch.zeros_like(albedo))
    kind = torch.where(dense, 1, torch.where(known, 2, 0)).to(torch.int32)
    return value, p, kind


def measure(torch, a, legs, m):
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
    return med, {leg: m / (med[leg] * 1e-3) / 1e6 for leg in legs}


def scene_records(tor, name):
    recs = tor.random_scene().to_records()
    if name == "lambertian":
        recs[:, 10], recs[:, 14] = 0.0, 0.0
    elif name == "metal":
        recs[:, 10], recs[:, 14] = 1.0, 0.3
    recs[:, 11:14] = np.where(recs[:, 10:11] == 2.0, 0.0, np.maximum(recs[:, 11:14], 0.05))
    return recs


def rate_row(a, name):
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    if not torch.cuda.is_available():
        sys.exit("bsdf_rate: no GPU -- a rate is measured on the device or not at all")
    recs = scene_records(tor, name)
    ctx = tor.Context()
    ctx.upload(tor.Scene.from_records(recs).list())
    m = a.items
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019)
    unit = lambda v: v / torch.sqrt((v * v).sum(dim=1))[:, None]
    nrm = unit(torch.randn((m, 3), dtype=torch.float64, device="cuda", generator=gen))
    d_in = unit(torch.randn((m, 3), dtype=torch.float64, device="cuda", generator=gen))
    d_in = torch.where(((d_in * nrm).sum(dim=1) > 0)[:, None], -d_in, d_in)
    obj = torch.randint(0, recs.shape[0], (m,), dtype=torch.int32, device="cuda", generator=gen)
    mats = torch.from_numpy(np.ascontiguousarray(recs[:, [10, 11, 12, 13, 14]])).cuda()
    # out: about the reflected direction, inside or just around the widest lobe, so that every branch is taken
    ud = d_in
    refl = ud - nrm * (2.0 * (ud * nrm).sum(dim=1))[:, None]
    ball = unit(torch.randn((m, 3), dtype=torch.float64, device="cuda", generator=gen)) \
        * torch.rand((m, 1), dtype=torch.float64, device="cuda", generator=gen) ** (1.0 / 3.0)
    spread = torch.where(mats[obj.long(), 0] == 1.0, 1.2 * mats[obj.long(), 4].abs(), torch.full((m,), 1.5, dtype=torch.float64, device="cuda"))
    d_out = (refl + ball * spread[:, None]) * (0.1 + 9.9 * torch.rand((m, 1), dtype=torch.float64, device="cuda", generator=gen))
    rin = torch.zeros((m, 7), dtype=torch.float64, device="cuda")
    rout = torch.zeros((m, 7), dtype=torch.float64, device="cuda")
    raw = torch.zeros((m, 8), dtype=torch.float64, device="cuda")
    rin[:, 3:6], rout[:, 3:6], raw[:, 3:6] = d_in * 2.0, d_out, nrm
    raw.view(torch.int32)[:, 14] = obj
    got = ctx.bsdf(rin, raw, rout)
    value, pdf, kind = torch_bsdf(torch, mats, rin, raw, rout)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int64)
    mat_of = mats[obj.long(), 0]
    check = {"pdf_differ": int((bits(pdf) != bits(got.pdf)).sum()), "value_differ": int((bits(value) != bits(got.value)).any(dim=1).sum()),
             "kind_differ": int((kind != got.kind).sum()), "density": int((got.kind == 1).sum()), "delta": int((got.kind == 2).sum()),
             "positive": int((got.pdf > 0).sum())}
    metal = float(((mat_of == 1.0) & (got.kind == 1)).double().mean())
    per_item = OUT_BYTES + HIT_BYTES + RESULT_BYTES + COLD_BYTES + metal * IN_BYTES
    out = ctx.bsdf(rin, raw, rout)
    legs = {"library": lambda: ctx.bsdf(rin, raw, rout, out=out), "torch": lambda: torch_bsdf(torch, mats, rin, raw, rout)}
    med, rate = measure(torch, a, legs, m)
    ctx.close()
    print("ROW " + json.dumps({"case": name, "items": m, "ms": {k: round(v, 4) for k, v in med.items()},
                               "mitems_s": {k: round(v, 2) for k, v in rate.items()}, "bytes_per_item": round(per_item, 1),
                               "gb_s": round(rate["library"] * 1e6 * per_item / 1e9, 1),
                               "library_vs_torch": round(rate["library"] / rate["torch"], 1), "check": check,
                               "device": torch.cuda.get_device_name(0)}))
    return 0


def variances():
    """The child of the variance record: the glossy-floor frame of tests/bsdf_inputs.py, 8 x 8 pixels, 64 samples each, depth 4."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bsdf_inputs as I
    tor = importlib.import_module("trace-of-radiance_amd")
    side, spp, depth = 8, 64, 4
    recs, emission = I.glossy_scene()
    scene = tor.Scene.from_records(recs)
    ctx = tor.Context()
    ctx.upload(scene.list())
    ctx.set_lights([I.G_LAMP])
    ctx.set_groups(np.where(np.arange(len(recs)) == I.G_LAMP, 2, 1).astype(np.uint32))
    rays, rng = ctx.camera_rays(I.glossy_camera(tor), side, side, 0, spp)
    diffuse, glossy = tor.diffuse_objects(scene), tor.glossy_objects(scene)
    black = lambda r, idx: torch.zeros((len(idx), 3), dtype=torch.float64, device=r.device)
    kw = dict(max_depth=depth, sky=black, lamp_mask=1)
    runs = {"trace": lambda: ctx.trace(rays, rng.clone(), depth, sky=black, emission=emission)[0],
            "trace_direct": lambda: ctx.trace_direct(rays, rng.clone(), emission, diffuse, **kw)[0],
            "trace_direct mis": lambda: ctx.trace_direct(rays, rng.clone(), emission, diffuse, mis=True, **kw)[0],
            "glossy": lambda: ctx.trace_direct(rays, rng.clone(), emission, diffuse, glossy=glossy, **kw)[0],
            "glossy mis": lambda: ctx.trace_direct(rays, rng.clone(), emission, diffuse, mis=True, glossy=glossy, **kw)[0]}
    rows = []
    for name, run in runs.items():
        lum = run().mean(dim=1).reshape(side * side, spp).cpu().numpy()
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
        print(f"bsdf_rate: {what} ran past {limit} s -- stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"bsdf_rate: {what} failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a row may take")
    ap.add_argument("--row", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsdf_rate.txt"))
    a = ap.parse_args()
    if a.row == "variances":
        return variances()
    if a.row:
        return rate_row(a, a.row)
    common = ["--items", str(a.items), "--reps", str(a.reps), "--rounds", str(a.rounds), "--warm", str(a.warm)]
    rows = []
    for row in ROWS:   # each GPU step under its own limit; stop at the first that fails
        rc, got = child(["--row", row] + common, a.step_timeout, row)
        if rc:
            return rc
        rows.append(got)
    rc, var = child(["--row", "variances"], a.step_timeout, "the variance record")
    if rc:
        return rc
    lines = [f"bsdf_rate: M items/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events; {rows[0]['device']}",
             f"accounting, from the words touched: an item reads {OUT_BYTES} bytes of `out` (direction), {HIT_BYTES} of the record (normal, word 7), "
             f"{COLD_BYTES} of the gathered cold record (word 13, words 9..12) and, for a Metal with a density, {IN_BYTES} of `in` (direction); it "
             f"writes {RESULT_BYTES} (value, pdf, kind); GB/s = library rate x these (the strided records' cache lines carry more)",
             f"{'case':<14}{'items':>9}{'bytes/item':>12}{'library':>11}{'GB/s':>9}{'torch':>11}{'lib/torch':>11}  agreement with the torch leg"]
    for r in rows:
        g, c = r["mitems_s"], r["check"]
        lines.append(f"{r['case']:<14}{r['items']:>9}{r['bytes_per_item']:>12.1f}{g['library']:>11.1f}{r['gb_s']:>9.1f}{g['torch']:>11.2f}"
                     f"{r['library_vs_torch']:>11.1f}  " + ", ".join(f"{k} {v}" for k, v in c.items()))
    slower = [r["case"] for r in rows if r["library_vs_torch"] < 1.0]
    lines.append("rows slower than the torch leg: " + (", ".join(slower) if slower else "none"))
    lines += ["", "per-pixel variance on the glossy-floor frame of tests/bsdf_inputs.py (8 x 8 pixels, 64 samples per pixel, depth 4, black sky; "
              "without glossy= the Metal floor with fuzz 0.3 is booked specular and finds the lamp by chance): recorded, not asserted",
              f"{'estimator':<18}{'frame mean':>12}{'std error':>12}{'mean pixel variance':>22}{'max pixel variance':>21}"]
    for v in var:
        lines.append(f"{v['estimator']:<18}{v['frame_mean']:>12.5f}{v['standard_error']:>12.5f}{v['mean_pixel_variance']:>22.5g}"
                     f"{v['max_pixel_variance']:>21.5g}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "bsdf_rate", "unit": "M items/s", "rows": rows, "variances": var}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
