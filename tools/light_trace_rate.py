#!/usr/bin/env python3
"""Rates of the light-tracing queries (tor_camera_connect_device, tor_light_emit_device) against what a host does without them --
the same arithmetic on the same states in batched torch float64 on the same device: the generator's draws in int64 tensor
arithmetic, torch.searchsorted over the running sums, the lens point, the projection and the factor, the sphere point and the
cosine-weighted direction, elementwise in the header's order.  M points/s (paths/s) for a pinhole and a thin-lens camera and for
light tables of 1, 256 and 4096 lights.  Legs, interleaved per round between HIP events: the library (one launch into outputs
allocated before the timing; the states are written again and again) and torch.  Every leg: WARM warm-up runs, then ROUNDS timings
of REPS back-to-back runs; the median over the rounds.  torch's sin / cos are not the library's portable routine, so the legs
agree to rounding, not in every bit: the tool counts the pixels / lights that differ (a point within an ulp of a pixel border may)
and reports the largest difference of the factor (relative) and of the ray words (absolute).  No rate is fixed in advance; a row
in which the library is slower than the torch leg is reported as it is.

A last child records the per-pixel variance of trace_direct against trace_light on the caustic frame of tests/camera_inputs.py:
recorded, not asserted.

Each row runs in a child process of its own under a time limit; the run stops at the first child that fails.

    python tools/light_trace_rate.py [--points 1048576] [--reps 10] [--rounds 5] [--warm 2] [--out profiles/light_trace_rate.txt]
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

CAMERAS = {"pinhole": 0.0, "thin lens": 0.5}
LIGHTS = (1, 256, 4096)
CONNECT_BYTES = 32 + 32 + 32 + 56 + 4 + 8           # point and state in; state, ray, pixel and factor out
EMIT_BYTES = 32 + 32 + 56 + 24 + 4 + 16             # state in; state, ray, normal, light and densities out
TWO_PI, PI = 2.0 * 3.141592653589793, 3.141592653589793
NROWS, NCOLS = 1080, 1920


def torch_draws(torch, st, count):
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


def torch_connect(torch, cam, nrows, ncols, pts, st):
    """include/tor_camera.h's connection in torch: (pixel, factor, rays, states)."""
    origin, llc, H, V, u, v, w = (cam[3 * k:3 * k + 3] for k in range(7))
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    fd = dot(origin - llc, w)
    HH, VV = dot(H, H), dot(V, V)
    K = fd * fd * float(ncols - 1) * float(nrows - 1) / (np.sqrt(HH) * np.sqrt(VV))
    (u0, u1), st2 = torch_draws(torch, st, 2)
    lr = float(cam[21]) * torch.sqrt(u0)
    ang = u1 * TWO_PI
    rdx, rdy = lr * torch.cos(ang), lr * torch.sin(ang)
    y = [pts[:, k] for k in range(3)]
    x = [float(origin[k]) + float(u[k]) * rdx + float(v[k]) * rdy for k in range(3)]
    e = [y[k] - x[k] for k in range(3)]
    z = -dot(e, [float(c) for c in w])
    kk = fd / z
    q = [(x[k] + e[k] * kk) - float(llc[k]) for k in range(3)]
    a = dot(q, [float(c) for c in H]) / HH * float(ncols - 1)
    b = dot(q, [float(c) for c in V]) / VV * float(nrows - 1)
    z3 = z * z * z
    f = K * torch.sqrt(dot(e, e)) / z3
    valid = (z > 0) & (a >= 0) & (a < float(ncols)) & (b >= 0) & (b < float(nrows)) & (z3 < float("inf")) & (f >= 0) & (f < float("inf"))
    pixel = torch.where(valid, torch.floor(b).to(torch.int32) * ncols + torch.floor(a).to(torch.int32), torch.full_like(a, -1, dtype=torch.int32))
    rays = torch.empty((pts.shape[0], 7), dtype=torch.float64, device=pts.device)
    for k in range(3):
        rays[:, k], rays[:, 3 + k] = y[k], x[k] - y[k]
    rays[:, 6] = pts[:, 3]
    rays = torch.where(valid[:, None], rays, torch.zeros_like(rays))
    return pixel, torch.where(valid, f, torch.zeros_like(f)), rays, st2


def torch_emit(torch, tab, st, lo, hi):
    """include/tor_camera.h's emission in torch on the table's records: (light, pdf (m, 2), rays, normal, states)."""
    centre, radius, weight, runs, objects = tab
    (ut, u0, u1, u2, u3, u4), st2 = torch_draws(torch, st, 6)
    time = ut * (hi - lo) + lo
    time = torch.where(time <= lo, torch.full_like(time, lo), time)
    T = runs[-1]
    j = torch.searchsorted(runs, u0 * T, right=True).clamp(max=runs.numel() - 1)
    R = radius[j]
    zc = 1.0 - 2.0 * u1
    rr = torch.sqrt(4.0 * u1 * (1.0 - u1))
    a2 = u2 * TWO_PI
    n = [rr * torch.cos(a2), rr * torch.sin(a2), zc]
    sin_t, cos_t = torch.sqrt(u3), torch.sqrt(1.0 - u3)
    a4 = u4 * TWO_PI
    sg = torch.copysign(torch.ones_like(zc), zc)
    aa = -1.0 / (sg + n[2])
    bb = n[0] * n[1] * aa
    b1 = (1.0 + sg * n[0] * n[0] * aa, sg * bb, (-sg) * n[0])
    b2 = (bb, sg + n[1] * n[1] * aa, -n[1])
    e1, e2 = sin_t * torch.cos(a4), sin_t * torch.sin(a4)
    rays = torch.empty((st.shape[0], 7), dtype=torch.float64, device=st.device)
    c = centre[j]
    for k in range(3):
        rays[:, k] = c[:, k] + n[k] * R
        rays[:, 3 + k] = b1[k] * e1 + b2[k] * e2 + n[k] * cos_t
    rays[:, 6] = time
    pdf = torch.stack(((weight[j] / T) / ((4.0 * PI) * (R * R)), cos_t / PI), dim=1)
    return objects[j], pdf, rays, torch.stack(n, dim=1), st2


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


def connect_row(a, name):
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    if not torch.cuda.is_available():
        sys.exit("light_trace_rate: no GPU -- a rate is measured on the device or not at all")
    cam = tor.camera(look_from=(13, 2, 3), look_at=(0, 0, 0), vertical_field_of_view=20.0, aspect_ratio=16.0 / 9.0,
                     aperture=2.0 * CAMERAS[name], focus_distance=10.0)
    cam24 = cam.as_array()
    m = a.points
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019)
    pts = torch.rand((m, 4), dtype=torch.float64, device="cuda", generator=gen)
    pts[:, 0:3] = (pts[:, 0:3] - 0.5) * 8.0                               # a cube about the look-at point: most of it in the frame
    st0 = torch.randint(-(1 << 62), 1 << 62, (m, 4), dtype=torch.int64, device="cuda", generator=gen) * 2 + 1
    ctx = tor.Context()
    st = st0.clone()
    got = ctx.connect_camera(cam, NROWS, NCOLS, pts, st)
    pixel, f, rays, st2 = torch_connect(torch, cam24, NROWS, NCOLS, pts, st0)
    torch.cuda.synchronize()
    both = (pixel >= 0) & (got.pixel >= 0)
    check = {"states_equal": bool(torch.equal(st2, st)), "connected": int((got.pixel >= 0).sum()), "pixels_differ": int((pixel != got.pixel).sum()),
             "factor_rel": float(((f - got.factor).abs() / got.factor.abs().clamp(min=1e-300))[both].max()),
             "rays_abs": float((rays - got.rays)[both].abs().max())}
    st = st0.clone()
    out = ctx.connect_camera(cam, NROWS, NCOLS, pts, st)
    legs = {"library": lambda: ctx.connect_camera(cam, NROWS, NCOLS, pts, st, out=out),
            "torch": lambda: torch_connect(torch, cam24, NROWS, NCOLS, pts, st0)}
    med, rate = measure(torch, a, legs, m)
    ctx.close()
    print("ROW " + json.dumps({"entry": "connect", "case": name, "points": m, "ms": {k: round(v, 4) for k, v in med.items()},
                               "mpoints_s": {k: round(v, 2) for k, v in rate.items()},
                               "gb_s": round(rate["library"] * 1e6 * CONNECT_BYTES / 1e9, 1),
                               "library_vs_torch": round(rate["library"] / rate["torch"], 1), "check": check,
                               "device": torch.cuda.get_device_name(0)}))
    return 0


def emit_row(a, n_lights):
    import torch
    tor = importlib.import_module("trace-of-radiance_amd")
    if not torch.cuda.is_available():
        sys.exit("light_trace_rate: no GPU -- a rate is measured on the device or not at all")
    rs = np.random.RandomState(n_lights)
    recs = np.zeros((n_lights + 1, 16))
    recs[:, 1:4] = rs.uniform(-20.0, 20.0, size=(n_lights + 1, 3))
    recs[:, 4:7] = recs[:, 1:4]
    recs[:, 8] = 1.0
    recs[:, 9] = rs.uniform(0.05, 0.5, size=n_lights + 1)
    recs[:, 11:14] = 0.5
    recs[0, 1:4], recs[0, 4:7], recs[0, 9] = (0.0, -1000.0, 0.0), (0.0, -1000.0, 0.0), 970.0
    lights = np.arange(1, n_lights + 1, dtype=np.int32)
    weights = rs.uniform(0.1, 3.0, size=n_lights)
    runs = np.add.accumulate(weights)                                     # (ufunc.accumulate adds in order)
    ctx = tor.Context()
    ctx.upload(tor.Scene.from_records(recs).list())
    ctx.set_lights(lights, weights)
    m = a.points
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019 + n_lights)
    st0 = torch.randint(-(1 << 62), 1 << 62, (m, 4), dtype=torch.int64, device="cuda", generator=gen) * 2 + 1
    tab = tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (recs[lights, 1:4], np.abs(recs[lights, 9]), weights, runs,
                                                                            lights))
    st = st0.clone()
    got = ctx.emit_lights(st, (0.0, 1.0))
    light, pdf, rays, nrm, st2 = torch_emit(torch, tab, st0, 0.0, 1.0)
    torch.cuda.synchronize()
    check = {"states_equal": bool(torch.equal(st2, st)), "lights_differ": int((light != got.light).sum()),
             "lights_picked": int(torch.unique(got.light).numel()),
             "pdf_area_differ": int((pdf[:, 0].contiguous().view(torch.int64) != got.pdf_area.contiguous().view(torch.int64)).sum()),
             "rays_abs": float((rays - got.rays).abs().max()), "normal_abs": float((nrm - got.normal).abs().max())}
    st = st0.clone()
    out = ctx.emit_lights(st, (0.0, 1.0))
    legs = {"library": lambda: ctx.emit_lights(st, (0.0, 1.0), out=out), "torch": lambda: torch_emit(torch, tab, st0, 0.0, 1.0)}
    med, rate = measure(torch, a, legs, m)
    ctx.close()
    print("ROW " + json.dumps({"entry": "emit", "case": f"{n_lights} lights", "points": m, "ms": {k: round(v, 4) for k, v in med.items()},
                               "mpoints_s": {k: round(v, 2) for k, v in rate.items()},
                               "gb_s": round(rate["library"] * 1e6 * EMIT_BYTES / 1e9, 1),
                               "library_vs_torch": round(rate["library"] / rate["torch"], 1), "check": check,
                               "device": torch.cuda.get_device_name(0)}))
    return 0


def variances():
    """The child of the variance record: the caustic frame of tests/camera_inputs.py, trace_direct against trace_light."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import camera_inputs as I
    tor = importlib.import_module("trace-of-radiance_amd")
    side, spp, depth, batches = 8, 128, 8, 16
    recs, emission, lamp = I.caustic_scene()
    scene = tor.Scene.from_records(recs)
    ctx = tor.Context()
    ctx.upload(scene.list())
    ctx.set_lights([lamp])
    cam = I.frame_camera(tor)
    rays, rng = ctx.camera_rays(cam, side, side, 0, spp)
    diffuse = tor.diffuse_objects(scene)
    lum = ctx.trace_direct(rays, rng.clone(), emission, diffuse, depth)[0].mean(dim=1).reshape(side * side, spp).cpu().numpy()
    var = lum.var(axis=1, ddof=1)
    rows = [{"estimator": "trace_direct", "frame_mean": float(lum.mean()), "standard_error": float(np.sqrt((var / spp).sum()) / (side * side)),
             "mean_pixel_variance": float(var.mean()), "max_pixel_variance": float(var.max())}]
    per = side * side * spp // batches                                    # paths per batch: spp / batches samples per pixel each
    est = []
    for b in range(batches):
        st = torch.from_numpy(tor.rng_seed2(np.full(per, b, dtype=np.uint64), np.arange(per, dtype=np.uint64)).view(np.int64)).cuda()
        acc = torch.zeros(side * side, dtype=torch.float64, device="cuda")

        def splat(pixels, colors, index):
            at = index.long()
            keep = pixels[at] >= 0
            acc.index_add_(0, pixels[at][keep].long(), colors[at][keep].mean(dim=1))
        ctx.trace_light(cam, side, side, st, emission, diffuse, depth, splat=splat)
        est.append((acc * (side * side) / per).cpu().numpy())            # the batch's estimate of every pixel
    est = np.array(est)
    k = spp // batches                                                    # a batch is k samples per pixel: per-sample variance = k * the batches'
    var = est.var(axis=0, ddof=1) * k
    rows.append({"estimator": "trace_light", "frame_mean": float(est.mean()),
                 "standard_error": float(est.mean(axis=1).std(ddof=1) / np.sqrt(batches)),
                 "mean_pixel_variance": float(var.mean()), "max_pixel_variance": float(var.max())})
    ctx.close()
    print("ROW " + json.dumps(rows))
    return 0


def child(args, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"light_trace_rate: {what} ran past {limit} s -- stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"light_trace_rate: {what} failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_trace_rate.txt"))
    a = ap.parse_args()
    if a.row == "variances":
        return variances()
    if a.row.startswith("connect:"):
        return connect_row(a, a.row.split(":")[1])
    if a.row.startswith("emit:"):
        return emit_row(a, int(a.row.split(":")[1]))
    common = ["--points", str(a.points), "--reps", str(a.reps), "--rounds", str(a.rounds), "--warm", str(a.warm)]
    rows = []
    for row in [f"connect:{c}" for c in CAMERAS] + [f"emit:{n}" for n in LIGHTS]:   # each GPU step under its own limit; stop at the first that fails
        rc, got = child(["--row", row] + common, a.step_timeout, row)
        if rc:
            return rc
        rows.append(got)
    rc, var = child(["--row", "variances"], a.step_timeout, "the variance record")
    if rc:
        return rc
    lines = [f"light_trace_rate: M points/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events; "
             f"{rows[0]['device']}",
             f"accounting: a connected point moves {CONNECT_BYTES} bytes (32 point + 32 state in; 32 state + 56 ray + 4 pixel + 8 factor out), an "
             f"emitted path {EMIT_BYTES} (32 state in; 32 state + 56 ray + 24 normal + 4 light + 16 densities out) besides the table reads; "
             f"GB/s = library rate x these",
             f"{'entry':<9}{'case':<13}{'points':>9}{'library':>11}{'GB/s':>9}{'torch':>11}{'lib/torch':>11}  agreement with the torch leg"]
    for r in rows:
        g, c = r["mpoints_s"], r["check"]
        lines.append(f"{r['entry']:<9}{r['case']:<13}{r['points']:>9}{g['library']:>11.1f}{r['gb_s']:>9.1f}{g['torch']:>11.2f}"
                     f"{r['library_vs_torch']:>11.1f}  " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in c.items()))
    slower = [f"{r['entry']} {r['case']}" for r in rows if r["library_vs_torch"] < 1.0]
    lines.append("rows slower than the torch leg: " + (", ".join(slower) if slower else "none"))
    lines += ["", "per-pixel variance of trace_direct against trace_light on the caustic frame of tests/camera_inputs.py (8 x 8 pixels, 128 samples "
              "per pixel or as many light paths, depth 8; trace_light's per-sample variance from 16 batches): recorded, not asserted",
              f"{'estimator':<14}{'frame mean':>12}{'std error':>12}{'mean pixel variance':>22}{'max pixel variance':>21}"]
    for v in var:
        lines.append(f"{v['estimator']:<14}{v['frame_mean']:>12.5f}{v['standard_error']:>12.5f}{v['mean_pixel_variance']:>22.5g}"
                     f"{v['max_pixel_variance']:>21.5g}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "light_trace_rate", "unit": "M points/s", "rows": rows, "variances": var}))
    return 0 if all(r["check"]["states_equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
