#!/usr/bin/env python3
"""Rates of the density-grid march (tor_media_grid_march_device, include/tor_grid.h) against two yardsticks on the same device arrays
in one process: M rays/s per (grid, ray set), with the steps per ray.  random_scene plus one boundary sphere of radius 3 where the
camera looks (tools/media_rate.py's fog_scene(1)); the grid on the sphere's bounding cube, 16^3, 64^3 (2 MB) and 256^3 (128 MB) cells
of seeded uniform density, a fifth of them 0; ray sets camera (coherent) and incoherent (tools/occluded_rate.py's);
tau = -log1p(-u) of seeded uniforms; range (0, inf).  Legs, interleaved per round between HIP events:
    compose    what a host does without the entry: the same DDA written in torch.  Sphere, clip and entry cell in elementwise
               passes on every ray, one compaction to the rays that enter the grid, then ONE elementwise pass over those rays per
               DDA step (about 60 torch launches), done lanes masked, leaving when every ray is done (one host read per step).  It
               does not compact again as rays finish.
    grid_a     one tor_media_grid_march_device launch into outputs allocated before the timing
    grid_b     grid_a again: the run-to-run spread
    floor      tor_media_march_device of this build on ONE homogeneous medium (the same sphere without a grid, a context of its
               own) over the same rays and budgets: a march that takes at most two steps and loads no density
    floor_p    with --parent-lib: the same on the library of the parent commit (a context of its own), else absent
Every leg: WARM warm-up runs, then ROUNDS timings of REPS back-to-back runs; the median over the rounds.  No ratio is fixed in
advance: a win is claimed only where the slower grid leg beats compose by more than the spread of the two grid legs AND the spread
of compose's own rounds; a loss is said plainly.  The two answers must agree: status on every ray, t and depth within 1e-12
relative.  Steps per ray are the walk's iterations, counted by the composition: over the rays that enter the grid, and over all.
Each grid runs in a child process under --step-timeout; the first that fails or runs past it ends the run.  Writes the table to
--out and prints one JSON line.

    python tools/grid_rate.py [--parent-lib /path/to/parent/libtor_mi355x.so] [--reps 1] [--rounds 5] [--warm 1]
                              [--step-timeout 280] [--out profiles/grid_rate.txt]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import media_rate as M  # noqa: E402  (the scene)
import occluded_rate as W  # noqa: E402  (the ray sets)

tor = importlib.import_module("trace-of-radiance_amd")
GRIDS = (16, 64, 256)
SIGMA = 0.5
INF = float("inf")


class ParentMarch:
    """tor_media_march_device of another build of the library (the parent commit's), on a context of its own with the same scene
    and the one homogeneous medium."""

    def __init__(self, path, scene, objects, sigma):
        self.L = C.CDLL(os.path.abspath(path))
        self.L.tor_last_error.restype = C.c_char_p
        self.L.tor_context_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
        self.L.tor_context_destroy.argtypes = [C.c_void_p]
        self.L.tor_scene_upload.argtypes = [C.c_void_p, tor.HittableList]
        tor._bind(self.L, ("tor_scene_media", "tor_media_march_device"))
        self.h = C.c_void_p()
        self._ok(self.L.tor_context_create(-1, C.byref(self.h)))
        self._ok(self.L.tor_scene_upload(self.h, scene.list()))
        o, s = np.ascontiguousarray(objects, dtype=np.int32), np.ascontiguousarray(sigma, dtype=np.float64)
        self._ok(self.L.tor_scene_media(self.h, int(o.size), C.c_void_p(o.ctypes.data), C.c_void_p(s.ctypes.data), C.c_void_p(0)))

    def _ok(self, rc):
        if rc != 0:
            raise SystemExit("grid_rate: parent library: " + self.L.tor_last_error().decode("utf-8", "replace"))

    def march(self, rays, tau, out):
        n = int(rays.shape[0])
        p = lambda x: C.c_void_p(x.data_ptr())
        self._ok(self.L.tor_media_march_device(self.h, n, p(rays), C.c_void_p(0), p(tau), C.c_void_p(0), n, p(out.status), p(out.t),
                                               p(out.depth), p(out.active), p(out.rho),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def close(self):
        self.L.tor_context_destroy(self.h)


def torch_dda(rays, tau, centre, radius, lo, hi, h, dims, dens):
    """The march of include/tor_grid.h in torch, float64, the header's operations in the header's order (range (0, inf), a boundary
    that does not move): (status int32, t, depth, steps int32) per ray."""
    n = rays.shape[0]
    dev = rays.device
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    inf = torch.full((), INF, dtype=torch.float64, device=dev)
    d = [rays[:, 3 + k] for k in range(3)]
    oc = [rays[:, k] - centre[k] for k in range(3)]
    a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    ln = torch.sqrt(a)
    half_b = (oc[0] * d[0] + oc[1] * d[1]) + oc[2] * d[2]
    cc = ((oc[0] * oc[0] + oc[1] * oc[1]) + oc[2] * oc[2]) - radius * radius
    disc = half_b * half_b - a * cc
    has = disc > 0
    root = torch.sqrt(torch.where(has, disc, zero))
    s0, s1 = (-half_b - root) / a, (-half_b + root) / a
    refused = ~(tau >= 0)
    ok = has & ~refused
    t0, t1 = torch.where(s0 > 0, s0, zero), s1
    for k in range(3):
        still = d[k] == 0
        ok &= ~still | ((oc[k] >= lo[k]) & (oc[k] < hi[k]))
        ta, tb = (lo[k] - oc[k]) / d[k], (hi[k] - oc[k]) / d[k]
        up = d[k] > 0
        near, far = torch.where(up, ta, tb), torch.where(up, tb, ta)
        t0 = torch.where(~still & (near > t0), near, t0)
        t1 = torch.where(~still & (far < t1), far, t1)
    ok &= t0 < t1
    status = torch.where(refused, -1, 0).to(torch.int32)
    t_out = torch.where(refused, zero, inf).expand(n).clone()
    depth_out = torch.zeros(n, dtype=torch.float64, device=dev)
    steps_out = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = torch.nonzero(ok).reshape(-1)          # the one compaction: the rays that enter the grid
    if rows.numel() == 0:
        return status, t_out, depth_out, steps_out
    d, oc = [x[rows] for x in d], [x[rows] for x in oc]
    ln, t, t1, tau_r = ln[rows], t0[rows], t1[rows], tau[rows]
    m = rows.numel()
    i, dr, up1, tk = [], [], [], []
    for k in range(3):
        f = torch.floor(((oc[k] + t * d[k]) - lo[k]) / h[k])
        f = torch.where(f >= 0, f, zero)
        f = torch.where(f > dims[k] - 1, torch.full_like(f, dims[k] - 1), f)
        i.append(f.long())
        dr.append((d[k] > 0).long() - (d[k] < 0).long())
        up1.append((d[k] > 0).long())
        tk.append(torch.where(dr[k] == 0, inf, ((lo[k] + (i[k] + up1[k]).double() * h[k]) - oc[k]) / d[k]))
    D = torch.zeros(m, dtype=torch.float64, device=dev)
    done = torch.zeros(m, dtype=torch.bool, device=dev)
    st = torch.zeros(m, dtype=torch.int32, device=dev)
    t_c_out = torch.full((m,), INF, dtype=torch.float64, device=dev)
    steps = torch.zeros(m, dtype=torch.int32, device=dev)
    for _ in range(dims[0] + dims[1] + dims[2]):
        steps += (~done).int()
        tn, isy, isz = tk[0], tk[1] < tk[0], None
        tn = torch.where(isy, tk[1], tn)
        isz = tk[2] < tn
        tn = torch.where(isz, tk[2], tn)
        ks = [~isy & ~isz, isy & ~isz, isz]
        last = ~(tn < t1)
        tn = torch.where(last, t1, tn)
        tn = torch.where(tn < t, t, tn)
        rho = SIGMA * dens[(i[0] * dims[1] + i[1]) * dims[2] + i[2]]
        pos = rho > 0
        step = torch.where(pos, rho * ((tn - t) * ln), zero)
        rem = tau_r - D
        coll = ~done & pos & (rem < step)
        t_c = t + (rem / rho) / ln
        t_c = torch.where(tn < t_c, tn, t_c)
        st = torch.where(coll, 1, st).to(torch.int32)
        t_c_out = torch.where(coll, t_c, t_c_out)
        go = ~done & ~coll
        D = torch.where(go, D + step, D)
        done = done | coll | (go & last)
        for k in range(3):
            mv = ~done & ks[k]
            moved = i[k] + dr[k]
            left = mv & ((moved < 0) | (moved >= dims[k]))
            done = done | left
            mv = mv & ~left
            i[k] = torch.where(mv, moved, i[k])
            tk[k] = torch.where(mv, ((lo[k] + (i[k] + up1[k]).double() * h[k]) - oc[k]) / d[k], tk[k])
        t = torch.where(done, t, tn)
        if bool(done.all()):
            break
    status[rows] = st
    t_out[rows] = t_c_out
    depth_out[rows] = torch.where(st == 1, tau_r, D)
    steps_out[rows] = steps
    return status, t_out, depth_out, steps_out


def rate_rows(a, n_grid):
    """The rows of one grid size: runs in a child process (main's --row) and prints them as one ROW line."""
    if not torch.cuda.is_available():
        sys.exit("grid_rate: no GPU -- a rate is measured on the device or not at all")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261021 + n_grid)
    cam = tor.camera()
    recs, objects, _, groups = M.fog_scene(1)
    sigma = np.asarray([SIGMA])
    scene = tor.Scene.from_records(recs)
    g = np.random.default_rng(n_grid)
    dens = g.random((n_grid,) * 3)
    dens[g.random((n_grid,) * 3) < 0.2] = 0.0
    ctx, flat = tor.Context(), tor.Context()
    for c in (ctx, flat):
        c.upload(scene.list())
        c.set_groups(groups)
        c.set_media(objects, sigma)
    ctx.set_media_grid(0, dens)
    dims, box, _ = ctx.media_grid_info(0)
    lo, hi = [float(v) for v in box[:3]], [float(v) for v in box[3:]]
    h = [(hi[k] - lo[k]) / dims[k] for k in range(3)]
    rec = recs[int(objects[0])]
    centre, radius = [float(v) for v in rec[1:4]], float(rec[9])
    d_dens = torch.from_numpy(dens.reshape(-1)).cuda()
    parent = ParentMarch(a.parent_lib, scene, objects, sigma) if a.parent_lib else None
    legs_order = ["compose", "grid_a", "grid_b", "floor"] + (["floor_p"] if parent else [])
    rows = []
    for rname, rays, _ in W.ray_sets(ctx, cam, recs, a.rays, gen)[:2]:
        n = int(rays.shape[0])
        tau = -torch.log1p(-torch.rand(n, dtype=torch.float64, device="cuda", generator=gen))
        out = ctx.march_media_grid(rays, tau, 0)
        out_f = flat.march_media(rays, tau)
        out_p = flat.march_media(rays, tau)
        compose = lambda: torch_dda(rays, tau, centre, radius, lo, hi, h, dims, d_dens)
        legs = {"compose": compose, "grid_a": lambda: ctx.march_media_grid(rays, tau, 0, out=out),
                "grid_b": lambda: ctx.march_media_grid(rays, tau, 0, out=out), "floor": lambda: flat.march_media(rays, tau, out=out_f)}
        if parent:
            legs["floor_p"] = lambda: parent.march(rays, tau, out_p)
        for leg in legs_order:
            for _ in range(a.warm):
                legs[leg]()
        status, t_c, depth, steps = compose()
        got = ctx.march_media_grid(rays, tau, 0)
        torch.cuda.synchronize()
        agree = float((status == got.status).double().mean())
        both = (status == 1) & (got.status == 1)
        rel = lambda x, y: float(((x - y).abs() / y.abs().clamp(min=1e-300)).max()) if x.numel() else 0.0
        t_err = rel(t_c[both], got.t[both])
        same = status == got.status
        d_err = rel(depth[same & (got.depth > 0)], got.depth[same & (got.depth > 0)])
        entered = steps > 0
        ms = {leg: [] for leg in legs_order}
        for _ in range(a.rounds):
            for leg in legs_order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    legs[leg]()
                e1.record()
                torch.cuda.synchronize()
                ms[leg].append(e0.elapsed_time(e1) / a.reps)
        rate = {leg: n / (statistics.median(ms[leg]) * 1e-3) / 1e6 for leg in legs_order}
        spread = abs(rate["grid_a"] - rate["grid_b"]) / max(rate["grid_a"], rate["grid_b"])
        c_spread = (max(ms["compose"]) - min(ms["compose"])) / statistics.median(ms["compose"])
        slow = min(rate["grid_a"], rate["grid_b"])
        ratio = slow / rate["compose"]
        margin = spread + c_spread
        verdict = "win" if ratio > 1.0 + margin else ("LOSS" if ratio < 1.0 - margin else "within the spread")
        rows.append({"device": torch.cuda.get_device_name(0), "grid": n_grid, "rays": rname, "n": n,
                     "entered_share": round(float(entered.double().mean()), 4),
                     "steps_per_entered_ray": round(float(steps[entered].double().mean()) if bool(entered.any()) else 0.0, 2),
                     "steps_per_ray": round(float(steps.double().mean()), 2), "steps_max": int(steps.max()),
                     "collided_share": round(float((got.status == 1).double().mean()), 4),
                     "mrays_s": {k: round(v, 2) for k, v in rate.items()}, "grid_spread": round(spread, 4),
                     "compose_spread": round(c_spread, 4), "grid_vs_compose": round(ratio, 1),
                     "grid_vs_floor": round(slow / rate["floor"], 3), "verdict": verdict, "status_agree": round(agree, 6),
                     "t_rel_err": t_err, "depth_rel_err": d_err})
    if parent is not None:
        parent.close()
    ctx.close()
    flat.close()
    print("ROW " + json.dumps(rows))
    return 0


def child(args, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"grid_rate: {what} ran past {limit} s -- stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"grid_rate: {what} failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--grids", default=",".join(str(v) for v in GRIDS), help="cells per axis, comma separated")
    ap.add_argument("--parent-lib", default=None, help="libtor_mi355x.so built from the parent commit: adds the floor_p leg")
    ap.add_argument("--step-timeout", type=int, default=280, help="seconds the rows of one grid may take")
    ap.add_argument("--row", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_rate.txt"))
    a = ap.parse_args()
    if a.row:
        return rate_rows(a, a.row)
    common = ["--rays", str(a.rays), "--reps", str(a.reps), "--rounds", str(a.rounds), "--warm", str(a.warm)]
    if a.parent_lib:
        common += ["--parent-lib", a.parent_lib]
    rows = []
    for n_grid in [int(v) for v in a.grids.split(",")]:   # each GPU step under its own limit; stop at the first that fails
        rc, got = child(["--row", str(n_grid)] + common, a.step_timeout, f"the {n_grid}^3 grid")
        if rc:
            return rc
        rows += got
    lines = [f"grid_rate: M rays/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events, legs "
             f"interleaved; {rows[0]['device']}; {a.rays} rays; floor_p: "
             f"{'the parent build ' + a.parent_lib if a.parent_lib else 'not run'}",
             f"{'grid':>6} {'rays':<11}{'entered':>8}{'steps/e':>9}{'steps':>8}{'max':>5}{'collide':>8}{'compose':>9}{'grid':>9}"
             f"{'again':>9}{'spread':>8}{'c.sprd':>8}{'g/c':>8}{'floor':>9}{'floor_p':>9}{'g/floor':>8}  verdict            status=  "
             f"t rel err  depth rel err"]
    for r in rows:
        g = r["mrays_s"]
        lines.append(f"{str(r['grid']) + '^3':>6} {r['rays']:<11}{r['entered_share']:>8.3f}{r['steps_per_entered_ray']:>9.2f}"
                     f"{r['steps_per_ray']:>8.2f}{r['steps_max']:>5}{r['collided_share']:>8.3f}{g['compose']:>9.2f}{g['grid_a']:>9.1f}"
                     f"{g['grid_b']:>9.1f}{r['grid_spread']:>8.3f}{r['compose_spread']:>8.3f}{r['grid_vs_compose']:>8.1f}"
                     f"{g['floor']:>9.1f}{g.get('floor_p', float('nan')):>9.1f}{r['grid_vs_floor']:>8.3f}  {r['verdict']:<18} "
                     f"{r['status_agree']:.6f}  {r['t_rel_err']:.2e}   {r['depth_rel_err']:.2e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "grid_rate", "unit": "M rays/s", "reps": a.reps, "rounds": a.rounds, "warm": a.warm,
                      "parent_lib": a.parent_lib, "rows": rows}))
    return 0 if all(r["status_agree"] == 1.0 and r["t_rel_err"] <= 1e-12 and r["depth_rel_err"] <= 1e-12 for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
