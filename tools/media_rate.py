#!/usr/bin/env python3
"""Rates of the optical-depth march (tor_media_march_device) against what a host does without it -- crossings(k=16, mask=the
boundaries' group) and a walk of the sorted events in torch -- on the same device arrays in one process: M rays/s per (number of
media, ray set).  random_scene (485 objects) with 1, 8 and 64 boundary spheres added in a group of their own; ray sets camera and
incoherent (tools/occluded_rate.py's); tau = -log1p(-u) of seeded uniforms.

The composition can answer only a ray all of whose boundary events fit the 16 entries, that is a ray that crosses at most 8
boundaries: the legs that are compared run on those rays (compacted copies); the march is also timed on every ray.  A count of 16
does not say whether more events follow, so the rays that have exactly 16 are told from the longer ones by a second query, k = 1
with t_min moved to the 16th event: no further crossing, and the ray is compared.  Legs, interleaved per round between HIP events:
    compose    one tor_crossings_device launch (k = 16, masked) -- of the library --parent-lib names (the parent commit's build,
               loaded next to this one with a context of its own on the same scene and groups), else of this build -- and the torch
               walk: densities at the events, the running depth, the first segment in which it passes tau, the collision there
    march_a    one tor_media_march_device launch into outputs allocated before the timing
    march_b    march_a again: the run-to-run spread
    march_all  the march on every ray of the set
Every leg: WARM warm-up runs, then ROUNDS timings of REPS back-to-back runs; the median over the rounds.  No ratio is fixed in
advance: a win is claimed only where march / compose lies above 1 by more than the spread of the two march legs, a loss is said
plainly.  The step count of a march is its events + 1, so the mean events per ray (capped at 16 by the query that counts them) are
reported next to each row, with the share of rays beyond it (more than 16 events: not compared).  The two answers must agree: status on every compared ray, t within
1e-9 relative (the composition's sums are not the march's bits).  Each table (1, 8, 64 media) runs in a child process under --step-timeout; the
first that fails or runs past it ends the run.  Writes the table to --out and prints one JSON line.

    python tools/media_rate.py [--parent-lib /path/to/parent/libtor_mi355x.so] [--reps 2] [--rounds 5] [--warm 1]
                               [--step-timeout 240] [--out profiles/media_rate.txt]
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

import occluded_rate as W  # noqa: E402  (the workloads)

tor = importlib.import_module("trace-of-radiance_amd")
K = tor.CROSSINGS_MAX
MEDIA = (1, 8, 64)
SURFACES, BOUNDARIES = 1, 2   # the two visibility groups


class ParentCrossings:
    """tor_crossings_device of another build of the library (the parent commit's), on a context of its own with the same scene and
    groups."""

    def __init__(self, path, scene, groups):
        self.L = C.CDLL(os.path.abspath(path))
        self.L.tor_last_error.restype = C.c_char_p
        self.L.tor_context_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
        self.L.tor_context_destroy.argtypes = [C.c_void_p]
        self.L.tor_scene_upload.argtypes = [C.c_void_p, tor.HittableList]
        tor._bind(self.L, ("tor_crossings_device", "tor_scene_groups"))
        self.h = C.c_void_p()
        self._ok(self.L.tor_context_create(-1, C.byref(self.h)))
        self._ok(self.L.tor_scene_upload(self.h, scene.list()))
        g = np.ascontiguousarray(groups, dtype=np.uint32)
        self._ok(self.L.tor_scene_groups(self.h, int(g.size), C.c_void_p(g.ctypes.data)))

    def _ok(self, rc):
        if rc != 0:
            raise SystemExit("media_rate: parent library: " + self.L.tor_last_error().decode("utf-8", "replace"))

    def crossings(self, rays, t_range, tr, raw, count):
        stream = torch.cuda.current_stream().cuda_stream
        self._ok(self.L.tor_crossings_device(self.h, int(rays.shape[0]), C.c_void_p(rays.data_ptr()), C.c_void_p(t_range.data_ptr()),
                                             C.c_void_p(0), int(rays.shape[0]), K, C.c_void_p(0), BOUNDARIES, tr[0], tr[1], tor.HIT_AUTO,
                                             C.c_void_p(raw.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(0), C.c_void_p(stream)))

    def close(self):
        self.L.tor_context_destroy(self.h)


def fog_scene(n_media, seed=20261020):
    """random_scene's records with n_media boundary spheres appended (centres over the scene's floor, radii 1.5 .. 3: they overlap),
    the media's objects, sigma and the group words."""
    base = tor.random_scene(0xFACADE).to_records()
    g = np.random.default_rng(seed)
    extra = np.zeros((n_media, 16))
    c = np.stack([g.uniform(-9, 9, n_media), g.uniform(0.5, 1.5, n_media), g.uniform(-9, 9, n_media)], axis=1)
    c[0] = (0.0, 1.0, 0.0)                                     # the first one where the camera looks, so that the 1-medium rows see it
    extra[:, 1:4], extra[:, 4:7], extra[:, 8] = c, c, 1.0
    extra[:, 9] = g.uniform(1.5, 3.0, n_media)
    extra[0, 9] = 3.0
    extra[:, 11:14] = 0.5
    recs = np.concatenate([base, extra])
    objects = np.arange(len(base), len(recs), dtype=np.int32)
    groups = np.where(np.arange(len(recs)) < len(base), SURFACES, BOUNDARIES).astype(np.uint32)
    return recs, objects, g.uniform(0.05, 0.5, n_media), groups


def walk(raw, count, sigma_of, tau, length):
    """The host's walk of the sorted events of crossings(k=16): (status, t, depth) per ray.  Event j is (t_j, object, which); the
    density after it is the density before plus or minus the object's sigma; a ray that starts inside a boundary sees its exit
    without its entry, which is how the density before the first event is found."""
    n = raw.shape[0]
    words = raw.view(torch.int32)
    t, obj, which = raw[:, :, 0], words[:, :, 2], words[:, :, 3]
    valid = torch.arange(K, device=raw.device)[None, :] < count[:, None]
    sig = torch.where(valid, sigma_of[obj.clamp(min=0).long()], torch.zeros((), dtype=torch.float64, device=raw.device))
    enter = which == 0
    rho0 = (sig * ~enter).sum(dim=1) - (sig * enter).sum(dim=1)
    after = rho0[:, None] + torch.cumsum(torch.where(enter, sig, -sig), dim=1)
    before = torch.cat([rho0[:, None], after[:, :-1]], dim=1).clamp(min=0.0)
    start = torch.cat([torch.zeros((n, 1), dtype=torch.float64, device=raw.device), t[:, :-1]], dim=1)
    steps = torch.where(valid, before * ((t - start) * length[:, None]), torch.zeros((), dtype=torch.float64, device=raw.device))
    depth = torch.cumsum(steps, dim=1)
    passed = valid & (depth > tau[:, None])
    first = torch.argmax(passed.int(), dim=1, keepdim=True)
    hit = passed.any(dim=1)
    d_before = torch.gather(depth - steps, 1, first)[:, 0]
    t_c = torch.gather(start, 1, first)[:, 0] + ((tau - d_before) / torch.gather(before, 1, first)[:, 0]) / length
    total = depth[:, -1]
    status = hit.int()
    return status, torch.where(hit, t_c, torch.full_like(t_c, float("inf"))), torch.where(hit, tau, total)


def rate_rows(a, n_media):
    """The rows of one table size: runs in a child process (main's --row) and prints them as one ROW line."""
    if not torch.cuda.is_available():
        sys.exit("media_rate: no GPU -- a rate is measured on the device or not at all")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261020 + n_media)
    cam = tor.camera()
    legs_order = ["compose", "march_a", "march_b", "march_all"]
    rows = []
    recs, objects, sigma, groups = fog_scene(n_media)
    scene = tor.Scene.from_records(recs)
    ctx = tor.Context()
    ctx.upload(scene.list())
    ctx.set_groups(groups)
    ctx.set_media(objects, sigma)
    parent = ParentCrossings(a.parent_lib, scene, groups) if a.parent_lib else None
    sigma_of = torch.zeros(len(recs), dtype=torch.float64, device="cuda")
    sigma_of[torch.from_numpy(objects).long().cuda()] = torch.from_numpy(sigma).cuda()
    for rname, all_rays, _ in W.ray_sets(ctx, cam, recs, a.rays, gen)[:2]:
        n_all = int(all_rays.shape[0])
        tr = tuple(float(v) for v in torch.aminmax(all_rays[:, 6]))
        tau_all = -torch.log1p(-torch.rand(n_all, dtype=torch.float64, device="cuda", generator=gen))
        counted = ctx.crossings(all_rays, K, torch.tensor([0.0, float("inf")], dtype=torch.float64, device="cuda").repeat(n_all, 1),
                                None, tr, "auto", mask=BOUNDARIES)
        torch.cuda.synchronize()
        events_all = float(counted.count.double().mean())
        # exactly 16 events, or more?  one more crossing past the 16th decides
        past = torch.empty((n_all, 2), dtype=torch.float64, device="cuda")
        past[:, :] = float("inf")
        past[:, 0] = torch.where(counted.count == K, counted.t[:, K - 1], past[:, 0])
        more = ctx.crossings(all_rays, 1, past, None, tr, "auto", mask=BOUNDARIES)
        torch.cuda.synchronize()
        keep = (counted.count < K) | ((counted.count == K) & (more.count == 0))
        capped = float((~keep).double().mean())
        rays, tau = all_rays[keep].contiguous(), tau_all[keep].contiguous()
        n = int(rays.shape[0])
        events = float(counted.count[keep].double().mean())
        t_range = torch.tensor([0.0, float("inf")], dtype=torch.float64, device="cuda").repeat(n, 1)
        length = torch.sqrt((rays[:, 3:6] * rays[:, 3:6]).sum(dim=1))
        raw = torch.zeros((n, K, 2), dtype=torch.float64, device="cuda")
        count = torch.zeros((n,), dtype=torch.int32, device="cuda")
        cr = ctx.crossings(rays, K, t_range, None, tr, "auto", mask=BOUNDARIES)

        def compose():
            if parent is not None:
                parent.crossings(rays, t_range, tr, raw, count)
                return walk(raw, count, sigma_of, tau, length)
            c = ctx.crossings(rays, K, t_range, None, tr, "auto", mask=BOUNDARIES, out=cr)
            return walk(c.raw, c.count, sigma_of, tau, length)

        out = ctx.march_media(rays, tau)
        out_all = ctx.march_media(all_rays, tau_all)
        legs = {"compose": compose, "march_a": lambda: ctx.march_media(rays, tau, out=out),
                "march_b": lambda: ctx.march_media(rays, tau, out=out), "march_all": lambda: ctx.march_media(all_rays, tau_all, out=out_all)}
        for leg in legs_order:
            for _ in range(a.warm):
                legs[leg]()
        status, t_c, depth = compose()
        m = ctx.march_media(rays, tau)
        torch.cuda.synchronize()
        agree = float((status == m.status).double().mean())
        both = (status == 1) & (m.status == 1)
        t_err = float(((t_c[both] - m.t[both]).abs() / m.t[both].abs().clamp(min=1e-300)).max()) if bool(both.any()) else 0.0
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
        size = {"compose": n, "march_a": n, "march_b": n, "march_all": n_all}
        rate = {leg: size[leg] / (statistics.median(ms[leg]) * 1e-3) / 1e6 for leg in legs_order}
        spread = abs(rate["march_a"] - rate["march_b"]) / max(rate["march_a"], rate["march_b"])
        ratio = min(rate["march_a"], rate["march_b"]) / rate["compose"]
        verdict = "win" if ratio > 1.0 + spread else ("LOSS" if ratio < 1.0 - spread else "within the spread")
        rows.append({"device": torch.cuda.get_device_name(0), "media": n_media, "rays": rname, "n_all": n_all, "n_compared": n,
                     "beyond_share": round(capped, 4), "events_per_ray_all": round(events_all, 3), "events_per_ray_compared": round(events, 3),
                     "collided_share": round(float((m.status == 1).double().mean()), 4),
                     "mrays_s": {k: round(v, 1) for k, v in rate.items()}, "march_spread": round(spread, 4),
                     "march_vs_compose": round(ratio, 2), "verdict": verdict, "status_agree": round(agree, 6), "t_rel_err": t_err})
    if parent is not None:
        parent.close()
    ctx.close()
    print("ROW " + json.dumps(rows))
    return 0


def child(args, limit, what):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"media_rate: {what} ran past {limit} s -- stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"media_rate: {what} failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    return 0, json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="libtor_mi355x.so built from the parent commit: the compose leg's crossings run on it")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds the rows of one table size may take")
    ap.add_argument("--row", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "media_rate.txt"))
    a = ap.parse_args()
    if a.row:
        return rate_rows(a, a.row)
    common = ["--rays", str(a.rays), "--reps", str(a.reps), "--rounds", str(a.rounds), "--warm", str(a.warm)]
    if a.parent_lib:
        common += ["--parent-lib", a.parent_lib]
    rows = []
    for n_media in MEDIA:   # each GPU step under its own limit; stop at the first that fails
        rc, got = child(["--row", str(n_media)] + common, a.step_timeout, f"the table of {n_media} media")
        if rc:
            return rc
        rows += got
    lines = [f"media_rate: M rays/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events; "
             f"{rows[0]['device']}; the compose leg's crossings: {'the parent build ' + a.parent_lib if a.parent_lib else 'this build'}",
             f"{'media':>5} {'rays':<11}{'compared':>9}{'beyond':>8}{'events':>8}{'ev(all)':>8}{'collide':>8}{'compose':>9}{'march':>9}"
             f"{'again':>9}{'spread':>8}{'m/c':>7}{'march(all)':>11}  verdict            status=  t rel err"]
    for r in rows:
        g = r["mrays_s"]
        lines.append(f"{r['media']:>5} {r['rays']:<11}{r['n_compared']:>9}{r['beyond_share']:>8.3f}{r['events_per_ray_compared']:>8.2f}"
                     f"{r['events_per_ray_all']:>8.2f}{r['collided_share']:>8.3f}{g['compose']:>9.1f}{g['march_a']:>9.1f}{g['march_b']:>9.1f}"
                     f"{r['march_spread']:>8.3f}{r['march_vs_compose']:>7.2f}{g['march_all']:>11.1f}  {r['verdict']:<18} {r['status_agree']:.6f}"
                     f"  {r['t_rel_err']:.2e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "media_rate", "unit": "M rays/s", "reps": a.reps, "rounds": a.rounds, "warm": a.warm,
                      "parent_lib": a.parent_lib, "rows": rows}))
    return 0 if all(r["status_agree"] > 0.9999 for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
