#!/usr/bin/env python3
"""Rates of the masked queries (tor_hit_masked_device, tor_occluded_masked_device, tor_bounce_masked_device) on the three workloads of
tools/bounce_rate.py, in auto mode, G rays/s:
    camera      the camera rays of random_scene at 1920x1080, samples [0, 16)
    incoherent  16 M rays with seeded origins in random_scene's box, uniform directions and seed1 states
    anim120     frame 120 of the animation (1601 spheres, the two-level culling layout): its camera rays at 1920x1080, one sample
For each entry (hit, occluded, bounce) four columns on the same rays:
    unmasked    the unmasked entry -- of ANOTHER build when --parent-lib names one (the parent commit's library, in a child process
                with the same seeds), else of this build
    all         the masked entry with every object visible (groups by material, mask 0xFFFFFFFF): what the group words cost
    no glass    groups by material, mask without the Dielectric bit: the shadow-ray case
    1 in 4      groups 1 << (j % 4), mask 1: where the box skip should show
The step overwrites its rays and states, so they are restored (untimed) before every launch; each launch sits between two events of
its own.  Warm-up first, REPS launches per round, ROUNDS rounds with the candidates interleaved; the best round counts, the worst is
printed next to it (the spread).  Prints a table and one JSON line.

    python tools/masked_rate.py [--parent-lib /path/to/parent/libtor_mi355x.so] [--reps 3] [--rounds 3] [--samples 16] [--out FILE.txt]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")
H, W = 1080, 1920
ENTRIES = ("hit", "occluded", "bounce")
ALL = 0xFFFFFFFF


def incoherent(recs, n, gen):
    r = torch.tensor(recs[:, 9:10], device="cuda").abs()
    c0, c1 = torch.tensor(recs[:, 1:4], device="cuda"), torch.tensor(recs[:, 4:7], device="cuda")
    lo = torch.quantile(torch.minimum(c0, c1) - r, 0.02, dim=0)
    hi = torch.quantile(torch.maximum(c0, c1) + r, 0.98, dim=0)
    rays = torch.empty((n, 7), dtype=torch.float64, device="cuda")
    rays[:, 0:3] = lo + (hi - lo) * torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    d = torch.randn((n, 3), dtype=torch.float64, device="cuda", generator=gen)
    rays[:, 3:6] = d / d.norm(dim=1, keepdim=True)
    rays[:, 6] = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    st = torch.from_numpy(tor.rng_seed1(np.arange(n, dtype=np.uint64)).view(np.int64)).cuda()
    return rays, st


def timed_each(prepare, fn, reps):
    total = 0.0
    for _ in range(reps):
        prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1) * 1e-3
    return total / reps


def workloads(a):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261016)
    rscene, rcam = tor.random_scene(0xFACADE), tor.camera()
    it = iter(tor.Animation(H, W, 0.005, 0.0, 7.2).scenes(6))
    for _ in range(121):
        acam, ascene, _t = next(it)
    for name, scene, cam, ns in (("camera", rscene, rcam, a.samples), ("incoherent", rscene, None, 0), ("anim120", ascene, acam, 1)):
        ctx = tor.Context()
        ctx.upload(scene.list())
        rays, st0 = ctx.camera_rays(cam, H, W, 0, ns, tor.SEED_SAMPLE) if cam is not None else incoherent(scene.to_records(), a.incoherent, gen)
        yield name, scene, ctx, rays, st0
        ctx.close()
        torch.cuda.empty_cache()


def measure(a, masked):
    """{workload: {entry: {column: [worst, best] G rays/s}}}; masked = False: the unmasked column alone (any build of the library)."""
    out = {}
    for name, scene, ctx, rays, st0 in workloads(a):
        n = rays.shape[0]
        tr = (float(rays[:, 6].min()), float(rays[:, 6].max()))
        work, st = rays.clone(), st0.clone()
        occ = torch.zeros((n,), dtype=torch.int32, device="cuda")
        res = ctx.bounce(work, st, None, tr, "auto")

        def restore():
            work.copy_(rays)
            st.copy_(st0)

        def calls(mask):
            kw = {} if mask is None else {"mask": mask}
            return {"hit": (lambda: None, lambda: ctx.hit(rays, None, tr, "auto", **kw)),
                    "occluded": (lambda: None, lambda: ctx.occluded(rays, None, None, tr, "auto", occ, **kw)),
                    "bounce": (restore, lambda: ctx.bounce(work, st, None, tr, "auto", out=res, **kw))}
        by_mat = tor.groups_by_material(scene)
        mod4 = (np.uint32(1) << (np.arange(len(scene)) % 4).astype(np.uint32)).astype(np.uint32)
        columns = [("unmasked", None, None)]
        if masked:
            columns += [("all", by_mat, ALL), ("no glass", by_mat, ALL & ~(1 << 2)), ("1 in 4", mod4, 1)]
        times = {e: {c[0]: [] for c in columns} for e in ENTRIES}
        for rnd in range(a.rounds + 1):                                     # round 0 warms up
            for col, groups, mask in columns:
                if groups is not None:
                    ctx.set_groups(groups)
                for e, (prep, fn) in calls(mask).items():
                    t = timed_each(prep, fn, a.reps if rnd else 1)
                    if rnd:
                        times[e][col].append(t)
        out[name] = {"rays": n, "objects": len(scene), "mode": res.mode,
                     "rates": {e: {c: [round(n / max(v) / 1e9, 3), round(n / min(v) / 1e9, 3)] for c, v in times[e].items()} for e in ENTRIES}}
        del work, st, occ, res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--incoherent", type=int, default=16 << 20)
    ap.add_argument("--parent-lib", default=None, help="libtor_mi355x.so built from the parent commit: the unmasked column is measured on it")
    ap.add_argument("--child-unmasked", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child_unmasked:
        print(json.dumps(measure(a, False)))
        return 0
    rows = measure(a, True)
    parent = None
    if a.parent_lib:
        env = dict(os.environ, TOR_AB_LIB=os.path.abspath(a.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--child-unmasked", "--reps", str(a.reps), "--rounds", str(a.rounds),
               "--samples", str(a.samples), "--incoherent", str(a.incoherent)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    lines = [f"masked_rate: G rays/s, worst .. best round ({a.rounds} rounds of {a.reps} launches), auto mode; unmasked (parent): "
             f"{a.parent_lib or '(not measured)'}",
             f"{'workload':<11}{'entry':<9}{'rays':>10}  {'unmasked (parent)':>18} {'unmasked':>16} {'all visible':>16} {'no glass':>16} {'1 in 4':>16}  all/unmasked"]
    for name, row in rows.items():
        for e in ENTRIES:
            r = row["rates"][e]
            p = parent[name]["rates"][e]["unmasked"] if parent else None
            base = p[1] if p else r["unmasked"][1]
            cell = lambda v: f"{v[0]:>7.3f} .. {v[1]:<6.3f}" if v else f"{'-':>17}"
            lines.append(f"{name:<11}{e:<9}{row['rays']:>10}  {cell(p):>18} {cell(r['unmasked'])} {cell(r['all'])} {cell(r['no glass'])} "
                         f"{cell(r['1 in 4'])}  {r['all'][1] / base:>8.3f}  ({row['mode']})")
    line = json.dumps({"tool": "masked_rate", "reps": a.reps, "rounds": a.rounds, "rows": rows, "parent": parent})
    text = "\n".join(lines + [line])
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
