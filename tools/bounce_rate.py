#!/usr/bin/env python3
"""Rates of the path steps (tor_bounce_device and friends) against the fused queries, from one run on the same rays, in auto mode:
    camera      the camera rays of random_scene at 1920x1080, samples [0, 16) (tor_camera_rays_device, TOR_SEED_SAMPLE)
    incoherent  16 M rays with seeded origins in random_scene's box, uniform directions and seed1 states
    anim120     frame 120 of the animation (1601 spheres, the two-level culling layout): its camera rays at 1920x1080, one sample
(a) one step: tor_bounce_device against tor_hit_device, G rays/s, with the bytes a step moves per ray (a hit reads the ray and
    the state and writes the ray, the state, the record, the attenuation and the status: 88 + 180 B; a miss reads the ray and writes
    record, attenuation and status: 56 + 92 B) over its time: the achieved traffic.  The step overwrites its rays and states, so
    they are restored (untimed) before every launch; each launch sits between two events of its own.
(b) the chain at depth 50: Context.trace and a bare C-ABI loop (tor_bounce_device + tor_sky_device + tor_bounce_select_device, the
    colours composed with torch) against tor_radiance_device on the same rays and states, M paths/s; colours and states hashed:
    all three must give the same bytes.  Events around the whole chain (its host synchronisations included).
Warm-up first, REPS launches per round, ROUNDS rounds with the candidates interleaved; best and worst round printed (the spread).
Prints a table and one JSON line.

    python tools/bounce_rate.py [--reps 3] [--rounds 3] [--samples 16] [--out FILE.json]
"""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

tor = importlib.import_module("trace-of-radiance_amd")
H, W, DEPTH = 1080, 1920, 50
HIT_BYTES = (56 + 32, 56 + 32 + 64 + 24 + 4)   # a hit: read ray + state; write ray, state, record, attenuation, status
MISS_BYTES = (56, 64 + 24 + 4)                 # a miss: read the ray; write record, attenuation, status


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
    """Seconds per launch of fn, each launch between two events of its own, prepare() (untimed) before each."""
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


def c_chain(ctx, rays, st, depth, tr, buf):
    """The bare C-ABI loop on full-size arrays and a shrinking list; st is updated in place.  Returns the colours."""
    L = tor.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = rays.shape[0]
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    work, hits, step_att, status, sky, color, att, lists = buf
    work.copy_(rays)
    color.zero_()
    att.fill_(1.0)
    cur, n_live = None, n
    for k in range(depth):
        if n_live == 0:
            break
        tor._check(L.tor_bounce_device(ctx._h, n, p(work), p(st), p(cur), n_live, tr[0], tr[1], tor.HIT_AUTO, p(hits), p(step_att),
                                       p(status), s))
        tor._check(L.tor_sky_device(ctx._h, n, p(work), p(cur), n_live, p(sky), s))      # (of every stepped ray: used where it missed)
        idx = slice(None) if cur is None else cur[:n_live].long()
        stat = status[idx]
        a = att[idx]
        color[idx] = torch.where((stat == tor.BOUNCE_MISS)[:, None], sky[idx] * a, color[idx])
        att[idx] = torch.where((stat == tor.BOUNCE_SCATTERED)[:, None], a * step_att[idx], a)
        nxt, n_out = lists[k % 2], C.c_int64(0)
        tor._check(L.tor_bounce_select_device(ctx._h, n, p(status), p(cur), n_live, p(nxt), C.byref(n_out), s))
        cur, n_live = nxt, int(n_out.value)
    return color


def digest(color, st):
    torch.cuda.synchronize()
    return hashlib.sha256(color.cpu().numpy().tobytes() + st.cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--incoherent", type=int, default=16 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261016)
    rscene, rcam = tor.random_scene(0xFACADE), tor.camera()
    it = iter(tor.Animation(H, W, 0.005, 0.0, 7.2).scenes(6))
    for _ in range(121):
        acam, ascene, _t = next(it)
    rows = []
    for name, scene, cam, ns in (("camera", rscene, rcam, a.samples), ("incoherent", rscene, None, 0), ("anim120", ascene, acam, 1)):
        ctx = tor.Context()
        ctx.upload(scene.list())
        if cam is not None:
            rays, st0 = ctx.camera_rays(cam, H, W, 0, ns, tor.SEED_SAMPLE)
        else:
            rays, st0 = incoherent(scene.to_records(), a.incoherent, gen)
        n = rays.shape[0]
        times = rays[:, 6]
        tr = (float(times.min()), float(times.max()))
        # ---- (a) one step against one hit query ----
        work, st = rays.clone(), st0.clone()
        res = ctx.bounce(work, st, None, tr, "auto")                                      # warm-up; the step's outcome counts
        torch.cuda.synchronize()
        n_miss = int((res.status == tor.BOUNCE_MISS).sum())
        n_absorbed = int((res.status == tor.BOUNCE_ABSORBED).sum())
        step_mode = res.mode
        hit_mode = ctx.hit(rays, None, tr, "auto").mode
        torch.cuda.synchronize()
        step_bytes = (n - n_miss) * sum(HIT_BYTES) + n_miss * sum(MISS_BYTES)
        t_step, t_hit = [], []

        def restore():
            work.copy_(rays)
            st.copy_(st0)
        for _ in range(a.rounds):
            t_hit.append(timed_each(lambda: None, lambda: ctx.hit(rays, None, tr, "auto"), a.reps))
            t_step.append(timed_each(restore, lambda: ctx.bounce(work, st, None, tr, "auto", out=res), a.reps))
        # ---- (b) the chain against the radiance query ----
        buf = (torch.empty_like(rays), torch.empty((n, 8), dtype=torch.float64, device="cuda"),
               torch.empty((n, 3), dtype=torch.float64, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda"),
               torch.zeros((n, 3), dtype=torch.float64, device="cuda"), torch.zeros((n, 3), dtype=torch.float64, device="cuda"),
               torch.ones((n, 3), dtype=torch.float64, device="cuda"), [torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2)])
        del work, res
        cands = {"radiance": lambda: ctx.radiance(rays, st, DEPTH, tr, "auto")[0],
                 "trace": lambda: ctx.trace(rays, st, DEPTH, time_range=tr, mode="auto")[0],
                 "c_chain": lambda: c_chain(ctx, rays, st, DEPTH, tr, buf)}
        hashes, t_chain = {}, {k: [] for k in cands}
        for k, fn in cands.items():                                                       # warm-up and the outputs' hashes
            st.copy_(st0)
            hashes[k] = digest(fn(), st)
        for _ in range(a.rounds):
            for k, fn in cands.items():
                t_chain[k].append(timed_each(lambda: st.copy_(st0), fn, a.reps))
        best = lambda ts: min(ts)
        row = {"workload": name, "objects": len(scene), "rays": n, "step_mode": step_mode, "hit_mode": hit_mode,
               "first_step": {"miss": n_miss, "absorbed": n_absorbed, "scattered": n - n_miss - n_absorbed},
               "hit_grays_s": [round(n / max(t_hit) / 1e9, 3), round(n / best(t_hit) / 1e9, 3)],
               "step_grays_s": [round(n / max(t_step) / 1e9, 3), round(n / best(t_step) / 1e9, 3)],
               "step_over_hit": round(best(t_hit) / best(t_step), 3),
               "step_bytes_per_ray": round(step_bytes / n, 1), "step_gb_s": round(step_bytes / best(t_step) / 1e9, 1),
               "hit_gb_s": round(n * (56 + 64) / best(t_hit) / 1e9, 1),
               "chain_mpaths_s": {k: [round(n / max(v) / 1e6, 1), round(n / best(v) / 1e6, 1)] for k, v in t_chain.items()},
               "trace_over_radiance": round(best(t_chain["radiance"]) / best(t_chain["trace"]), 3),
               "c_chain_over_radiance": round(best(t_chain["radiance"]) / best(t_chain["c_chain"]), 3),
               "hashes": hashes, "hashes_equal": len(set(hashes.values())) == 1}
        rows.append(row)
        del buf, cands
        ctx.close()
        torch.cuda.empty_cache()
    print("(a) one step against one hit query, G rays/s (worst .. best round)")
    print(f"{'workload':<12}{'rays':>10}  {'hit':>15}  {'step':>15}  step/hit  B/ray  step GB/s  hit GB/s  first step: miss / absorbed / scattered")
    for r in rows:
        f = r["first_step"]
        print(f"{r['workload']:<12}{r['rays']:>10}  {r['hit_grays_s'][0]:>6.3f} .. {r['hit_grays_s'][1]:<6.3f} {r['step_grays_s'][0]:>6.3f} .. "
              f"{r['step_grays_s'][1]:<6.3f} {r['step_over_hit']:>8.3f} {r['step_bytes_per_ray']:>6.1f} {r['step_gb_s']:>10.1f} {r['hit_gb_s']:>9.1f}  "
              f"{f['miss']} / {f['absorbed']} / {f['scattered']}  ({r['step_mode']})")
    print(f"(b) the chain at depth {DEPTH}, M paths/s (worst .. best round)")
    print(f"{'workload':<12}{'radiance':>20}{'trace':>20}{'c_chain':>20}  trace/rad  c_chain/rad  hashes equal")
    for r in rows:
        c = r["chain_mpaths_s"]
        print(f"{r['workload']:<12}" + "".join(f"{c[k][0]:>10.1f} .. {c[k][1]:<6.1f}" for k in ("radiance", "trace", "c_chain")) +
              f"  {r['trace_over_radiance']:>9.3f}  {r['c_chain_over_radiance']:>11.3f}  {r['hashes_equal']}  {r['hashes']['radiance']}")
    line = json.dumps({"tool": "bounce_rate", "depth": DEPTH, "reps": a.reps, "rounds": a.rounds, "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["hashes_equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
