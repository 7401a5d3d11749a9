#!/usr/bin/env python3
"""Rates of the ordered multi-hit queries (tor_crossings_device) against what a host does without them -- K chained closest-hit
queries (tor_hit_device) with t_min moved to the last t on the device -- on the same device arrays in one process: M rays/s per
(scene, ray set, mode).  The workloads are tools/occluded_rate.py's:
    scenes     random_scene (485 objects) and frame 120 of the animation (1601 spheres, the two-level culling layout)
    ray sets   camera, incoherent, segments (see occluded_rate.py)
    modes      brute, blocks
Legs, interleaved per round between HIP events:
    hit_a      one tor_hit_device launch -- of the library --parent-lib names (the parent commit's build, loaded next to this one
               with a context of its own on the same scene), else of this build
    chain K    K tor_hit_device launches of that same library, t_min := t of the last hit between them (one torch.where on the
               device; a ray that has missed keeps missing), for K = 2, 4 and TOR_CROSSINGS_MAX
    cross K    one tor_crossings_device launch at K = 1, 2, 4 and TOR_CROSSINGS_MAX, into outputs allocated before the timing
    hit_b      hit_a again: the run-to-run spread
Every leg: WARM warm-up launches, then ROUNDS timings of REPS back-to-back runs; the median over the rounds.  The claim under test:
crossings(K) beats the K chained hits on the blocks rows by more than the spread of the two hit legs; rows where it does not are
marked.  K = 1 is reported against hit as a plain number.  crossing 0 must equal hit's (t, object) on every row.  Writes the table
to --out and prints one JSON line.

    python tools/crossings_rate.py [--parent-lib /path/to/parent/libtor_mi355x.so] [--reps 2] [--rounds 5] [--warm 1]
                                   [--out profiles/crossings_rate.txt]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import occluded_rate as W  # noqa: E402  (the workloads)

tor = importlib.import_module("trace-of-radiance_amd")
MODES = ("brute", "blocks")
KMAX = tor.CROSSINGS_MAX
CHAIN_KS = (2, 4, KMAX)
CROSS_KS = (1, 2, 4, KMAX)


class ParentHit:
    """tor_hit_device of another build of the library (the parent commit's), on a context of its own with the same scene."""

    def __init__(self, path, scene):
        self.L = C.CDLL(os.path.abspath(path))
        self.L.tor_last_error.restype = C.c_char_p
        self.L.tor_context_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
        self.L.tor_context_destroy.argtypes = [C.c_void_p]
        self.L.tor_scene_upload.argtypes = [C.c_void_p, tor.HittableList]
        tor._bind(self.L, ("tor_hit_device", "tor_hit_host"))
        self.h = C.c_void_p()
        self._ok(self.L.tor_context_create(-1, C.byref(self.h)))
        self._ok(self.L.tor_scene_upload(self.h, scene.list()))

    def _ok(self, rc):
        if rc != 0:
            raise SystemExit("crossings_rate: parent library: " + self.L.tor_last_error().decode("utf-8", "replace"))

    def hit(self, rays, t_range, tr, mode, raw):
        stream = torch.cuda.current_stream().cuda_stream
        self._ok(self.L.tor_hit_device(self.h, int(rays.shape[0]), C.c_void_p(rays.data_ptr()),
                                       C.c_void_p(t_range.data_ptr() if t_range is not None else 0), tr[0], tr[1], tor.HIT_MODES[mode],
                                       C.c_void_p(raw.data_ptr()), C.c_void_p(stream)))

    def close(self):
        self.L.tor_context_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="libtor_mi355x.so built from the parent commit: the hit and chain legs run on it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossings_rate.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("crossings_rate: no GPU -- a rate is measured on the device or not at all")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261017)
    it = iter(tor.Animation(1080, 1920, 0.005, 0.0, 7.2).scenes(6))
    for _ in range(121):
        acam, ascene, _t = next(it)
    legs_order = ["hit_a"] + [f"chain{k}" for k in CHAIN_KS] + [f"cross{k}" for k in CROSS_KS] + ["hit_b"]
    rows = []
    for sname, scene, cam in (("random_scene", tor.random_scene(0xFACADE), tor.camera()), ("anim120", ascene, acam)):
        ctx = tor.Context()
        ctx.upload(scene.list())
        parent = ParentHit(a.parent_lib, scene) if a.parent_lib else None
        for rname, rays, t_range in W.ray_sets(ctx, cam, scene.to_records(), a.rays, gen):
            n = int(rays.shape[0])
            tr = tuple(float(v) for v in torch.aminmax(rays[:, 6]))
            raw = torch.empty((n, 8), dtype=torch.float64, device="cuda")
            words = raw.view(torch.int32)
            base = t_range if t_range is not None else torch.tensor([0.001, float("inf")], dtype=torch.float64, device="cuda").repeat(n, 1)
            moving = base.clone()
            for m in MODES:
                def hit(tr_now):
                    if parent is not None:
                        parent.hit(rays, tr_now, tr, m, raw)
                        return raw[:, 6], words[:, 14]
                    h = ctx.hit(rays, tr_now, tr, m)
                    return h.t, h.object

                def chain(k):
                    moving.copy_(base)
                    for _ in range(k):
                        t, obj = hit(moving)
                        found = obj >= 0
                        moving[:, 0] = torch.where(found, t, moving[:, 0])
                        moving[:, 1] = torch.where(found, moving[:, 1], torch.full_like(t, -1.0))

                legs = {"hit_a": lambda: hit(t_range), "hit_b": lambda: hit(t_range)}
                legs.update({f"chain{k}": (lambda k=k: chain(k)) for k in CHAIN_KS})
                outs = {k: ctx.crossings(rays, k, t_range, None, tr, m) for k in CROSS_KS}   # written again by every timed call
                legs.update({f"cross{k}": (lambda k=k: ctx.crossings(rays, k, t_range, None, tr, m, out=outs[k])) for k in CROSS_KS})
                for leg in legs_order:
                    for _ in range(a.warm):
                        legs[leg]()
                t0, o0 = hit(t_range)
                t0, o0 = t0.clone(), o0.clone()
                c = ctx.crossings(rays, KMAX, t_range, None, tr, m)
                torch.cuda.synchronize()
                equal = bool(torch.equal(c.object[:, 0], o0) and torch.equal(c.t[:, 0].view(torch.int64), t0.view(torch.int64)))
                mean_count = float(c.count.double().mean())
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
                spread = abs(rate["hit_a"] - rate["hit_b"]) / max(rate["hit_a"], rate["hit_b"])
                gain = {k: rate[f"cross{k}"] / rate[f"chain{k}"] for k in CHAIN_KS}
                rows.append({"scene": sname, "objects": len(scene), "rays": rname, "n": n, "mode": m, "ran": c.mode,
                             "mean_count_at_max": round(mean_count, 3), "mrays_s": {k: round(v, 1) for k, v in rate.items()},
                             "hit_spread": round(spread, 4), "cross1_vs_hit": round(rate["cross1"] / max(rate["hit_a"], rate["hit_b"]), 3),
                             "cross_vs_chain": {str(k): round(v, 2) for k, v in gain.items()},
                             "claim_holds": {str(k): bool(v > 1.0 + spread) for k, v in gain.items()}, "equal": equal})
        if parent is not None:
            parent.close()
        ctx.close()
    lines = [f"crossings_rate: M rays/s, median of {a.rounds} rounds of {a.reps} runs after {a.warm} warm-up runs, HIP events; "
             f"{torch.cuda.get_device_name(0)}; hit and chain legs: {'the parent build ' + a.parent_lib if a.parent_lib else 'this build'}",
             f"{'scene':<13}{'rays':<11}{'mode':<7}{'count@max':>9}{'hit':>9}" + "".join(f"{'chain' + str(k):>9}" for k in CHAIN_KS)
             + "".join(f"{'cross' + str(k):>9}" for k in CROSS_KS) + f"{'hit again':>10}{'spread':>8}{'c1/hit':>8}"
             + "".join(f"{'x/ch' + str(k):>8}" for k in CHAIN_KS) + "  claim  equal"]
    for r in rows:
        g = r["mrays_s"]
        claim = "holds" if all(r["claim_holds"].values()) else "FAILS at K=" + ",".join(k for k, v in r["claim_holds"].items() if not v)
        lines.append(f"{r['scene']:<13}{r['rays']:<11}{r['mode']:<7}{r['mean_count_at_max']:>9.2f}{g['hit_a']:>9.1f}"
                     + "".join(f"{g['chain' + str(k)]:>9.1f}" for k in CHAIN_KS) + "".join(f"{g['cross' + str(k)]:>9.1f}" for k in CROSS_KS)
                     + f"{g['hit_b']:>10.1f}{r['hit_spread']:>8.3f}{r['cross1_vs_hit']:>8.2f}"
                     + "".join(f"{r['cross_vs_chain'][str(k)]:>8.2f}" for k in CHAIN_KS) + f"  {claim}  {r['equal']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "crossings_rate", "unit": "M rays/s", "reps": a.reps, "rounds": a.rounds, "warm": a.warm,
                      "parent_lib": a.parent_lib, "rows": rows}))
    return 0 if all(r["equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
