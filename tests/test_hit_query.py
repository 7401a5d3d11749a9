"""Closest-hit queries without a GPU: tor_hit_device / tor_hit_host are declared, exported and bound, the TorRay / TorHit mirrors
match the header, every argument check that needs no device answers TOR_ERR_INVALID_ARGUMENT, and the numpy restatement of
world.hit (tests/hit_restatement.py) -- what the GPU tests hold the kernels to -- is anchored to the CPU oracle, which the reference's
PNG pins: at max_depth = 1 a sample is black exactly when its camera ray hits something."""
import ctypes as C
import math
import os
import re

import numpy as np

import hit_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tor_hit_device", "tor_hit_host")


def _err(tor):
    return tor.lib().tor_last_error().decode()


def test_new_symbols_are_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in NEW:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
        assert name in tor.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    assert "TOR_HIT_AUTO = 0, TOR_HIT_BRUTE = 1, TOR_HIT_BLOCKS = 2" in src
    assert (tor.HIT_AUTO, tor.HIT_BRUTE, tor.HIT_BLOCKS) == (0, 1, 2)
    assert callable(tor.Context.hit)
    assert L.tor_version() == b"tor_mi355x 0.6 (gfx950)"


def test_struct_mirrors_match_the_header(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    assert "typedef struct TorRay { TorVec3 origin, direction; double time; } TorRay;" in src
    assert "typedef struct TorHit { TorVec3 p, normal; double t; int32_t object; int32_t front_face; } TorHit;" in src
    assert C.sizeof(tor.Ray) == 56
    assert (tor.Ray.origin.offset, tor.Ray.direction.offset, tor.Ray.time.offset) == (0, 24, 48)
    assert C.sizeof(tor.Hit) == 64
    assert (tor.Hit.p.offset, tor.Hit.normal.offset, tor.Hit.t.offset, tor.Hit.object.offset, tor.Hit.front_face.offset) == \
        (0, 24, 48, 56, 60)
    # the library checks the same layout at compile time
    q = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "tor_query.hip")).read()
    assert "sizeof(TorRay) == 56" in q and "sizeof(TorHit) == 64" in q
    assert "tor_query.hip" in open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()


def test_argument_checks_need_no_device(tor):
    L = tor.lib()
    b = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    for fn, extra in ((L.tor_hit_device, (None,)), (L.tor_hit_host, ())):
        assert fn(None, 4, b, None, 0.0, 1.0, 0, b, *extra) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
        assert fn(b, -1, b, None, 0.0, 1.0, 0, b, *extra) == tor.ERR_INVALID_ARGUMENT and "n_rays" in _err(tor)
        for lo, hi in ((math.nan, 1.0), (0.0, math.nan), (-math.inf, 1.0), (0.0, math.inf), (1.0, 0.5)):
            assert fn(b, 4, b, None, lo, hi, 0, b, *extra) == tor.ERR_INVALID_ARGUMENT, (lo, hi)
            assert "time range" in _err(tor)
        for mode in (-1, 3, 7):
            assert fn(b, 4, b, None, 0.0, 1.0, mode, b, *extra) == tor.ERR_INVALID_ARGUMENT and "mode" in _err(tor)
        assert fn(b, 4, None, None, 0.0, 1.0, 0, b, *extra) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
        assert fn(b, 4, b, None, 0.0, 1.0, 0, None, *extra) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)


def test_context_hit_rejects_bad_shapes_before_the_library(tor):
    ctx = object.__new__(tor.Context)  # a context whose creation never happened (no device here)
    ctx._h = C.c_void_p()
    for rays, tr in ((np.zeros((4, 6)), None), (np.zeros(7), None), (np.zeros((4, 7)), np.zeros((4, 3)))):
        try:
            ctx.hit(rays, t_range=tr)
        except ValueError:
            continue
        raise AssertionError("Context.hit accepted a malformed batch")
    try:
        ctx.hit(np.zeros((4, 7)), mode="fastest")
    except KeyError:
        pass
    else:
        raise AssertionError("Context.hit accepted an unknown mode")
    try:
        ctx.hit(np.zeros((4, 7)))
    except tor.TorError as e:
        assert e.code == tor.ERR_INVALID_ARGUMENT  # the NULL context, refused by the library
    else:
        raise AssertionError("a NULL context must raise")


def _sphere(c, r):
    return [0, *c, *c, 0, 1, r, 0, .5, .5, .5, 0, 0]


def _mover(c0, c1, t0, t1, r):
    return [1, *c0, *c1, t0, t1, r, 0, .5, .5, .5, 0, 0]


def test_restatement_on_cases_worked_by_hand():
    recs = np.array([_sphere((0, 0, -5), 1.0), _sphere((0, 0, -5), 1.0), _sphere((0, 0, -2.5), 0.5),
                     _mover((3, 0, -5), (3, 2, -5), 0.0, 1.0, 1.0), _sphere((0, 10, 0), -2.0)])
    rays = np.array([
        [0, 0, 0, 0, 0, -1, 0.5],     # straight at the small sphere in front: t = 2, object 2
        [0, 0, -5, 0, 0, -1, 0.5],    # from inside the duplicate pair: second root, back face, the lower index (0)
        [3, 1, 0, 0, 0, -1, 0.5],     # the mover at time 0.5 sits at y = 1: t = 4
        [3, 1, 0, 0, 0, -1, math.nan],  # ... and a NaN time never hits it
        [0, 0, 0, 0, 0, 0, 0.0],      # zero direction: never a hit
        [0, 15, 0, 0, -1, 0, 0.0],    # negative radius: t = 3, the outward normal points inward, so front_face flips
    ])
    got = R.fields(R.world_hit(recs, rays))
    assert list(got["object"]) == [2, 0, 3, -1, -1, 4]
    assert list(got["t"]) == [2.0, 1.0, 4.0, 0.0, 0.0, 3.0]
    assert list(got["front_face"]) == [1, 0, 1, 0, 0, 0]
    assert np.array_equal(got["normal"][0], [0, 0, 1]) and np.array_equal(got["normal"][1], [0, 0, 1])
    assert np.array_equal(got["normal"][5], [0, 1, 0]) and np.array_equal(got["p"][5], [0, 12, 0])
    # t_max cuts the first hit off, t_min pushes past it
    cut = R.fields(R.world_hit(recs, rays[:1], np.array([[0.001, 2.0]])))
    assert cut["object"][0] == -1
    far = R.fields(R.world_hit(recs, rays[:1], np.array([[2.5, np.inf]])))
    assert far["object"][0] == 2 and far["t"][0] == 3.0 and far["front_face"][0] == 0


def test_restatement_is_the_order_independent_minimum():
    """What the kernels compute -- the smallest accepted root over all objects, ties to the lowest index -- is what the sequential
    closest_so_far loop gives, on random lists with exact duplicates (ties) and random t ranges."""
    rng = np.random.default_rng(7)
    base = R.group_scene(3, 120)
    recs = np.concatenate([base, base[rng.integers(0, len(base), 40)]])   # duplicates behind their originals
    recs = recs[rng.permutation(len(recs))]
    rays = R.incoherent_rays(recs, 4000, 11, (-1.0, 2.5))
    tr = np.stack([rng.choice([0.0, 0.001, 2.0], 4000), rng.choice([np.inf, 5.0, 30.0], 4000)], axis=1)
    seq = R.world_hit(recs, rays, tr)
    # per object alone: its accepted root under the caller's (t_min, t_max)
    roots = np.stack([R.fields(R.world_hit(recs[i:i + 1], rays, tr))["t"] for i in range(len(recs))], axis=1)
    hit = np.stack([R.fields(R.world_hit(recs[i:i + 1], rays, tr))["object"] == 0 for i in range(len(recs))], axis=1)
    roots = np.where(hit, roots, np.inf)
    want = np.where(hit.any(axis=1), np.argmin(roots, axis=1), -1)   # argmin: the first (lowest) index among equal minima
    assert np.array_equal(R.fields(seq)["object"], want)
    s = np.sort(roots, axis=1)
    assert hit.sum() > 1000 and ((s[:, 0] == s[:, 1]) & np.isfinite(s[:, 0])).sum() > 10   # hits, and ties among them


def test_restatement_matches_the_oracle_on_camera_rays(oracle, ref_scene, ref_camera):
    """random_scene at 96x54, sample 0 of the per-sample streams, max_depth = 1: a hit is black (the depth runs out or the material
    absorbs), a miss is the sky (every channel > 0).  The restatement's hit mask on the regenerated camera rays must be the oracle's
    black pixels."""
    objs, _ = ref_scene
    nrows, ncols = 54, 96
    sums, _ = oracle.accumulate(nrows, ncols, 0, 1, ref_camera, objs, max_depth=1)
    black = (sums == 0).all(axis=2).reshape(-1)
    assert black.any() and not black.all()
    rays = R.camera_rays(oracle, ref_camera, nrows, ncols)
    got = R.fields(R.world_hit(objs, rays))
    assert np.array_equal(got["object"] >= 0, black)
