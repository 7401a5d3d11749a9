"""The reach pass in front of the plane screen's whole words (tor_screen.hpp reach_ray / reach_miss; include/tor_reach.h), on the
host: a ray that does not reach a word must lose every slot of that word to the segment's own second-stage test anyway
(tor_debug_screen2_scene's code is never 2 there) and to the reference's test; degenerate rays reach every word; the pass is not
vacuous on random_scene; the Morton order is a permutation whose whole words lie inside their segment and whose boxes contain
their centres; and a build whose boxes are not grown (-DTOR_SCREEN_MUTATE=4) fails the first check.

Run as a script (the mutation check does, against the mutant build through TOR_AB_LIB) it prints the number of (ray, object) pairs
that break the first check on random_scene."""
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_filter32 import _unit
from test_plane32 import _rays, _scenes, _sphere, _translated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOK_FROM = np.array([13.0, 2.0, 3.0])   # scenes.nim's camera


def _wall():
    """A wall of spheres seen edge-on: 96 centres on the line z = 0.5 (+ the ground)."""
    recs = [_sphere(0, -1000, 0, 1000)] + [_sphere(x, 0.2, 0.5, 0.2) for x in np.linspace(-12, 12, 96)]
    return np.asarray(recs, dtype=np.float64)


def _y_movers(rng):
    """A segment of movers along y at a common height (xkind 12) and one at any height (xkind 14)."""
    recs = [_sphere(0, -1000, 0, 1000)]
    for i in range(160):
        x, z = rng.uniform(-9, 9, 2)
        y = 0.2 if i < 90 else rng.uniform(0.2, 3.0)
        recs.append([1, x, y, z, x, y + rng.uniform(-0.3, 0.6), z, 0.0, 1.0, 0.2, 0, .5, .5, .5, 0, 0])
    return np.asarray(recs, dtype=np.float64)


def _shifted_origin(shift):
    return np.asarray(shift, dtype=np.float64)


def _sane_rays(rng, recs, shift, n):
    """Camera rays and bounce rays: from the ground and from sphere surfaces, up and down; times inside [0, 1]."""
    shift = _shifted_origin(shift)
    small = np.flatnonzero(np.abs(recs[:, 9]) < 5.0)
    # camera rays at points of the field
    o_cam = np.tile(LOOK_FROM + shift, (n, 1)) + rng.normal(0, 0.05, (n, 3))
    tgt = np.column_stack([rng.uniform(-11, 11, n), rng.uniform(0.0, 0.4, n), rng.uniform(-11, 11, n)]) + shift
    d_cam = tgt - o_cam
    # bounce rays leaving the ground (the ground sphere's top is y = shift.y)
    o_gr = np.column_stack([rng.uniform(-11, 11, n), np.zeros(n), rng.uniform(-11, 11, n)]) + shift
    d_gr = _unit(rng, n)
    d_gr[:, 1] = np.abs(d_gr[:, 1]) + 1e-3
    # bounce rays leaving sphere surfaces, up and down
    pick = rng.choice(small, n)
    nrm = _unit(rng, n)
    o_sp = recs[pick, 1:4] + nrm * np.abs(recs[pick, 9])[:, None]
    d_sp = nrm + 0.9 * _unit(rng, n)
    o = np.concatenate([o_cam, o_gr, o_sp])
    d = np.concatenate([d_cam, d_gr, d_sp]) * rng.choice([1.0, 1e-3, 1e3], size=(3 * n, 1))
    return o, d, rng.uniform(0.0, 1.0, 3 * n)


def _edge_rays(rng, recs, boxes, n):
    """Rays that run exactly along a word box's edge, start exactly on one, or have dy = 0 at the slab's faces and inside it."""
    real = boxes[np.isfinite(boxes).all(axis=1)]
    if len(real) == 0:
        real = np.array([[-1.0, 1.0, -1.0, 1.0, 0.0, 0.4]])
    b = real[rng.integers(0, len(real), n)]
    corner_x = np.where(rng.random(n) < 0.5, b[:, 0], b[:, 1])
    corner_z = np.where(rng.random(n) < 0.5, b[:, 2], b[:, 3])
    y_face = np.where(rng.random(n) < 0.5, b[:, 4], b[:, 5])
    o = np.column_stack([corner_x, y_face, corner_z])
    along = rng.integers(0, 4, n)
    d = np.zeros((n, 3))
    d[along == 0] = [1.0, 0.0, 0.0]            # along the edge, dy = 0, on the slab's face
    d[along == 1] = [0.0, 0.0, -1.0]
    d[along == 2] = [1.0, 0.0, 1.0]            # leaving the corner outward or inward, dy = 0
    d[along == 3] = [-1.0, 0.0, -1.0]
    back = rng.uniform(0.0, 4.0, (n, 1)) * (rng.random((n, 1)) < 0.7)
    o = o - d * back
    tilt = rng.choice([0.0, 0.0, 1e-12, -1e-12, 0.3, -0.3], n)
    d[:, 1] = tilt
    flat_inside = rng.random(n) < 0.3          # dy = 0 inside the slab, towards the field
    o[flat_inside, 1] = (0.5 * (b[:, 4] + b[:, 5]))[flat_inside]
    d[flat_inside, 1] = 0.0
    return o, d, rng.uniform(0.0, 1.0, n)


def _degenerate_rays(rng, recs, shift, n):
    """Rays that must reach every word: a time fraction outside [0, 1] or not a number (movers), wild and non-finite rays, no
    ground track.  Returns (o, d, t, statics_too): statics_too False where only a mover segment is degenerate (its f)."""
    shift = _shifted_origin(shift)
    o = np.column_stack([rng.uniform(-11, 11, n), rng.uniform(0.0, 3.0, n), rng.uniform(-11, 11, n)]) + shift
    d = _unit(rng, n)
    t = rng.uniform(0.0, 1.0, n)
    kind = np.arange(n) % 8
    t[kind == 0] = rng.uniform(1.0001, 3.0, np.count_nonzero(kind == 0))
    t[kind == 1] = rng.uniform(-3.0, -0.0001, np.count_nonzero(kind == 1))
    t[kind == 2] = np.nan
    d[kind == 3] = d[kind == 3] * 1e-310                 # wild: |d|^2 underflows
    d[kind == 4] = d[kind == 4] * 1e200                  # wild: |d|^2 overflows
    d[kind == 5] = [0.0, -1.0, 0.0]                      # vertical: no ground track
    o[kind == 6, 0] = np.inf                             # non-finite origin
    d[kind == 7, 2] = np.nan                             # non-finite direction
    return o, d, t, kind >= 3


def _need(tor, recs, o, d, t):
    """The reference's own test per (ray, object) (tor_selftest_screen_host's `need`)."""
    n_rays, n_obj = len(t), len(recs)
    R, O = np.meshgrid(np.arange(n_rays), np.arange(n_obj), indexing="ij")
    R, O = R.ravel(), O.ravel()
    c0 = recs[O, 1:4]
    dc = recs[O, 4:7] - c0
    mv = (recs[O, 0] != 0).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(mv != 0, (t[R] - recs[O, 7]) / (recs[O, 8] - recs[O, 7]), 0.0)
    _, need = tor.selftest_screen(o[R], d[R], c0, dc, mv, f, recs[O, 9] ** 2)
    return need.reshape(n_rays, n_obj) != 0


def _violations(tor, recs, o, d, t):
    """(pairs where the word is not reached and yet stage two keeps the slot or the reference hits it, unreached pairs, boxed pairs)"""
    scene = tor.Scene.from_records(recs)
    reach, word, _, _ = tor.debug_reach_scene(scene.list(), o, d, t)
    keep, _ = tor.debug_screen2_scene(scene.list(), o, d, t)
    need = _need(tor, recs, o, d, t)
    unreached = reach == 0
    assert not np.any(unreached[:, word < 0])
    bad = unreached & ((keep == 2) | need)
    return int(np.count_nonzero(bad)), int(np.count_nonzero(unreached)), int(np.count_nonzero(word >= 0)) * len(t), np.argwhere(bad)[:5]


def _all_scenes(tor, rng):
    """(name, records, shift): random_scene, the mixed scene, the cloud and the field of tests/test_plane32.py where they are and at
    +-1e4 and +-1e7; a wall seen edge-on; a segment of movers along y."""
    xs, zs = np.meshgrid(np.linspace(-10, 10, 9), np.linspace(-10, 10, 9))
    field = np.asarray([_sphere(x, 0.2, z, 0.2) for x, z in zip(xs.ravel(), zs.ravel())], dtype=np.float64)
    out = []
    for name, recs in _scenes(tor, rng) + [("field", field)]:
        for shift in ((0.0, 0.0, 0.0), (1e4, 0.0, -1e4), (-1e7, 3.0, 1e7)):
            out.append((name, _translated(recs, np.asarray(shift)), shift))
    out.append(("wall", _wall(), (0.0, 0.0, 0.0)))
    out.append(("y movers", _y_movers(rng), (0.0, 0.0, 0.0)))
    return out


def test_an_unreached_word_holds_no_candidate(tor):
    """For every ray x object of every scene: the word is not reached => stage two's code is not 2 and the reference misses."""
    rng = np.random.default_rng(71)
    total_unreached = 0
    for name, recs, shift in _all_scenes(tor, rng):
        scene = tor.Scene.from_records(recs)
        _, _, _, boxes = tor.debug_reach_scene(scene.list(), np.zeros((1, 3)), np.ones((1, 3)), np.zeros(1))
        o1, d1, t1 = _sane_rays(rng, recs, shift, 120)
        o2, d2, t2 = _rays(rng, recs, 200)                       # tests/test_plane32.py's: near objects, aimed, times in [-0.2, 1.2]
        o3, d3, t3 = _edge_rays(rng, recs, boxes, 160)
        if name == "wall":                                       # edge-on: along the wall's line, from both ends and from inside
            k = 60
            o4 = np.column_stack([rng.uniform(-20, 20, k), rng.uniform(0.0, 0.5, k), np.full(k, 0.5) + rng.choice([0.0, 0.0, 0.19, -0.21], k)])
            d4 = np.column_stack([rng.choice([-1.0, 1.0], k), rng.choice([0.0, 1e-3, -1e-2], k), np.zeros(k)])
            o1, d1, t1 = np.concatenate([o1, o4]), np.concatenate([d1, d4]), np.concatenate([t1, np.zeros(k)])
        o, d, t = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3]), np.concatenate([t1, t2, t3])
        bad, unreached, boxed, where = _violations(tor, recs, o, d, t)
        assert bad == 0, (name, shift, bad, where)
        total_unreached += unreached
        # (at +-1e7 the slack, 2^-21 of the ray's bound B -- twice what stage two's own margin 2^-45 B^2 lets it keep --, is 9 units:
        # most of a field of 22 is reached, as it is kept)
        # (random_scene's 481 are in Morton order; the small segments keep the order of appearance: their boxes are wide)
        if name in ("random_scene", "field", "wall", "y movers") and abs(shift[0]) <= 1e4:
            assert boxed > 0 and unreached > (0.3 * boxed if name == "random_scene" else 0), (name, shift, boxed, unreached)
    assert total_unreached > 100000


def test_degenerate_rays_reach_every_word(tor):
    rng = np.random.default_rng(72)
    for name, recs, shift in _all_scenes(tor, rng):
        o, d, t, statics_too = _degenerate_rays(rng, recs, shift, 64)
        scene = tor.Scene.from_records(recs)
        reach, word, _, _ = tor.debug_reach_scene(scene.list(), o, d, t)
        _, kind = tor.debug_screen2_scene(scene.list(), o, d, t)
        assert np.all(reach[statics_too] == 1), (name, shift)
        timed = np.isin(kind, (12, 14))                          # the segments that have a time fraction
        assert np.all(reach[:, timed] == 1), (name, shift)


def test_the_pass_is_not_vacuous_on_random_scene(tor):
    """At least half of all (ray, boxed word) pairs of camera and bounce rays are unreached."""
    rng = np.random.default_rng(73)
    recs = tor.random_scene(0xFACADE).to_records()
    o, d, t = _sane_rays(rng, recs, (0.0, 0.0, 0.0), 400)
    reach, word, _, boxes = tor.debug_reach_scene(tor.Scene.from_records(recs).list(), o, d, t)
    words = np.unique(word[word >= 0])
    assert len(words) == 15                                      # 481 resting spheres: 15 whole words and a block
    first_of_word = np.array([np.flatnonzero(word == w)[0] for w in words])
    unreached = reach[:, first_of_word] == 0                     # (a word's reach bit is the same for all its objects)
    for w in words:
        assert np.all(reach[:, word == w] == reach[:, [np.flatnonzero(word == w)[0]]])
    share = float(np.mean(unreached))
    print(f"random_scene: {share:.3f} of the (ray, whole word) pairs are unreached; camera {np.mean(unreached[:400]):.3f}, "
          f"ground {np.mean(unreached[400:800]):.3f}, surfaces {np.mean(unreached[800:]):.3f}")
    assert share >= 0.5


def test_morton_order_words_and_boxes(tor):
    """The order inside a segment is a permutation of its objects, a boxed word lies wholly inside one segment of xkind 10 / 11 / 12
    / 14, boxes contain their centres (and the slab both ends of a mover's travel), the segments stay as tests/test_screen.py pins
    them, and consecutive slots are near each other on the ground."""
    rng = np.random.default_rng(74)
    for name, recs, shift in _all_scenes(tor, rng):
        scene = tor.Scene.from_records(recs)
        segs = tor.debug_layout_segments(scene.list())
        reach, word, slot, boxes = tor.debug_reach_scene(scene.list(), np.zeros((1, 3)), np.ones((1, 3)), np.zeros(1))
        _, kind = tor.debug_screen2_scene(scene.list(), np.zeros((1, 3)), np.ones((1, 3)), np.zeros(1))
        assert len(np.unique(slot)) == len(recs) and slot.min() >= 0
        seg_of = np.full(len(recs), -1)
        for s, (xkind, n_obj, n_slots, first) in enumerate(segs):
            inside = (slot >= first) & (slot < first + n_obj)
            assert np.count_nonzero(inside) == n_obj, (name, s)                  # a permutation of the segment's objects
            assert np.all(kind[inside] == xkind)
            seg_of[inside] = s
        assert np.all(seg_of >= 0)
        boxed = word >= 0
        assert np.all(word[boxed] == slot[boxed] // 32)
        for w in np.unique(word[boxed]):
            members = np.flatnonzero(word == w)
            xkind, n_obj, n_slots, first = segs[seg_of[members[0]]]
            assert xkind in (10, 11, 12, 14) and first <= 32 * w and 32 * (w + 1) <= first + n_slots, (name, w)
            assert len(members) == min(32, first + n_obj - 32 * w)                # every real slot of the word
            b = boxes[w]
            r = np.abs(recs[members, 9])
            for c in (recs[members, 1:4], recs[members, 4:7]):
                assert np.all(b[0] <= c[:, 0] - r) and np.all(c[:, 0] + r <= b[1]) and np.all(b[2] <= c[:, 2] - r) and np.all(c[:, 2] + r <= b[3])
                assert np.all(b[4] <= c[:, 1] - r) and np.all(c[:, 1] + r <= b[5])
        unboxed_words = np.setdiff1d(np.arange(len(boxes)), word[boxed])
        assert np.all(np.isinf(boxes[unboxed_words][:, :4]))
    assert tor.debug_layout_segments(tor.random_scene(0xFACADE).list()) == [(12, 481, 488, 0), (10, 4, 8, 488)]
    # random_scene: a word is a patch of ground, not a sample of the whole field (22 x 22 units)
    recs = tor.random_scene(0xFACADE).to_records()
    _, word, _, boxes = tor.debug_reach_scene(tor.random_scene(0xFACADE).list(), np.zeros((1, 3)), np.ones((1, 3)), np.zeros(1))
    area = [(boxes[w][1] - boxes[w][0]) * (boxes[w][3] - boxes[w][2]) for w in np.unique(word[word >= 0])]
    assert np.median(area) < 0.25 * 22.0 * 22.0, area


def _mutant_library(tmp):
    """The library with -DTOR_SCREEN_MUTATE=4 built into `tmp` with the flags of tools/mutation_check.sh -- its host side (`make
    hostlib`): this test runs no kernel, so the mutant's host objects are linked with the kernels' objects of the in-tree build.
    Without an in-tree build's objects the whole mutant is built, as the script does (a minute and a half)."""
    csrc = os.path.join(ROOT, "trace-of-radiance_amd", "csrc")
    kobj = os.path.join(ROOT, "trace-of-radiance_amd", "lib", "obj")
    flags = "-O2 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden -munsafe-fp-atomics -Wall -Wno-unused-function -pthread"
    target = "hostlib" if os.path.exists(os.path.join(kobj, "tor_kernels.hip.o")) else "all"
    r = subprocess.run(["make", "-C", csrc, f"OUT={tmp}", f"KOBJ={kobj}", "JOBS=16", f"CXXFLAGS={flags} -DTOR_SCREEN_MUTATE=4", target],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(tmp, "libtor_mi355x.so")


def _script_count(env_lib):
    env = dict(os.environ)
    env.pop("TOR_AB_LIB", None)
    if env_lib:
        env["TOR_AB_LIB"] = env_lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return int(r.stdout.strip().splitlines()[-1])


def test_ungrown_boxes_fail_the_first_check():
    """-DTOR_SCREEN_MUTATE=4 (boxes and slab not grown by the radius, no slack, nothing rounded outward): rays that graze the
    spheres at a word's rim find candidates in words they do not reach.  The product build finds none on the same rays."""
    with tempfile.TemporaryDirectory(prefix="tor_mut4_") as tmp:
        lib = _mutant_library(tmp)
        mutant = _script_count(lib)
    assert mutant > 0
    assert _script_count(None) == 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    tor_mod = importlib.import_module("trace-of-radiance_amd")
    rng_main = np.random.default_rng(75)
    recs_main = tor_mod.random_scene(0xFACADE).to_records()
    o_m, d_m, t_m = _sane_rays(rng_main, recs_main, (0.0, 0.0, 0.0), 300)
    print(_violations(tor_mod, recs_main, o_m, d_m, t_m)[0])
