"""Ordered multi-hit queries without a GPU: tor_crossings_device / tor_crossings_host are declared, exported and bound with matching
signatures, every argument check that needs no device answers TOR_ERR_INVALID_ARGUMENT with its reason, and the numpy restatement
the GPU tests compare against (tests/crossings_restatement.py) is itself held to hand-worked cases, to hit_restatement.world_hit
for crossing 0, to the order independence the kernel's pruning rests on, and to the chain property: crossing k + 1 is world.hit
with t_min := crossing k's t."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import crossings_restatement as X
import hit_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tor_crossings_device", "tor_crossings_host")


def _err(tor):
    return tor.lib().tor_last_error().decode()


def _sphere(c, r, mat=0):
    return [0, *c, *c, 0, 1, r, mat, .5, .5, .5, 0, 1.5]


def test_new_symbols_are_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in NEW:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
        assert name in tor.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
        # the C parameter list and the ctypes signature have the same length
        decl = re.search(r"TOR_API\s+int\s+" + name + r"\s*\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(getattr(L, name).argtypes), name
    assert len(L.tor_crossings_device.argtypes) == 16 and len(L.tor_crossings_host.argtypes) == 15
    assert re.search(r"TOR_CROSSINGS_MAX\s*=\s*(\d+)", src).group(1) == str(tor.CROSSINGS_MAX)
    assert re.search(r"typedef struct TorCrossing \{ double t; int32_t object; int32_t which; \} TorCrossing;", src)
    kw = list(inspect.signature(tor.Context.crossings).parameters)
    assert kw == ["self", "rays", "k", "t_range", "index", "time_range", "mode", "mask", "records", "out"]
    assert hasattr(tor, "CrossingsResult")
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*tor_crossings\.hip", mk, re.M) and re.search(r"^ASM_SRCS = .*tor_crossings\.hip", mk, re.M)


def test_argument_checks_need_no_device(tor):
    L = tor.lib()
    b = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    for name, extra in (("tor_crossings_device", (None,)), ("tor_crossings_host", ())):
        fn = getattr(L, name)

        def refused(word, ctx=b, n_rays=4, rays=b, lst=None, n_list=4, k=4, lo=0.0, hi=1.0, mode=0, cross=b, count=b):
            rc = fn(ctx, n_rays, rays, None, lst, n_list, k, None, 0xFFFFFFFF, lo, hi, mode, cross, count, None, *extra)
            msg = _err(tor)
            assert rc == tor.ERR_INVALID_ARGUMENT, (name, word, rc)
            assert msg.startswith(name + ":") and word in msg, (name, word, msg)

        refused("NULL", ctx=None)
        refused("n_rays", n_rays=-1, n_list=-1)
        refused("n_rays", n_rays=(0x7fffffff * 256) + 1, n_list=(0x7fffffff * 256) + 1)
        for k in (0, -1, tor.CROSSINGS_MAX + 1, 1 << 20):
            refused("k must be", k=k)
        for lo, hi in ((math.nan, 1.0), (0.0, math.nan), (-math.inf, 1.0), (0.0, math.inf), (1.0, 0.5)):
            refused("time range", lo=lo, hi=hi)
        for mode in (-1, 3, 7):
            refused("mode", mode=mode)
        refused("NULL", rays=None)
        refused("NULL", cross=None)
        refused("NULL", count=None)
        # the list rules of tor_occluded_device
        refused("n_list", lst=b, n_list=-1)
        refused("n_list", lst=None, n_list=3)
        refused("n_list", lst=b, n_list=(0x7fffffff * 256) + 1)
        refused("NULL", lst=b, n_list=2, cross=None)


def test_context_crossings_rejects_bad_arguments_before_the_library(tor):
    ctx = object.__new__(tor.Context)  # a context whose creation never happened (no device here)
    ctx._h = C.c_void_p()
    for rays, k, tr in ((np.zeros((4, 6)), 2, None), (np.zeros(7), 2, None), (np.zeros((4, 7)), 2, np.zeros((4, 3))),
                        (np.zeros((4, 7)), 0, None), (np.zeros((4, 7)), tor.CROSSINGS_MAX + 1, None)):
        with pytest.raises(ValueError):
            ctx.crossings(rays, k, t_range=tr)
    with pytest.raises(ValueError):
        ctx.crossings(np.zeros((4, 7)), 2, out=np.zeros((4, 2, 2)))
    with pytest.raises(KeyError):
        ctx.crossings(np.zeros((4, 7)), 2, mode="fastest")
    with pytest.raises(tor.TorError) as e:
        ctx.crossings(np.zeros((4, 7)), 2)
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "tor_crossings_host" in str(e.value)  # the NULL context, refused by the library


def test_hollow_glass_ball_by_hand():
    """Concentric radii r = 2 and -0.9 r = -1.8 at the origin, a ray along +x from x = -5: the roots are 5 -+ 2 and 5 -+ 1.8
    (exactly: the discriminants 4 and 3.24... are computed from 25 - 21 and 25 - 21.76; the near roots take which = 0)."""
    recs = np.array([_sphere((0, 0, 0), 2.0, 2), _sphere((0, 0, 0), -1.8, 2)])
    ray = np.array([[-5.0, 0, 0, 1, 0, 0, 0]])
    cr = X.crossings(recs, ray, 6)
    assert cr["count"][0] == 4 and cr["total"][0] == 4 and not cr["tied"][0]
    assert cr["object"][0].tolist() == [0, 1, 1, 0, -1, -1] and cr["which"][0].tolist() == [0, 0, 1, 1, 0, 0]
    want = [5.0 - 2.0, 5.0 - math.sqrt(25.0 - (25.0 - 1.8 * 1.8)), 5.0 + math.sqrt(25.0 - (25.0 - 1.8 * 1.8)), 7.0, 0.0, 0.0]
    assert cr["t"][0].tolist() == want
    assert abs(cr["t"][0, 1] - 3.2) < 1e-12 and abs(cr["t"][0, 2] - 6.8) < 1e-12
    # truncation keeps the first k, and the count saturates
    cr2 = X.crossings(recs, ray, 2)
    assert cr2["count"][0] == 2 and cr2["total"][0] == 4 and cr2["t"][0].tolist() == want[:2]
    # the records: the outer shell is entered from outside (front face), the inner shell's negative radius turns its normal inward
    rec = X.records(recs, ray, cr)
    w = rec.view(np.int32)
    assert w[0, :, 14].tolist() == [0, 1, 1, 0, -1, -1]
    assert rec[0, 0, 0:3].tolist() == [-2.0, 0, 0] and rec[0, 0, 3:6].tolist() == [-1.0, 0, 0] and w[0, 0, 15] == 1
    assert w[0, 1, 15] == 0 and w[0, 2, 15] == 1 and w[0, 3, 15] == 0     # negative radius: outward = (p - c) / r points inward
    assert (rec[0, 4:, 0:7] == 0).all()


def test_origin_inside_miss_cut_range_and_ties_by_hand():
    one = np.array([_sphere((0, 0, 0), 1.0)])
    # from inside: only the far root lies ahead
    cr = X.crossings(one, np.array([[0.0, 0, 0, 1, 0, 0, 0]]), 4)
    assert cr["count"][0] == 1 and cr["t"][0, 0] == 1.0 and cr["object"][0, 0] == 0 and cr["which"][0, 0] == 1
    # a miss: every entry unused
    cr = X.crossings(one, np.array([[0.0, 5, 0, 1, 0, 0, 0]]), 4)
    assert cr["count"][0] == 0 and (cr["object"][0] == -1).all() and (cr["t"][0] == 0).all() and (cr["which"][0] == 0).all()
    # a range that cuts between the roots 4 and 6: either one alone; the comparisons are strict
    ray = np.array([[-5.0, 0, 0, 1, 0, 0, 0]])
    for tr, want in (((0.001, 5.0), [(4.0, 0)]), ((5.0, 100.0), [(6.0, 1)]), ((4.0, 6.0), []), ((0.001, 6.0), [(4.0, 0)]),
                     ((np.nextafter(4.0, 0), np.nextafter(6.0, 7)), [(4.0, 0), (6.0, 1)])):
        cr = X.crossings(one, ray, 4, np.array([tr]))
        got = [(cr["t"][0, e], cr["which"][0, e]) for e in range(cr["count"][0])]
        assert got == want, (tr, got)
    # two identical spheres tie at both roots: the lower index first, and an equal t is reported
    two = np.array([_sphere((0, 0, 0), 1.0), _sphere((0, 0, 0), 1.0)])
    cr = X.crossings(two, ray, 4)
    assert cr["t"][0].tolist() == [4.0, 4.0, 6.0, 6.0] and cr["object"][0].tolist() == [0, 1, 0, 1]
    assert cr["which"][0].tolist() == [0, 0, 1, 1] and cr["tied"][0]
    cr = X.crossings(two, ray, 1)
    assert cr["object"][0].tolist() == [0] and cr["tied"][0]              # entries K and K + 1 share one t: the lower index is kept


@pytest.fixture(scope="module")
def scene_rays():
    recs = R.group_scene(5)
    rays = R.incoherent_rays(recs, 4096, 31, (-1.0, 2.5))
    rng = np.random.default_rng(32)
    tr = np.stack([rng.choice([0.0, 0.001, 2.0], 4096), rng.choice([np.inf, 5.0, 30.0], 4096)], axis=1)
    return recs, rays, tr


def test_crossing_0_is_world_hit(scene_rays):
    recs, rays, tr = scene_rays
    for t_range in (None, tr):
        hit = R.fields(R.world_hit(recs, rays, t_range))
        cr = X.crossings(recs, rays, 3, t_range)
        assert np.array_equal(cr["object"][:, 0], hit["object"])
        assert np.array_equal(cr["t"][:, 0].view(np.uint64), hit["t"].view(np.uint64))
        assert np.array_equal(cr["count"] == 0, hit["object"] < 0)
        assert 0.05 < (hit["object"] >= 0).mean() < 0.95
        # ... and its record is world_hit's, in all 8 words
        rec = X.records(recs, rays, cr)
        assert not R.mismatches(rec[:, 0], R.world_hit(recs, rays, t_range))


def test_crossings_do_not_depend_on_the_list_order(scene_rays):
    """The crossings are a set of keys, one per (object, root); a permutation of the list renames the objects and nothing else.
    Mapped back, every t, object and which is the same wherever no two crossings share a t (there the tie order follows the
    permuted indices, as specified)."""
    recs, rays, tr = scene_rays
    rng = np.random.default_rng(33)
    want = X.crossings(recs, rays, 3, tr)
    clear = ~want["tied"]
    assert clear.mean() > 0.99 and (want["total"] > 3).sum() > 40         # truncation is in the batch
    for _ in range(3):
        perm = rng.permutation(len(recs))
        got = X.crossings(recs[perm], rays, 3, tr)
        back = np.where(got["object"] >= 0, perm[np.maximum(got["object"], 0)], -1)
        assert np.array_equal(got["count"], want["count"])
        assert np.array_equal(got["t"][clear].view(np.uint64), want["t"][clear].view(np.uint64))
        assert np.array_equal(back[clear], want["object"][clear]) and np.array_equal(got["which"][clear], want["which"][clear])


def test_chain_property(scene_rays):
    """On rays without equal-t crossings, crossing k + 1 is world.hit with t_min := crossing k's t: same ray, same objects, same
    roots; only the range moves."""
    recs, rays, tr = scene_rays
    cr = X.crossings(recs, rays, 5, tr)
    clear = ~cr["tied"]
    assert clear.mean() > 0.99
    t_range = tr.copy()
    for k in range(5):
        hit = R.fields(R.world_hit(recs, rays, t_range))
        assert np.array_equal(hit["object"][clear], cr["object"][clear, k]), k
        assert np.array_equal(hit["t"][clear].view(np.uint64), cr["t"][clear, k].view(np.uint64)), k
        t_range[:, 0] = np.where(hit["object"] >= 0, hit["t"], t_range[:, 0])
        t_range[:, 1] = np.where(hit["object"] >= 0, t_range[:, 1], -1.0)   # a ray that has missed stays a miss
    assert (cr["count"] == 5).sum() > 40 and (cr["count"] == 0).sum() > 40


def test_masked_restatement_is_the_sub_list(scene_rays):
    recs, rays, tr = scene_rays
    groups = (np.uint32(1) << recs[:, 10].astype(np.uint32)).astype(np.uint32)
    masks = np.random.default_rng(34).choice(np.array([0, 1, 2, 5, X.ALL], dtype=np.uint32), len(rays))
    got = X.masked_crossings(recs, groups, rays, masks, 4, tr)
    assert (got["count"][masks == 0] == 0).all()
    full = X.crossings(recs, rays, 4, tr)
    every = masks == X.ALL
    for name in ("t", "object", "which", "count"):
        assert np.array_equal(got[name][every], full[name][every])
    glass = np.nonzero(groups == 4)[0]
    sel = masks == 5                                                      # Lambertian and glass
    seen = np.nonzero((groups & 5) != 0)[0]
    sub = X.crossings(recs[seen], rays[sel], 4, tr[sel])
    assert np.array_equal(np.where(sub["object"] >= 0, seen[np.maximum(sub["object"], 0)], -1), got["object"][sel])
    assert glass.size and np.isin(got["object"][sel], np.concatenate([seen, [-1]])).all()
