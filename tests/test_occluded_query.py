"""Any-hit (occlusion) queries without a GPU: tor_occluded_device / tor_occluded_host are declared, exported and bound, every
argument check that needs no device answers TOR_ERR_INVALID_ARGUMENT with a message that names the entry, the occluded bit of the
numpy restatement of world.hit (tests/hit_restatement.py, anchored to the CPU oracle by tests/test_hit_query.py) does not depend on
the order of the list -- the claim the kernel's early exit rests on -- and Context.visible builds the segments it says it builds."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hit_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tor_occluded_device", "tor_occluded_host")


def _err(tor):
    return tor.lib().tor_last_error().decode()


def test_new_symbols_are_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in NEW:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
        assert name in tor.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    assert len(L.tor_occluded_device.argtypes) == 11 and len(L.tor_occluded_host.argtypes) == 10
    assert callable(tor.Context.occluded) and callable(tor.Context.visible)
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert "tor_occluded.hip" in mk


def test_argument_checks_need_no_device(tor):
    L = tor.lib()
    b = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    for name, extra in (("tor_occluded_device", (None,)), ("tor_occluded_host", ())):
        fn = getattr(L, name)

        def refused(word, ctx=b, n_rays=4, rays=b, lst=None, n_list=4, lo=0.0, hi=1.0, mode=0, out=b):
            rc = fn(ctx, n_rays, rays, None, lst, n_list, lo, hi, mode, out, *extra)
            msg = _err(tor)
            assert rc == tor.ERR_INVALID_ARGUMENT, (name, word, rc)
            assert msg.startswith(name + ":") and word in msg, (name, word, msg)

        # everything tor_hit_device refuses
        refused("NULL", ctx=None)
        refused("n_rays", n_rays=-1, n_list=-1)
        refused("n_rays", n_rays=(0x7fffffff * 256) + 1, n_list=(0x7fffffff * 256) + 1)
        for lo, hi in ((math.nan, 1.0), (0.0, math.nan), (-math.inf, 1.0), (0.0, math.inf), (1.0, 0.5)):
            refused("time range", lo=lo, hi=hi)
        for mode in (-1, 3, 7):
            refused("mode", mode=mode)
        refused("NULL", rays=None)
        refused("NULL", out=None)
        # the list rules of the path steps
        refused("n_list", lst=b, n_list=-1)
        refused("n_list", lst=None, n_list=3)
        refused("n_list", lst=None, n_list=0)
        refused("n_list", lst=b, n_list=(0x7fffffff * 256) + 1)
        # NULL arrays are refused with work to do, with a list too
        refused("NULL", lst=b, n_list=2, rays=None)
        refused("NULL", lst=b, n_list=2, out=None)


def test_context_occluded_rejects_bad_shapes_before_the_library(tor):
    ctx = object.__new__(tor.Context)  # a context whose creation never happened (no device here)
    ctx._h = C.c_void_p()
    for rays, tr, out in ((np.zeros((4, 6)), None, None), (np.zeros(7), None, None), (np.zeros((4, 7)), np.zeros((4, 3)), None),
                          (np.zeros((4, 7)), None, np.zeros(4, dtype=np.int64)), (np.zeros((4, 7)), None, np.zeros(5, dtype=np.int32))):
        with pytest.raises(ValueError):
            ctx.occluded(rays, t_range=tr, out=out)
    with pytest.raises(KeyError):
        ctx.occluded(np.zeros((4, 7)), mode="fastest")
    with pytest.raises(tor.TorError) as e:
        ctx.occluded(np.zeros((4, 7)))
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "tor_occluded_host" in str(e.value)  # the NULL context, refused by the library


def test_occluded_bit_does_not_depend_on_the_list_order():
    """HittableList.hit returns hit_anything; the closest_so_far it shrinks can only reject a later object's root after an earlier
    object was accepted.  So the bit is the OR of the per-object tests and survives any permutation of the list, although the
    object and the root the sequential loop ends with do not."""
    recs = R.group_scene(5)
    rays = R.incoherent_rays(recs, 4096, 31, (-1.0, 2.5))
    rng = np.random.default_rng(32)
    tr = np.stack([rng.choice([0.0, 0.001, 2.0], 4096), rng.choice([np.inf, 1.0, 5.0, 30.0], 4096)], axis=1)
    for t_range in (None, tr):
        want = R.fields(R.world_hit(recs, rays, t_range))["object"] >= 0
        assert 0.05 < want.mean() < 0.95
        for _ in range(3):
            perm = rng.permutation(len(recs))
            got = R.fields(R.world_hit(recs[perm], rays, t_range))["object"] >= 0
            assert np.array_equal(got, want)
    # ... and it IS the OR of the objects taken one at a time, each with the caller's t_max
    sub = slice(0, 512)
    each = np.stack([R.fields(R.world_hit(recs[i:i + 1], rays[sub], tr[sub]))["object"] == 0 for i in range(len(recs))], axis=1)
    assert np.array_equal(each.any(axis=1), R.fields(R.world_hit(recs, rays[sub], tr[sub]))["object"] >= 0)


def test_visible_builds_the_segments_it_says(tor):
    rng = np.random.default_rng(33)
    p, q = rng.normal(size=(17, 3)), rng.normal(size=(17, 3))
    rays, tr = tor.Context.shadow_segments(p, q)
    assert rays.shape == (17, 7) and rays.dtype == np.float64 and tr.shape == (17, 2) and tr.dtype == np.float64
    assert np.array_equal(rays[:, 0:3], p) and np.array_equal(rays[:, 3:6], q - p) and (rays[:, 6] == 0.0).all()
    assert (tr[:, 0] == 0.001).all() and (tr[:, 1] == 1.0).all()
    times = rng.uniform(0, 1, 17)
    rays, tr = tor.Context.shadow_segments(p.astype(np.float32).tolist(), q[0], time=times, t_min=0.0)
    assert rays.shape == (17, 7) and np.array_equal(rays[:, 6], times) and (tr[:, 0] == 0.0).all() and (tr[:, 1] == 1.0).all()
    assert np.array_equal(rays[:, 3:6], q[0] - rays[:, 0:3])          # one target for every origin
    one, tr1 = tor.Context.shadow_segments([0, 0, 0], [1, 2, 3])
    assert one.shape == (1, 7) and tr1.shape == (1, 2) and one[0].tolist() == [0, 0, 0, 1, 2, 3, 0]
    # visible() hands exactly these to occluded(), and negates the bits
    ctx = object.__new__(tor.Context)
    seen = {}

    class _Res:
        occluded = np.array([True, False] * 8 + [True])

    def fake(rays, t_range=None, **kw):
        seen.update(rays=rays, t_range=t_range, kw=kw)
        return _Res()

    ctx.occluded = fake
    vis = ctx.visible(p, q, time=0.25, t_min=0.01, mode="brute")
    assert np.array_equal(vis, ~_Res.occluded) and seen["kw"] == {"mode": "brute"}
    want_rays, want_tr = tor.Context.shadow_segments(p, q, 0.25, 0.01)
    assert np.array_equal(seen["rays"], want_rays) and np.array_equal(seen["t_range"], want_tr)
