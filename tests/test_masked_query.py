"""Visibility groups and per-ray masks without a GPU: the six new entry points are declared, exported and bound with the unmasked
entries' arguments plus (d_mask, mask), a C compiler sees those signatures, the Python keywords exist, every argument check that
needs no device answers TOR_ERR_INVALID_ARGUMENT, and the restatement the GPU tests hold the kernels to
(tests/masked_restatement.py: hit_restatement.world_hit on the sub-list a ray sees, `object` mapped back) is worked by hand."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hit_restatement as H
import masked_restatement as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("tor_hit_masked_device", "tor_hit_device"), ("tor_hit_masked_host", "tor_hit_host"),
         ("tor_occluded_masked_device", "tor_occluded_device"), ("tor_occluded_masked_host", "tor_occluded_host"),
         ("tor_bounce_masked_device", "tor_bounce_device"))


def _err(tor):
    return tor.lib().tor_last_error().decode()


def test_new_symbols_are_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in ("tor_scene_groups",) + tuple(p[0] for p in PAIRS):
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
        assert name in tor.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    for masked, plain in PAIRS:   # the unmasked entry's arguments, then the per-ray words and the scalar word
        assert list(getattr(L, masked).argtypes) == list(getattr(L, plain).argtypes) + [C.c_void_p, C.c_uint32], masked
    assert list(L.tor_scene_groups.argtypes) == [C.c_void_p, C.c_int64, C.c_void_p]


def test_python_keywords_exist(tor):
    for name in ("hit", "occluded", "visible", "bounce", "trace"):
        par = inspect.signature(getattr(tor.Context, name)).parameters
        assert "mask" in par and par["mask"].default is None, name
    for name in ("hit", "occluded", "bounce", "trace"):   # trailing: every existing positional call keeps its meaning
        assert list(inspect.signature(getattr(tor.Context, name)).parameters)[-1] == "mask", name
    assert callable(tor.Context.set_groups) and callable(tor.groups_by_material)
    recs = np.zeros((4, 16))
    recs[:, 10] = [0, 1, 2, 0]
    g = tor.groups_by_material(recs)
    assert g.dtype == np.uint32 and g.tolist() == [1, 2, 4, 1]
    assert tor.groups_by_material(tor.Scene.from_records(recs)).tolist() == [1, 2, 4, 1]


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_c_program_sees_the_signatures_and_the_exports(tor, tmp_path):
    prog = tmp_path / "abi.c"
    prog.write_text(r'''
#include <dlfcn.h>
#include <stdio.h>
#include "tor_render.h"
typedef int (*groups_fn)(TorContext*, int64_t, const uint32_t*);
typedef int (*hit_fn)(TorContext*, int64_t, const TorRay*, const double*, double, double, int32_t, TorHit*, void*, const uint32_t*, uint32_t);
typedef int (*hit_host_fn)(TorContext*, int64_t, const TorRay*, const double*, double, double, int32_t, TorHit*, const uint32_t*, uint32_t);
typedef int (*occ_fn)(TorContext*, int64_t, const TorRay*, const double*, const int32_t*, int64_t, double, double, int32_t, int32_t*, void*,
                      const uint32_t*, uint32_t);
typedef int (*occ_host_fn)(TorContext*, int64_t, const TorRay*, const double*, const int32_t*, int64_t, double, double, int32_t, int32_t*,
                           const uint32_t*, uint32_t);
typedef int (*bounce_fn)(TorContext*, int64_t, TorRay*, TorRng*, const int32_t*, int64_t, double, double, int32_t, TorHit*, double*,
                         int32_t*, void*, const uint32_t*, uint32_t);
int main(int argc, char** argv) {
  /* the header's declarations have exactly these types */
  groups_fn a = tor_scene_groups; hit_fn b = tor_hit_masked_device; hit_host_fn c = tor_hit_masked_host;
  occ_fn d = tor_occluded_masked_device; occ_host_fn e = tor_occluded_masked_host; bounce_fn f = tor_bounce_masked_device;
  (void)a; (void)b; (void)c; (void)d; (void)e; (void)f;
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h) { printf("dlopen: %s\n", dlerror()); return 2; }
  const char* names[6] = {"tor_scene_groups", "tor_hit_masked_device", "tor_hit_masked_host", "tor_occluded_masked_device",
                          "tor_occluded_masked_host", "tor_bounce_masked_device"};
  for (int k = 0; k < 6; ++k) if (!dlsym(h, names[k])) { printf("missing %s\n", names[k]); return 3; }
  groups_fn g = (groups_fn)dlsym(h, "tor_scene_groups");
  if (g(0, 0, 0) != TOR_ERR_INVALID_ARGUMENT) return 4;
  printf("ok\n");
  return 0;
}
''')
    exe = tmp_path / "abi"
    # (-Wl,--unresolved-symbols: the function-pointer initialisers reference the entries; they resolve when the library is loaded)
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog), tor.LIB_PATH,
                    "-Wl,-rpath," + os.path.dirname(tor.LIB_PATH), "-ldl"], check=True, capture_output=True)
    out = subprocess.run([str(exe), tor.LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_argument_checks_need_no_device(tor):
    L = tor.lib()
    b = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    assert L.tor_scene_groups(None, 0, None) == tor.ERR_INVALID_ARGUMENT and _err(tor).startswith("tor_scene_groups:")
    for name, extra in (("tor_hit_masked_device", (None,)), ("tor_hit_masked_host", ())):
        fn = getattr(L, name)

        def refused(word, ctx=b, n_rays=4, rays=b, lo=0.0, hi=1.0, mode=0, out=b):
            rc = fn(ctx, n_rays, rays, None, lo, hi, mode, out, *extra, None, 0xFFFFFFFF)
            msg = _err(tor)
            assert rc == tor.ERR_INVALID_ARGUMENT, (name, word, rc)
            assert msg.startswith(name + ":") and word in msg, (name, word, msg)

        refused("NULL", ctx=None)
        refused("n_rays", n_rays=-1)
        refused("n_rays", n_rays=(0x7fffffff * 256) + 1)
        for lo, hi in ((math.nan, 1.0), (0.0, math.inf), (1.0, 0.5)):
            refused("time range", lo=lo, hi=hi)
        for mode in (-1, 3):
            refused("mode", mode=mode)
        refused("NULL", rays=None)
        refused("NULL", out=None)
    for name, extra in (("tor_occluded_masked_device", (None,)), ("tor_occluded_masked_host", ())):
        fn = getattr(L, name)

        def refused(word, ctx=b, n_rays=4, rays=b, lst=None, n_list=4, lo=0.0, hi=1.0, mode=0, out=b):
            rc = fn(ctx, n_rays, rays, None, lst, n_list, lo, hi, mode, out, *extra, None, 1)
            msg = _err(tor)
            assert rc == tor.ERR_INVALID_ARGUMENT, (name, word, rc)
            assert msg.startswith(name + ":") and word in msg, (name, word, msg)

        refused("NULL", ctx=None)
        refused("n_rays", n_rays=-1, n_list=-1)
        refused("time range", lo=1.0, hi=0.5)
        refused("mode", mode=3)
        refused("NULL", rays=None)
        refused("NULL", out=None)
        refused("n_list", lst=b, n_list=-1)
        refused("n_list", lst=None, n_list=3)
    rc = L.tor_bounce_masked_device(None, 4, b, b, None, 4, 0.0, 1.0, 0, b, b, b, None, None, 1)
    assert rc == tor.ERR_INVALID_ARGUMENT and _err(tor).startswith("tor_bounce_masked_device:")


# ---- the restatement by hand: three unit spheres on the x axis, a ray along +x from x = -10 --------------------------------------

def _three():
    recs = np.zeros((3, 16))
    for k, x in enumerate((0.0, 4.0, 8.0)):
        recs[k, 1:4] = recs[k, 4:7] = (x, 0.0, 0.0)
        recs[k, 8], recs[k, 9] = 1.0, 1.0
    return recs, np.array([[-10.0, 0, 0, 1.0, 0, 0, 0.0]])


def test_hide_the_nearest_and_the_second_wins():
    recs, ray = _three()
    groups = np.array([1, 2, 4], dtype=np.uint32)
    f = H.fields(M.world_hit(recs, groups, ray, 0xFFFFFFFF))
    assert f["object"][0] == 0 and f["t"][0] == 9.0
    f = H.fields(M.world_hit(recs, groups, ray, 2 | 4))
    assert f["object"][0] == 1 and f["t"][0] == 13.0 and f["p"][0].tolist() == [3.0, 0.0, 0.0] and f["front_face"][0] == 1
    f = H.fields(M.world_hit(recs, groups, ray, 4))
    assert f["object"][0] == 2 and f["t"][0] == 17.0                       # the index in the FULL list
    assert M.occluded(recs, groups, ray, 4, [[0.001, 16.0]])[0] == False   # noqa: E712  (the visible one lies beyond the segment)
    assert H.fields(H.world_hit(recs, ray, [[0.001, 16.0]]))["object"][0] == 0   # ... which the unmasked query finds blocked


def test_coincident_spheres_give_the_lowest_visible_index():
    recs, ray = _three()
    recs[1], recs[2] = recs[0], recs[0]                                    # three coincident spheres
    groups = np.array([1, 2, 2], dtype=np.uint32)
    assert H.fields(M.world_hit(recs, groups, ray, 3))["object"][0] == 0
    assert H.fields(M.world_hit(recs, groups, ray, 2))["object"][0] == 1   # 1 and 2 tie: the lowest VISIBLE index
    per_ray = M.world_hit(recs, groups, np.repeat(ray, 3, axis=0), np.array([1, 2, 3], dtype=np.uint32))
    assert H.fields(per_ray)["object"].tolist() == [0, 1, 0]
    assert (H.fields(per_ray)["t"] == 9.0).all()


def test_mask_zero_misses():
    recs, ray = _three()
    raw = M.world_hit(recs, None, ray, 0)
    assert raw.view(np.int32)[0, 14] == -1 and not raw[0, :7].any() and raw.view(np.int32)[0, 15] == 0
    assert not M.occluded(recs, None, ray, 0)[0]
    raw = M.world_hit(recs, np.array([1, 1, 1], dtype=np.uint32), ray, 2)  # nothing the ray sees: the same miss
    assert raw.view(np.int32)[0, 14] == -1 and not raw[0, :7].any()


def test_every_object_visible_is_world_hit():
    recs = H.group_scene(5, 120)
    rays = H.incoherent_rays(recs, 500, 3, (-0.5, 1.5))
    want = H.world_hit(recs, rays)
    rng = np.random.default_rng(1)
    for groups, mask in ((None, 0xFFFFFFFF), (None, 1), (np.full(120, 8, dtype=np.uint32), rng.choice([8, 9, 0xFFFFFFFF], 500)),
                         (rng.integers(1, 2**32, 120, dtype=np.uint64).astype(np.uint32), 0xFFFFFFFF)):
        assert not H.mismatches(M.world_hit(recs, groups, rays, mask), want)
    assert 0.2 < (H.fields(want)["object"] >= 0).mean() < 1.0
    # int32 words count by their bits
    g = np.full(120, -2**31, dtype=np.int32)
    assert not H.mismatches(M.world_hit(recs, g, rays, np.full(500, -2**31, dtype=np.int32)), want)
    assert (H.fields(M.world_hit(recs, g, rays, 0x7FFFFFFF))["object"] == -1).all()
