"""Path steps without a GPU: the six new entry points are declared, exported, bound and laid out as a C compiler sees them; every
argument check that needs no device answers TOR_ERR_INVALID_ARGUMENT; and the numpy restatement of one step
(tests/bounce_restatement.py) -- what the GPU tests hold the kernels to -- is anchored: chained max_depth times it equals
radiance_restatement.radiance (which test_radiance_query.py ties to the oracle's sample sums and the reference's PNG), colours and
states, bit for bit; plus cases worked by hand for each material."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bounce_restatement as BR
import radiance_restatement as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tor_bounce_device", "tor_bounce_host", "tor_scatter_device", "tor_scatter_host", "tor_sky_device", "tor_bounce_select_device")


def _err(tor):
    return tor.lib().tor_last_error().decode()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_new_symbols_are_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in NEW:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
        assert name in tor.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    assert "enum { TOR_BOUNCE_MISS = 0, TOR_BOUNCE_SCATTERED = 1, TOR_BOUNCE_ABSORBED = 2 };" in src
    assert (tor.BOUNCE_MISS, tor.BOUNCE_SCATTERED, tor.BOUNCE_ABSORBED) == (0, 1, 2) == (BR.MISS, BR.SCATTERED, BR.ABSORBED)
    for name in ("bounce", "scatter", "sky", "bounce_select", "trace"):
        assert callable(getattr(tor.Context, name))
    assert issubclass(tor.BounceResult, tor.HitResult)


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_c_program_sees_the_layout_and_the_exports(tor, tmp_path):
    prog = tmp_path / "abi.c"
    prog.write_text(r'''
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>
#include "tor_render.h"
_Static_assert(sizeof(TorHit) == 64 && offsetof(TorHit, normal) == 24 && offsetof(TorHit, t) == 48, "TorHit");
_Static_assert(offsetof(TorHit, object) == 56 && offsetof(TorHit, front_face) == 60, "TorHit: object, front_face");
_Static_assert(sizeof(TorRay) == 56 && sizeof(TorRng) == 32, "TorRay, TorRng");
_Static_assert(TOR_BOUNCE_MISS == 0 && TOR_BOUNCE_SCATTERED == 1 && TOR_BOUNCE_ABSORBED == 2, "status");
typedef int (*bounce_fn)(TorContext*, int64_t, TorRay*, TorRng*, const int32_t*, int64_t, double, double, int32_t, TorHit*, double*,
                         int32_t*, void*);
typedef int (*select_fn)(TorContext*, int64_t, const int32_t*, const int32_t*, int64_t, int32_t*, int64_t*, void*);
int main(int argc, char** argv) {
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
  bounce_fn bd = (bounce_fn)dlsym(h, "tor_bounce_device");
  select_fn sel = (select_fn)dlsym(h, "tor_bounce_select_device");
  if (!bd || !sel || !dlsym(h, "tor_bounce_host") || !dlsym(h, "tor_scatter_device") || !dlsym(h, "tor_scatter_host") ||
      !dlsym(h, "tor_sky_device")) { fprintf(stderr, "missing export\n"); return 3; }
  int64_t n_out = 7;
  printf("%zu %d %d\n", sizeof(TorHit), bd(NULL, 1, NULL, NULL, NULL, 1, 0.0, 1.0, TOR_HIT_AUTO, NULL, NULL, NULL, NULL),
         sel(NULL, 1, NULL, NULL, 1, NULL, &n_out, NULL));
  return n_out == 7 ? 0 : 4;
}
''')
    exe = tmp_path / "abi"
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe), "-ldl"],
                   check=True)
    out = subprocess.run([str(exe), tor.LIB_PATH], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["64", str(tor.ERR_INVALID_ARGUMENT), str(tor.ERR_INVALID_ARGUMENT)]


def test_argument_checks_need_no_device(tor):
    L = tor.lib()
    b = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    bad = tor.ERR_INVALID_ARGUMENT
    for fn, extra in ((L.tor_bounce_device, (None,)), (L.tor_bounce_host, ())):
        def call(ctx=b, n=4, rays=b, rng=b, lst=None, n_list=4, lo=0.0, hi=1.0, mode=0, hits=b, att=b, status=b):
            return fn(ctx, n, rays, rng, lst, n_list, lo, hi, mode, hits, att, status, *extra)
        assert call(ctx=None) == bad and "NULL" in _err(tor)
        assert call(n=-1) == bad and "n_rays" in _err(tor)
        assert call(n_list=-1, lst=b) == bad and "n_list" in _err(tor)
        assert call(n_list=3) == bad and "n_list" in _err(tor)          # no list: n_list must be n_rays
        for lo, hi in ((math.nan, 1.0), (0.0, math.inf), (1.0, 0.5)):
            assert call(lo=lo, hi=hi) == bad and "time range" in _err(tor)
        for mode in (-1, 3):
            assert call(mode=mode) == bad and "mode" in _err(tor)
        for kw in ("rays", "rng", "hits", "att", "status"):
            assert call(**{kw: None}) == bad and "NULL" in _err(tor), kw
    for fn, extra in ((L.tor_scatter_device, (None,)), (L.tor_scatter_host, ())):
        def call(ctx=b, n=4, rays=b, hits=b, rng=b, lst=None, n_list=4, att=b, status=b):
            return fn(ctx, n, rays, hits, rng, lst, n_list, att, status, *extra)
        assert call(ctx=None) == bad and "NULL" in _err(tor)
        assert call(n=-1) == bad and "n_rays" in _err(tor)
        assert call(n_list=-1, lst=b) == bad and "n_list" in _err(tor)
        assert call(n_list=5) == bad and "n_list" in _err(tor)
        for kw in ("rays", "hits", "rng", "att", "status"):
            assert call(**{kw: None}) == bad and "NULL" in _err(tor), kw
    sky = L.tor_sky_device
    assert sky(None, 4, b, None, 4, b, None) == bad and "NULL" in _err(tor)
    assert sky(b, -1, b, None, -1, b, None) == bad and "n_rays" in _err(tor)
    assert sky(b, 4, b, None, 2, b, None) == bad and "n_list" in _err(tor)
    assert sky(b, 4, None, None, 4, b, None) == bad and "NULL" in _err(tor)
    assert sky(b, 4, b, None, 4, None, None) == bad and "NULL" in _err(tor)
    sel = L.tor_bounce_select_device
    n_out = C.c_int64(7)
    assert sel(None, 4, b, None, 4, b, C.byref(n_out), None) == bad and "NULL" in _err(tor)
    assert sel(b, 4, b, None, 4, b, None, None) == bad and "NULL" in _err(tor)
    assert sel(b, -1, b, None, -1, b, C.byref(n_out), None) == bad and "n_rays" in _err(tor)
    assert sel(b, 2**31, b, None, 4, b, C.byref(n_out), None) == bad and "n_rays" in _err(tor)
    assert sel(b, 4, b, b, -1, b, C.byref(n_out), None) == bad and "n_in" in _err(tor)
    assert sel(b, 4, b, None, 3, b, C.byref(n_out), None) == bad and "n_in" in _err(tor)
    assert sel(b, 4, None, None, 4, b, C.byref(n_out), None) == bad and "NULL" in _err(tor)
    assert sel(b, 4, b, None, 4, None, C.byref(n_out), None) == bad and "NULL" in _err(tor)
    assert sel(b, 4, b, b, 4, b, C.byref(n_out), None) == bad and "alias" in _err(tor)
    assert n_out.value == 7


# ---- the restatement: cases worked by hand ------------------------------------------------------------------------------------

def _sphere(radius, mat, albedo=(0, 0, 0), fuzz=0.0, ri=0.0):
    return np.asarray([[0, 0, 0, 0, 0, 0, 0, 0, 1, radius, mat, *albedo, fuzz, ri]], dtype=np.float64)


def _draws(oracle, state, n):
    """The state after n draws."""
    st = np.array(state, dtype=np.uint64).reshape(1, 4).copy()
    for _ in range(n):
        oracle.lib().oracle_rng_uniform01(RR._ptr(st, 0))
    return st[0]


HEAD_ON = np.array([[0, 0, 3, 0, 0, -1, 0.3]], dtype=np.float64)   # hits the unit sphere at (0, 0, 1), t = 2, normal (0, 0, 1)


def test_by_hand_lambertian_and_miss(oracle, tor):
    recs = _sphere(1.0, 0, (.4, .2, .1))
    st = tor.rng_seed1(np.arange(2, dtype=np.uint64))
    rays = np.concatenate([HEAD_ON, [[0, 0, 3, 0, 0, 1, 0.7]]])     # the second ray points away: a miss
    res = BR.step(oracle, recs, rays, st)
    assert res["status"].tolist() == [BR.SCATTERED, BR.MISS]
    rec = BR.H.fields(res["raw"])
    assert rec["object"].tolist() == [0, -1] and rec["t"].tolist() == [2.0, 0.0] and rec["front_face"].tolist() == [1, 0]
    assert res["attenuation"].tolist() == [[.4, .2, .1], [0, 0, 0]]
    assert res["rays"][0, 0:3].tolist() == [0, 0, 1] and res["rays"][0, 6] == 0.3         # origin rec.p, the time kept
    off = res["rays"][0, 3:6] - np.array([0, 0, 1.0])                                      # normal + a unit vector
    assert abs(np.linalg.norm(off) - 1.0) < 1e-12
    assert (res["states"][0] == _draws(oracle, st[0], 2)).all()                            # two draws
    assert (_bits(res["rays"][1]) == _bits(rays[1])).all() and (res["states"][1] == st[1]).all()   # the miss: untouched
    assert (res["raw"][1, :7] == 0).all()


def test_by_hand_metal_scatters_and_is_absorbed(oracle, tor):
    sharp = BR.step(oracle, _sphere(1.0, 1, (.7, .6, .5), 0.0), HEAD_ON, tor.rng_seed1(np.array([5], dtype=np.uint64)))
    assert sharp["status"].tolist() == [BR.SCATTERED] and sharp["attenuation"].tolist() == [[.7, .6, .5]]
    assert sharp["rays"][0].tolist() == [0, 0, 1, 0, 0, 1, 0.0]       # the mirror direction (fuzz 0), time 0 (rays.nim:19)
    # fuzz 3: some draws push the direction below the surface -> absorbed; `scattered` is written all the same
    n = 64
    st = tor.rng_seed1(np.arange(n, dtype=np.uint64))
    res = BR.step(oracle, _sphere(1.0, 1, (.7, .6, .5), 3.0), np.repeat(HEAD_ON, n, axis=0), st)
    absorbed = res["status"] == BR.ABSORBED
    assert absorbed.any() and (res["status"] == BR.SCATTERED).any() and (absorbed | (res["status"] == BR.SCATTERED)).all()
    assert (res["attenuation"][absorbed] == 0).all() and (res["attenuation"][~absorbed] == [.7, .6, .5]).all()
    L = oracle.lib()
    for i in range(n):
        g = st[i:i + 1].copy()
        while True:
            v = [L.oracle_rng_uniform_range(RR._ptr(g, 0), -1.0, 1.0) for _ in range(3)]
            if v[0] * v[0] + v[1] * v[1] + v[2] * v[2] < 1.0:
                break
        want = [0.0 + v[0] * 3.0, 0.0 + v[1] * 3.0, 1.0 + v[2] * 3.0]
        assert res["rays"][i].tolist() == [0, 0, 1, *want, 0.0], i
        assert bool(absorbed[i]) == (not want[2] > 0) and (res["states"][i] == g[0]).all()


def test_by_hand_dielectric(oracle, tor):
    glass = _sphere(1.0, 2, ri=1.5)
    # total internal reflection from inside: no draw, the state is unchanged
    inside = np.array([[0, 0.9, 0, 1, 0, 0, 0.4]], dtype=np.float64)
    st = tor.rng_seed1(np.array([9], dtype=np.uint64))
    res = BR.step(oracle, glass, inside, st)
    rec = BR.H.fields(res["raw"])
    assert rec["front_face"].tolist() == [0] and res["status"].tolist() == [BR.SCATTERED]
    assert res["attenuation"].tolist() == [[1, 1, 1]] and (res["states"] == st).all() and res["rays"][0, 6] == 0.0
    n = rec["normal"][0]
    assert (res["rays"][0, 3:6] == np.array([1.0, 0, 0]) - n * (2.0 * n[0])).all()         # reflect((1, 0, 0), n)
    # head on from outside: reflects with probability r0 = ((1 - 1/1.5) / (1 + 1/1.5))^2 = 0.04, else goes straight through
    k = 400
    st = tor.rng_seed1(np.arange(k, dtype=np.uint64))
    res = BR.step(oracle, glass, np.repeat(HEAD_ON, k, axis=0), st)
    up = res["rays"][:, 5] == 1.0
    assert (res["status"] == BR.SCATTERED).all() and (res["attenuation"] == 1).all() and (res["rays"][:, 6] == 0).all()
    assert 0 < up.sum() < k / 5 and (res["rays"][~up, 3:6] == [0, 0, -1]).all() and (res["rays"][up, 3:6] == [0, 0, 1]).all()
    L = oracle.lib()
    eta = 1.0 / 1.5
    r0 = (1.0 - eta) / (1.0 + eta)
    r0 = r0 * r0
    for i in range(k):
        g = st[i:i + 1].copy()
        assert bool(up[i]) == (L.oracle_rng_uniform01(RR._ptr(g, 0)) < r0) and (res["states"][i] == g[0]).all()   # one draw


def test_by_hand_scatter_takes_the_callers_record_and_lists(oracle, tor):
    recs = RR.three_material_scene()
    rays = np.repeat(np.array([[0, 1, 5, 0, 0, -1, 0.3]]), 5, axis=0)   # head on at the glass sphere (object 1), normal (0, 0, 1)
    st = tor.rng_seed1(np.arange(5, dtype=np.uint64))
    raw = BR.H.world_hit(recs, rays)
    assert BR.H.fields(raw)["object"].tolist() == [1] * 5 and raw[0, 3:6].tolist() == [0, 0, 1]
    raw[1, 3:6] = [0.0, 0.6, 0.8]                       # a perturbed normal
    raw.view(np.int32)[2, 14] = 99                      # no such object: a miss
    raw.view(np.int32)[3, 14] = 4                       # another object's material (the sharp metal) on the same record
    res = BR.scatter(oracle, recs, rays, raw, st, index=[3, 2, 1, 0, -1, 5])
    assert res["status"].tolist() == [1, 1, 0, 1, 0] and (res["states"][4] == st[4]).all() and (res["states"][2] == st[2]).all()
    assert res["attenuation"][3].tolist() == [.7, .6, .5] and res["attenuation"][2].tolist() == [0, 0, 0]
    assert res["rays"][3].tolist() == [0, 1, 1, 0, 0, 1, 0.0]
    assert (_bits(res["rays"][4]) == _bits(rays[4])).all() and (_bits(res["rays"][2]) == _bits(rays[2])).all()
    # ray 0 goes straight on or straight back; ray 1 follows the caller's normal
    assert res["rays"][0, 3:5].tolist() == [0, 0] and res["rays"][1, 4] != 0


# ---- the anchor ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [1, 2, 50])
@pytest.mark.parametrize("scene", ["random", "three"])
def test_chained_steps_equal_the_radiance_restatement(oracle, ref_scene, ref_camera, scene, depth):
    """max_depth steps driven the reference's way (bounce_restatement.trace with its defaults) give radiance_restatement.radiance's
    colours and states bit for bit -- and so the oracle's sample sums, which test_radiance_query.py ties that restatement to."""
    recs = ref_scene[0] if scene == "random" else RR.three_material_scene()
    cam = ref_camera if scene == "random" else oracle.camera(look_from=(0, 2, 9), look_at=(0, 0.8, 0), vfov=40.0)
    nrows, ncols, first, ns = 9, 16, 3, 2
    pixels = np.arange(nrows * ncols)[::2] if scene == "random" else None
    rays, st = RR.camera_rays(oracle, cam, nrows, ncols, pixels, first, ns)
    want_c, want_s = RR.radiance(oracle, recs, rays, st, depth)
    lengths = []
    color, st_out = BR.trace(oracle, recs, rays, st, depth, on_bounce=lambda k, index, res: lengths.append(len(index)))
    assert (_bits(color) == _bits(want_c)).all() and (st_out == want_s).all()
    assert lengths[0] == rays.shape[0] and lengths == sorted(lengths, reverse=True) and len(lengths) <= depth
    s, m = RR.sums_and_moments(color, rays.shape[0] // ns, ns)
    want_sum, want_mom = oracle.accumulate(nrows, ncols, first, ns, cam, recs, max_depth=depth, pixels=pixels)
    sel = pixels if pixels is not None else np.arange(nrows * ncols)
    assert (_bits(s) == _bits(want_sum.reshape(-1, 3)[sel])).all() and (_bits(m) == _bits(want_mom.reshape(-1, 3)[sel])).all()


def test_trace_restatement_with_emission_sky_and_hook(oracle):
    """One lit sphere: depth 1 gives emission[object] on a hit and the caller's sky on a miss, by hand."""
    recs = RR.three_material_scene()
    emission = np.zeros((recs.shape[0], 3))
    emission[3] = [4.0, 3.0, 2.0]
    rays = np.array([[-4, 1, 5, 0, 0, -1, 0.0], [-4, 1, 5, 0, 1, 0, 0.0], [0, 1, 5, 0, 0, -1, 0.0]], dtype=np.float64)
    st = np.arange(12, dtype=np.uint64).reshape(3, 4) + np.uint64(1)
    seen = []
    color, _ = BR.trace(oracle, recs, rays, st, 1, sky_fn=lambda r, index: np.full((len(index), 3), 0.25), emission=emission,
                        on_bounce=lambda k, index, res: seen.append((k, list(index), BR.H.fields(res["raw"])["object"].tolist())))
    assert color.tolist() == [[4.0, 3.0, 2.0], [0.25, 0.25, 0.25], [0, 0, 0]]
    assert seen == [(0, [0, 1, 2], [3, -1, 1])]
