"""Radiance queries without a GPU: the host seed helpers equal the oracle's seeding, TorRng and the three new entry points are declared,
exported and laid out as a C compiler sees them, every argument check that needs no device answers TOR_ERR_INVALID_ARGUMENT, and
the numpy restatement of radiance() (tests/radiance_restatement.py) -- what the GPU tests hold the kernels to -- is anchored to the
CPU oracle's sample sums, which the reference's PNG pins."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import radiance_restatement as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tor_radiance_device", "tor_radiance_host", "tor_camera_rays_device")
EDGE = [0, 1, 2, 0x7fffffff, 0x80000000, 0xffffffff, 0x100000000, 0x7fffffffffffffff, 0x8000000000000000, 0xffffffffffffffff]


def _err(tor):
    return tor.lib().tor_last_error().decode()


def _oracle_seed(L, fn, *args):
    st = (C.c_uint64 * 4)()
    fn(*args, st)
    return [int(v) for v in st]


def test_rng_seed_helpers_equal_the_oracle(tor, oracle):
    L = oracle.lib()
    rng = np.random.default_rng(7)
    keys = np.concatenate([np.array(EDGE, dtype=np.uint64), rng.integers(0, 2**63, 40, dtype=np.uint64) * np.uint64(2) + np.uint64(1)])
    got1 = tor.rng_seed1(keys)
    assert got1.dtype == np.uint64 and got1.shape == (keys.size, 4)
    for k, row in zip(keys, got1):
        assert [int(v) for v in row] == _oracle_seed(L, L.oracle_rng_seed1, int(k))
    small = np.array(EDGE[:6] + [12345, 1079, 1919], dtype=np.uint64)
    xs, ys = np.meshgrid(small, small, indexing="ij")
    got2 = tor.rng_seed2(xs.reshape(-1), ys.reshape(-1))
    for x, y, row in zip(xs.reshape(-1), ys.reshape(-1), got2):
        assert [int(v) for v in row] == _oracle_seed(L, L.oracle_rng_seed2, int(x), int(y))
    rows, cols, samples = rng.integers(0, 4096, 50), rng.integers(0, 4096, 50), rng.integers(0, 2**31, 50)
    rows[:3], cols[:3], samples[:3] = (0, 2**31 - 1, 7), (0, 2**31 - 1, 0), (0, 2**31 - 1, 2**31 - 1)
    got3 = tor.rng_seed3(rows, cols, samples)
    for r, c, s, row in zip(rows, cols, samples, got3):
        assert [int(v) for v in row] == _oracle_seed(L, L.oracle_rng_seed3, int(r), int(c), int(s))
    # scalars broadcast; negative integers are their two's-complement bits, as the C ABI's uint64_t
    assert (tor.rng_seed3(3, 5, np.arange(4)) == tor.rng_seed3([3] * 4, [5] * 4, [0, 1, 2, 3])).all()
    assert [int(v) for v in tor.rng_seed1(-1)[0]] == _oracle_seed(L, L.oracle_rng_seed1, 2**64 - 1)


def test_new_symbols_are_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in NEW:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
        assert name in tor.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    assert "typedef struct TorRng { uint64_t s0, s1, s2, s3; } TorRng;" in src
    assert C.sizeof(tor.Rng) == 32 and [getattr(tor.Rng, f).offset for f in ("s0", "s1", "s2", "s3")] == [0, 8, 16, 24]
    assert callable(tor.Context.radiance) and callable(tor.Context.camera_rays)
    assert L.tor_version() == b"tor_mi355x 0.6 (gfx950)"


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_c_program_sees_the_layout_and_the_exports(tor, tmp_path):
    prog = tmp_path / "abi.c"
    prog.write_text(r'''
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>
#include "tor_render.h"
_Static_assert(sizeof(TorRng) == 32, "TorRng is 32 bytes");
_Static_assert(offsetof(TorRng, s0) == 0 && offsetof(TorRng, s1) == 8 && offsetof(TorRng, s2) == 16 && offsetof(TorRng, s3) == 24,
               "TorRng field offsets");
_Static_assert(sizeof(TorRay) == 56, "TorRay is 56 bytes");
int main(int argc, char** argv) {
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
  int (*rd)(TorContext*, int64_t, const TorRay*, TorRng*, int32_t, double, double, int32_t, double*, void*) =
      (int (*)(TorContext*, int64_t, const TorRay*, TorRng*, int32_t, double, double, int32_t, double*, void*))dlsym(h, "tor_radiance_device");
  void* rh = dlsym(h, "tor_radiance_host");
  void* cr = dlsym(h, "tor_camera_rays_device");
  if (!rd || !rh || !cr) { fprintf(stderr, "missing export\n"); return 3; }
  printf("%zu %d\n", sizeof(TorRng), rd(NULL, 1, NULL, NULL, 1, 0.0, 1.0, TOR_HIT_AUTO, NULL, NULL));
  return 0;
}
''')
    exe = tmp_path / "abi"
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe), "-ldl"],
                   check=True)
    out = subprocess.run([str(exe), tor.LIB_PATH], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["32", str(tor.ERR_INVALID_ARGUMENT)]


def test_argument_checks_need_no_device(tor):
    L = tor.lib()
    b = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    for fn, extra in ((L.tor_radiance_device, (None,)), (L.tor_radiance_host, ())):
        assert fn(None, 4, b, b, 5, 0.0, 1.0, 0, b, *extra) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
        assert fn(b, -1, b, b, 5, 0.0, 1.0, 0, b, *extra) == tor.ERR_INVALID_ARGUMENT and "n_rays" in _err(tor)
        assert fn(b, 4, b, b, -1, 0.0, 1.0, 0, b, *extra) == tor.ERR_INVALID_ARGUMENT and "max_depth" in _err(tor)
        for lo, hi in ((math.nan, 1.0), (0.0, math.inf), (1.0, 0.5)):
            assert fn(b, 4, b, b, 5, lo, hi, 0, b, *extra) == tor.ERR_INVALID_ARGUMENT and "time range" in _err(tor)
        for mode in (-1, 3):
            assert fn(b, 4, b, b, 5, 0.0, 1.0, mode, b, *extra) == tor.ERR_INVALID_ARGUMENT and "mode" in _err(tor)
        for args in ((None, b, b), (b, None, b), (b, b, None)):
            assert fn(b, 4, args[0], args[1], 5, 0.0, 1.0, 0, args[2], *extra) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
    cam = tor.camera()
    f = L.tor_camera_rays_device
    ok = dict(cam=C.byref(cam), nrows=4, ncols=6, pix=None, n=24, first=0, ns=1, seeding=tor.SEED_SAMPLE, rng=b, rays=b)

    def call(**kw):
        a = dict(ok, **kw)
        return f(b, a["cam"], a["nrows"], a["ncols"], a["pix"], a["n"], a["first"], a["ns"], a["seeding"], a["rng"], a["rays"], None)

    assert f(None, C.byref(cam), 4, 6, None, 24, 0, 1, 1, b, b, None) == tor.ERR_INVALID_ARGUMENT
    assert call(cam=None) == tor.ERR_INVALID_ARGUMENT
    for kw, word in ((dict(nrows=1), "nrows"), (dict(ncols=1), "nrows"), (dict(n=-1, pix=b), "n_pixels"), (dict(n=23), "n_pixels"),
                     (dict(seeding=2), "seeding"), (dict(seeding=tor.SEED_PIXEL, ns=2, n=24), "n_samples"),
                     (dict(first=-1), "first_sample"), (dict(ns=0), "n_samples"), (dict(first=2**31 - 2, ns=2), "first_sample"),
                     (dict(rng=None), "NULL"), (dict(rays=None), "NULL")):
        assert call(**kw) == tor.ERR_INVALID_ARGUMENT, kw
        assert word in _err(tor), (kw, _err(tor))


def test_restatement_on_cases_worked_by_hand(oracle):
    empty = np.zeros((0, 16))
    rays = np.array([[0, 0, 0, 0, 1, 0, 0.3], [0, 0, 0, 0, -3, 0, 0.0], [1, 2, 3, 1, 0, 0, 0.0]], dtype=np.float64)
    st = np.arange(12, dtype=np.uint64).reshape(3, 4) + np.uint64(1)
    color, st2 = RR.radiance(oracle, empty, rays, st, 50)
    # the sky (sic, 0.5 * y + 1.0): straight up t = 1.5, straight down t = 0.5, horizontal t = 1.0; no draws
    assert color.tolist() == [[1.0 * (1.0 - t) + a * t for a in (0.5, 0.7, 1.0)] for t in (1.5, 0.5, 1.0)]
    assert color[0, 0] == 0.25 and color[1, 2] == 1.0
    assert (st2 == st).all()
    color, st3 = RR.radiance(oracle, RR.three_material_scene(), rays, st, 0)
    assert (color == 0).all() and (st3 == st).all()


@pytest.mark.parametrize("depth", [1, 2, 50])
@pytest.mark.parametrize("scene", ["random", "three"])
def test_restatement_matches_the_oracle_sample_sums(oracle, ref_scene, ref_camera, scene, depth):
    """Camera rays with their post-draw states through the restatement, quantised and summed per pixel, equal oracle.accumulate's
    sums and moments bit for bit."""
    recs = ref_scene[0] if scene == "random" else RR.three_material_scene()
    cam = ref_camera if scene == "random" else oracle.camera(look_from=(0, 2, 9), look_at=(0, 0.8, 0), vfov=40.0)
    nrows, ncols, first, ns = 9, 16, 3, 2
    pixels = np.arange(nrows * ncols)[::2] if scene == "random" else None
    rays, st = RR.camera_rays(oracle, cam, nrows, ncols, pixels, first, ns)
    color, _ = RR.radiance(oracle, recs, rays, st, depth)
    n_pix = nrows * ncols // 2 if scene == "random" else nrows * ncols
    s, m = RR.sums_and_moments(color, n_pix, ns)
    want_s, want_m = oracle.accumulate(nrows, ncols, first, ns, cam, recs, max_depth=depth, pixels=pixels)
    sel = pixels if pixels is not None else np.arange(nrows * ncols)
    assert (s.view(np.uint64) == want_s.reshape(-1, 3)[sel].view(np.uint64)).all()
    assert (m.view(np.uint64) == want_m.reshape(-1, 3)[sel].view(np.uint64)).all()
    # the numpy rounding is the oracle's
    L = oracle.lib()
    flat = color.reshape(-1)[:64]
    assert [L.oracle_quantize36(float(x)) for x in flat] == RR.quantize36(flat).tolist()
