"""Progressive rendering without a GPU: the three entry points are declared and exported, the Python layer binds them,
and every argument check that needs no device answers TOR_ERR_INVALID_ARGUMENT."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tor_render_accumulate_device", "tor_resolve_device", "tor_accum_noise_device")


def test_new_symbols_are_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    L = tor.lib()
    for name in NEW:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_render.h"
        assert name in tor.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    for meth in ("accumulate_device", "resolve_device", "accum_noise_device"):
        assert callable(getattr(tor.Context, meth))
    for meth in ("add", "image", "to_canvas", "noise", "state", "from_state", "render_until"):
        assert callable(getattr(tor.Progressive, meth))
    assert L.tor_version() != b"tor_mi355x 0.4 (gfx950)"


def _err(tor):
    return tor.lib().tor_last_error().decode()


def test_accumulate_rejects_bad_ranges_and_null_arguments(tor):
    L, cam, opt = tor.lib(), tor.camera(), tor.make_options(seeding=tor.SEED_SAMPLE)
    buf = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    for first, n in ((-1, 4), (0, 0), (0, -3), (1 << 17, 1), ((1 << 17) - 4, 5), (0, (1 << 17) + 1)):
        rc = L.tor_render_accumulate_device(None, C.byref(cam), 8, 8, first, n, 50, C.byref(opt), buf, None, None)
        assert rc == tor.ERR_INVALID_ARGUMENT, (first, n)
        assert "2^17" in _err(tor)
    rc = L.tor_render_accumulate_device(None, C.byref(cam), 8, 8, 0, 4, 50, C.byref(opt), buf, None, None)
    assert rc == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)


def test_resolve_and_noise_reject_without_a_device(tor):
    L = tor.lib()
    buf = C.c_void_p(16)
    out = (C.c_double * 2)()
    assert L.tor_resolve_device(None, buf, 12, 4, 2.2, buf, None) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
    for total in (0, (1 << 17) + 1):
        assert L.tor_resolve_device(None, buf, 12, total, 2.2, buf, None) == tor.ERR_INVALID_ARGUMENT
    assert L.tor_accum_noise_device(None, buf, buf, 4, 8, None, out, None) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
    for npix, total in ((4, 1), (4, 0), (0, 8), (4, (1 << 17) + 1)):
        assert L.tor_accum_noise_device(None, buf, buf, npix, total, None, out, None) == tor.ERR_INVALID_ARGUMENT, (npix, total)
    L.tor_accum_noise_device(None, buf, buf, 4, 1, None, out, None)
    assert "two samples" in _err(tor)


def test_context_methods_raise_on_a_null_context(tor):
    ctx = object.__new__(tor.Context)  # a context whose creation never happened (no device here)
    ctx._h = C.c_void_p()
    cam, opt = tor.camera(), tor.make_options(seeding=tor.SEED_SAMPLE)
    with pytest.raises(tor.TorError) as e:
        ctx.accumulate_device(cam, 8, 8, 0, 4, 50, opt, 0)
    assert e.value.code == tor.ERR_INVALID_ARGUMENT
    with pytest.raises(tor.TorError) as e:
        ctx.resolve_device(0, 12, 4, 2.2, 0)
    assert e.value.code == tor.ERR_INVALID_ARGUMENT
    with pytest.raises(tor.TorError) as e:
        ctx.accum_noise_device(0, 0, 4, 8)
    assert e.value.code == tor.ERR_INVALID_ARGUMENT


def test_progressive_refuses_pixel_seeding(tor):
    with pytest.raises(tor.TorError) as e:
        tor.Progressive(None, tor.camera(), 8, 8, 50, tor.make_options(seeding=tor.SEED_PIXEL))
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "SEED_SAMPLE" in str(e.value)
