"""Resumable rendering on the reference's per-pixel streams without a GPU: tor_render_resume_device is declared, exported and bound,
every argument check that needs no device answers TOR_ERR_INVALID_ARGUMENT, PixelProgressive refuses sample streams and checks the
shapes of a checkpoint, and the documents speak of the entry."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tor_render_resume_device"


def _err(tor):
    return tor.lib().tor_last_error().decode()


def test_symbol_is_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    assert re.search(r"TOR_API\s+int\s+" + NAME + r"\s*\(", src), f"{NAME} is not declared in tor_render.h"
    assert NAME in tor.EXPORTED_SYMBOLS
    assert len(getattr(tor.lib(), NAME).argtypes) == 12
    assert callable(tor.Context.resume_device)
    for meth in ("add", "image", "to_canvas", "noise", "state", "from_state", "render_until"):
        assert callable(getattr(tor.PixelProgressive, meth))
    # tor_debug_last_variant's comment names the new kernel variants
    doc = src[:src.index("TOR_API int tor_debug_last_variant")]
    doc = doc[doc.rindex("/*"):]
    assert "5 (resumable pixel streams)" in doc and "6 (" in doc


def test_split_accessor_is_declared_exported_and_checks_its_arguments(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    assert re.search(r"TOR_API\s+int\s+tor_debug_last_split_tiles\s*\(", src)
    assert "tor_debug_last_split_tiles" in tor.EXPORTED_SYMBOLS and callable(tor.Context.last_split_tiles)
    out = C.c_int64(7)
    assert tor.lib().tor_debug_last_split_tiles(None, C.byref(out)) == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)
    assert out.value == 7


def test_resume_rejects_bad_ranges_and_null_arguments(tor):
    L, cam, opt = tor.lib(), tor.camera(), tor.make_options(seeding=tor.SEED_PIXEL)
    buf = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    for first, n in ((-1, 4), (0, 0), (0, -3), (1 << 17, 1), ((1 << 17) - 4, 5), (0, (1 << 17) + 1)):
        rc = L.tor_render_resume_device(None, C.byref(cam), 8, 8, first, n, 50, C.byref(opt), buf, buf, None, None)
        assert rc == tor.ERR_INVALID_ARGUMENT, (first, n)
        # not an exactness bound in this mode: the message says whose range it is
        assert "2^17" in _err(tor) and "tor_resolve_device" in _err(tor) and "tor_accum_noise_device" in _err(tor)
    for args in ((None, C.byref(cam), buf, buf), ):
        rc = L.tor_render_resume_device(args[0], args[1], 8, 8, 0, 4, 50, C.byref(opt), args[2], args[3], None, None)
        assert rc == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor) and NAME in _err(tor)


def test_context_method_raises_on_a_null_context(tor):
    ctx = object.__new__(tor.Context)  # a context whose creation never happened (no device here)
    ctx._h = C.c_void_p()
    with pytest.raises(tor.TorError) as e:
        ctx.resume_device(tor.camera(), 8, 8, 0, 4, 50, tor.make_options(seeding=tor.SEED_PIXEL), 0, 0)
    assert e.value.code == tor.ERR_INVALID_ARGUMENT


def test_pixel_progressive_refuses_sample_seeding_and_progressive_still_refuses_pixel_seeding(tor):
    with pytest.raises(tor.TorError) as e:
        tor.PixelProgressive(None, tor.camera(), 8, 8, 50, tor.make_options(seeding=tor.SEED_SAMPLE))
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "SEED_PIXEL" in str(e.value) and "Progressive" in str(e.value)
    with pytest.raises(tor.TorError) as e:
        tor.Progressive(None, tor.camera(), 8, 8, 50, tor.make_options(seeding=tor.SEED_PIXEL))
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "SEED_SAMPLE" in str(e.value)


def test_default_options_and_checkpoint_shapes(tor):
    cam = tor.camera()
    pp = tor.PixelProgressive(None, cam, 9, 8, 50, moments=True, device="cpu")
    assert pp.options.seeding == tor.SEED_PIXEL and pp.options.accel == (tor.ACCEL_BLOCKS | tor.ACCEL_F32)
    st = pp.state()
    assert st["samples"] == 0 and st["sums"].shape == (9, 8, 3) and st["moments"].shape == (9, 8, 3)
    assert st["rng"].shape == (9, 8, 4) and st["rng"].dtype == np.uint64
    # a row shard keeps its own rows only
    shard = tor.PixelProgressive(None, cam, 9, 8, 50, tor.make_options(seeding=tor.SEED_PIXEL, shard_index=1, shard_count=2, row_tile=2), device="cpu")
    assert shard.state()["rng"].shape == (len(tor.shard_rows(9, 2, 1, 2)), 8, 4) and shard.state()["moments"] is None
    # a round trip keeps every bit, the top one of a state word included
    st["rng"][...] = np.uint64(0xF123456789ABCDEF)
    st["sums"][...] = 1.5
    st["moments"][...] = 2.5
    st["samples"] = 7
    back = tor.PixelProgressive.from_state(None, cam, 9, 8, 50, None, st, device="cpu")
    again = back.state()
    assert again["samples"] == 7 and np.array_equal(again["rng"], st["rng"]) and np.array_equal(again["sums"], st["sums"])
    assert np.array_equal(again["moments"], st["moments"])
    for key, bad in (("rng", np.zeros((9, 8, 3), dtype=np.uint64)), ("rng", np.zeros((9, 8, 4), dtype=np.int64)), ("rng", None),
                     ("sums", np.zeros((9, 8, 4))), ("moments", np.zeros((8, 9, 3)))):
        broken = dict(st)
        broken[key] = bad
        with pytest.raises(tor.TorError) as e:
            tor.PixelProgressive.from_state(None, cam, 9, 8, 50, None, broken, device="cpu")
        assert e.value.code == tor.ERR_INVALID_ARGUMENT, key


def test_documents_mention_the_entry():
    for doc, words in (("README.md", (NAME, "PixelProgressive")), ("INTEGRATION.md", (NAME, "TorRng")), ("DESIGN.md", (NAME, "hand-off")),
                       (os.path.join("include", "tor_render.h"), (NAME, "tor_render_accumulate_device", "render.nim:63-65"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)


def test_knob_document_still_matches_the_table():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_knob_doc.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
