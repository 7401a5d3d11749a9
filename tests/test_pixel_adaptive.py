"""Adaptive sampling on the reference's per-pixel streams without a GPU: tor_render_resume_list_device is declared, exported and
bound, every argument check that needs no device answers TOR_ERR_INVALID_ARGUMENT, PixelAdaptive refuses sample streams (and Adaptive
still refuses the pixel streams), checks the arrays of a checkpoint, and the documents speak of the entry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tor_render_resume_list_device"


def _err(tor):
    return tor.lib().tor_last_error().decode()


def test_symbol_is_declared_exported_and_bound(tor):
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    assert re.search(r"TOR_API\s+int\s+" + NAME + r"\s*\(", src), f"{NAME} is not declared in tor_render.h"
    assert NAME in tor.EXPORTED_SYMBOLS
    assert len(getattr(tor.lib(), NAME).argtypes) == 14
    assert callable(tor.Context.resume_list_device)
    for meth in ("step", "run", "counts", "active_list", "total_samples", "image", "to_canvas", "state", "from_state", "validate_list"):
        assert callable(getattr(tor.PixelAdaptive, meth)), meth
    assert issubclass(tor.PixelAdaptive, tor.Adaptive)
    # tor_debug_last_variant's comment names the new kernel variant, and the version did not move
    doc = src[:src.index("TOR_API int tor_debug_last_variant")]
    doc = doc[doc.rindex("/*"):]
    assert "7 (" in doc and NAME in doc
    assert tor.lib().tor_version() == b"tor_mi355x 0.6 (gfx950)"


def test_rejections_that_need_no_device(tor):
    L, cam, opt = tor.lib(), tor.camera(), tor.make_options(seeding=tor.SEED_PIXEL)
    buf = C.c_void_p(16)  # never dereferenced: every call below fails its checks first
    fn = L.tor_render_resume_list_device
    for first, n in ((-1, 4), (0, 0), (0, -3), (1 << 17, 1), ((1 << 17) - 4, 5), (0, (1 << 17) + 1)):
        rc = fn(None, C.byref(cam), 8, 8, buf, 4, first, n, 50, C.byref(opt), buf, buf, buf, None)
        assert rc == tor.ERR_INVALID_ARGUMENT and "2^17" in _err(tor) and NAME in _err(tor), (first, n)
    rc = fn(None, C.byref(cam), 8, 8, buf, -1, 0, 4, 50, C.byref(opt), buf, buf, buf, None)
    assert rc == tor.ERR_INVALID_ARGUMENT and "n_list" in _err(tor)
    rc = fn(None, C.byref(cam), 8, 8, buf, 65, 0, 4, 50, C.byref(opt), buf, buf, buf, None)
    assert rc == tor.ERR_INVALID_ARGUMENT and "above the shard's 64 pixels" in _err(tor)
    shard = tor.make_options(seeding=tor.SEED_PIXEL, shard_index=1, shard_count=2, row_tile=1)  # rows 1, 3, 5, 7: 32 pixels
    rc = fn(None, C.byref(cam), 8, 8, buf, 33, 0, 4, 50, C.byref(shard), buf, buf, buf, None)
    assert rc == tor.ERR_INVALID_ARGUMENT and "above the shard's 32 pixels" in _err(tor)
    # ctx, cam, list (with n_list > 0), generator states, sums, moments
    for k in range(6):
        a = [buf, C.byref(cam), buf, buf, buf, buf]
        a[k] = None
        rc = fn(a[0], a[1], 8, 8, a[2], 4, 0, 4, 50, C.byref(opt), a[3], a[4], a[5], None)
        assert rc == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor) and NAME in _err(tor), k
    # an empty list may come without a pointer, but not without a context
    rc = fn(None, C.byref(cam), 8, 8, None, 0, 0, 4, 50, C.byref(opt), buf, buf, buf, None)
    assert rc == tor.ERR_INVALID_ARGUMENT and "NULL" in _err(tor)


def test_context_method_raises_on_a_null_context(tor):
    ctx = object.__new__(tor.Context)  # a context whose creation never happened (no device here)
    ctx._h = C.c_void_p()
    with pytest.raises(tor.TorError) as e:
        ctx.resume_list_device(tor.camera(), 8, 8, 16, 4, 0, 4, 50, tor.make_options(seeding=tor.SEED_PIXEL), 16, 16, 16)
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "NULL" in str(e.value)


def test_pixel_adaptive_refuses_sample_seeding_and_adaptive_still_refuses_pixel_seeding(tor):
    with pytest.raises(tor.TorError) as e:
        tor.PixelAdaptive(None, tor.camera(), 8, 8, 50, tor.make_options(seeding=tor.SEED_SAMPLE))
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "SEED_PIXEL" in str(e.value) and "Adaptive's" in str(e.value)
    with pytest.raises(tor.TorError) as e:
        tor.Adaptive(None, tor.camera(), 8, 8, 50, tor.make_options(seeding=tor.SEED_PIXEL))
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "SEED_SAMPLE" in str(e.value) and "PixelAdaptive" in str(e.value)
    assert "cannot be resumed" not in str(e.value)
    for kw in ({"abs_tol": -1.0}, {"rel_tol": float("nan")}, {"min_samples": 1}, {"pass_samples": 0}, {"max_samples": (1 << 17) + 1}):
        with pytest.raises(tor.TorError) as e:
            tor.PixelAdaptive(None, tor.camera(), 8, 8, 50, **kw)
        assert e.value.code == tor.ERR_INVALID_ARGUMENT and "PixelAdaptive" in str(e.value), kw


def test_default_options_and_checkpoint_shapes(tor):
    cam = tor.camera()
    ad = tor.PixelAdaptive(None, cam, 9, 8, 50, device="cpu")
    assert ad.options.seeding == tor.SEED_PIXEL and ad.options.accel == (tor.ACCEL_BLOCKS | tor.ACCEL_F32)
    assert ad.active == 72 and ad.active_list().tolist() == list(range(72)) and ad.total_samples() == 0
    st = ad.state()
    assert set(st) == {"samples", "sums", "moments", "counts", "list", "rng"}
    assert st["samples"] == 0 and st["sums"].shape == (9, 8, 3) and st["moments"].shape == (9, 8, 3)
    assert st["sums"].dtype == np.float64 and st["moments"].dtype == np.float64
    assert st["counts"].shape == (9, 8) and st["counts"].dtype == np.int32
    assert st["list"].shape == (72,) and st["list"].dtype == np.int32
    assert st["rng"].shape == (9, 8, 4) and st["rng"].dtype == np.uint64
    # a row shard keeps its own rows only
    sopt = tor.make_options(seeding=tor.SEED_PIXEL, shard_index=1, shard_count=2, row_tile=2)
    shard = tor.PixelAdaptive(None, cam, 9, 8, 50, sopt, device="cpu")
    rows = len(tor.shard_rows(9, 2, 1, 2))
    assert shard.state()["rng"].shape == (rows, 8, 4) and shard.state()["list"].size == rows * 8
    # Adaptive's own checkpoint has no generator states
    assert "rng" not in tor.Adaptive(None, cam, 9, 8, 50, device="cpu").state()
    # a round trip keeps every bit, the top one of a state word included
    st["rng"][...] = np.uint64(0xF123456789ABCDEF)
    st["sums"][...] = 1.5
    st["moments"][...] = 2.5
    st["samples"] = 16
    st["counts"][...] = 8
    st["list"] = np.array([3, 17, 40], dtype=np.int32)
    st["counts"].reshape(-1)[st["list"]] = 16
    back = tor.PixelAdaptive.from_state(None, cam, 9, 8, 50, None, st, device="cpu", rel_tol=0.1, max_samples=64)
    again = back.state()
    assert again["samples"] == 16 and back.active == 3 and back.rel_tol == 0.1 and back.max_samples == 64
    for key in ("rng", "sums", "moments", "counts", "list"):
        assert np.array_equal(again[key], st[key]) and again[key].dtype == st[key].dtype, key


def test_from_state_refuses_bad_lists_and_generator_states(tor):
    cam = tor.camera()
    st = tor.PixelAdaptive(None, cam, 9, 8, 50, device="cpu").state()
    st["samples"] = 16
    st["counts"][...] = 16
    good = tor.PixelAdaptive.from_state(None, cam, 9, 8, 50, None, st, device="cpu")
    assert good.active == 72 and good.samples == 16
    # a listed pixel that does not hold N samples
    broken = dict(st)
    broken["counts"] = st["counts"].copy()
    broken["counts"][2, 3] = 8
    with pytest.raises(tor.TorError) as e:
        tor.PixelAdaptive.from_state(None, cam, 9, 8, 50, None, broken, device="cpu")
    assert e.value.code == tor.ERR_INVALID_ARGUMENT and "exactly N samples" in str(e.value) and "PixelAdaptive" in str(e.value)
    # ... is fine once it is off the list
    broken["list"] = np.delete(st["list"], 2 * 8 + 3)
    assert tor.PixelAdaptive.from_state(None, cam, 9, 8, 50, None, broken, device="cpu").active == 71
    for bad in ([3, 2, 5], [1, 4, 4, 9], [-1, 3], [0, 72]):
        broken = dict(st)
        broken["list"] = np.array(bad)
        with pytest.raises(tor.TorError) as e:
            tor.PixelAdaptive.from_state(None, cam, 9, 8, 50, None, broken, device="cpu")
        assert e.value.code == tor.ERR_INVALID_ARGUMENT, bad
    for key, bad in (("rng", np.zeros((9, 8, 3), dtype=np.uint64)), ("rng", np.zeros((9, 8, 4), dtype=np.int64)), ("rng", None),
                     ("rng", np.zeros((8, 9, 4), dtype=np.uint64)), ("sums", np.zeros((9, 8, 4))), ("moments", np.zeros((8, 9, 3))),
                     ("counts", np.zeros((9, 9), dtype=np.int32))):
        broken = dict(st)
        broken[key] = bad
        with pytest.raises(tor.TorError) as e:
            tor.PixelAdaptive.from_state(None, cam, 9, 8, 50, None, broken, device="cpu")
        assert e.value.code == tor.ERR_INVALID_ARGUMENT, key
    # a checkpoint without generator states (Adaptive's) is refused before anything else happens
    plain = {k: v for k, v in st.items() if k != "rng"}
    with pytest.raises(tor.TorError) as e:
        tor.PixelAdaptive.from_state(None, cam, 9, 8, 50, None, plain, device="cpu")
    assert "generator states" in str(e.value)


def test_documents_mention_the_entry():
    for doc, words in (("README.md", (NAME, "PixelAdaptive")), ("INTEGRATION.md", (NAME, "PixelAdaptive")),
                       ("DESIGN.md", (NAME, "TOR_COOP_MAX_PIXELS", "probe")), (os.path.join("tools", "README.md"), ("pixel_adaptive_rate.py",)),
                       (os.path.join("include", "tor_render.h"), (NAME, "tor_resolve_counts_device", "seeding 7", "TOR_COOP_MAX_PIXELS"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
    # the sample-mode list entry no longer sends TOR_SEED_PIXEL callers nowhere
    src = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    block = src[src.index(" * tor_render_accumulate_list_device:"):src.index(" * tor_adaptive_select_device:")]
    assert NAME in block
