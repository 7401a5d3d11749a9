"""Planar patch queries on the CPU (include/tor_patches.h): the numpy restatement (tests/patch_restatement.py) against hand-worked
rows, the order-independence of its winner, the any-hit bit against the closest hit, the merge against "closest of both", each of its
variants told apart by a named case of tests/patch_inputs.py; the C ABI as declared, bound and built; the refusals that need no
device; and the Python glue on a recording stand-in for the library.  tests/test_gpu_patch_query.py holds the library to the
restatement bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hit_restatement as H
import patch_inputs as I
import patch_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_inputs_do_what_their_names_say():
    assert I.NAMES == ["one_quad", "one_triangle", "parallel", "range", "default_range", "ties", "ties_range", "materials", "masks",
                       "mask_scalar", "mask_zero", "overflow", "soup9", "soup63", "soup64", "soup65", "soup130", "room"]
    I.assert_coverage()


# ---- hand-worked rows -------------------------------------------------------------------------------------------------------------------

def _one(patch, o, d, **kw):
    got = R.hit([patch], I.rays_of([o], [d]), **kw)
    f = H.fields(got["raw"])
    return (int(got["patch"][0]), float(f["t"][0]), tuple(f["p"][0]), tuple(f["normal"][0]), int(f["object"][0]), int(f["front_face"][0]),
            tuple(got["uv"][0]))


def test_b_a_unit_quad_by_hand():
    """q = 0, u = x, v = z; the ray from (0.25, 2, 0.5) straight down.  pv = cross(d, v) = (-1, 0, 0), det = u . pv = -1;
    tv = (0.25, 2, 0.5), an = -0.25; qv = cross(tv, u) = (0, 0.5, -2), bn = d . qv = -0.5, tn = v . qv = -2.  det < 0 flips all
    four: det 1, an 0.25, bn 0.5, tn 2, so t = 2, p = (0.25, 0, 0.5), uv = (0.25, 0.5).  n = cross(u, v) = (0, -1, 0) = N;
    d . N = 1 is not < 0: the back face, normal = -N = (-0, 1, -0).  From below the same point is the front face, normal N."""
    quad = R.quad((0, 0, 0), (1, 0, 0), (0, 0, 1), material=7)
    got = _one(quad, (0.25, 2.0, 0.5), (0.0, -1.0, 0.0))
    assert got == (0, 2.0, (0.25, 0.0, 0.5), (0.0, 1.0, 0.0), 7, 0, (0.25, 0.5))
    assert np.signbit(got[3][0]) and np.signbit(got[3][2])                       # -N, component by component
    assert _one(quad, (0.25, -2.0, 0.5), (0.0, 1.0, 0.0)) == (0, 2.0, (0.25, 0.0, 0.5), (0.0, -1.0, 0.0), 7, 1, (0.25, 0.5))
    assert _one(quad, (0.25, -4.0, 0.5), (0.0, 2.0, 0.0))[1] == 2.0              # t is in units of d
    assert _one(quad, (1.25, 2.0, 0.5), (0.0, -1.0, 0.0)) == (-1, 0.0, (0.0,) * 3, (0.0,) * 3, -1, 0, (0.0, 0.0))   # the miss record
    assert _one(quad, (1.0, 2.0, 1.0), (0.0, -1.0, 0.0))[0] == 0 and _one(quad, (0.0, 2.0, 0.0), (0.0, -1.0, 0.0))[6] == (0.0, 0.0)


def test_b_a_unit_triangle_by_hand():
    """The same ray against the triangle (0, 0, 0), (1, 0, 0), (0, 0, 1): an + bn = 0.75 <= det = 1, the same record; at
    (0.75, ., 0.5) the sum is 1.25: outside the triangle and inside the quad; at (0.5, ., 0.5) the sum is det exactly: on the
    edge, a hit."""
    tri = R.triangle((0, 0, 0), (1, 0, 0), (0, 0, 1), material=3)
    assert _one(tri, (0.25, 2.0, 0.5), (0.0, -1.0, 0.0)) == (0, 2.0, (0.25, 0.0, 0.5), (0.0, 1.0, 0.0), 3, 0, (0.25, 0.5))
    assert _one(tri, (0.75, 2.0, 0.5), (0.0, -1.0, 0.0))[0] == -1
    assert _one(R.quad((0, 0, 0), (1, 0, 0), (0, 0, 1)), (0.75, 2.0, 0.5), (0.0, -1.0, 0.0))[0] == 0
    assert _one(tri, (0.5, 2.0, 0.5), (0.0, -1.0, 0.0))[6] == (0.5, 0.5)
    assert R.triangle((1, 2, 3), (2, 2, 3), (1, 2, 5))["u"].tolist() == [1.0, 0.0, 0.0]


def test_b_a_slanted_ray_and_a_scaled_normal_by_hand():
    """u = (0, 3, 0), v = (0, 0, 4): n = (12, 0, 0), nn = 144, N = n * (1 / 12) -- (1, 0, 0) up to the rounding of 1 / 12 * 12.
    The ray from (5, 1, 1) along (-1, 0.5, 0.25) meets x = 0 at t = 5 in p = (0, 3.5, 2.25): a = 3.5 / 3 > 1, a miss.  Along
    (-1, 0.25, 0.25) it is p = (0, 2.25, 2.25): a = 0.75, b = 0.5625, and d . N < 0: the front face, normal N."""
    quad = R.quad((0, 0, 0), (0, 3, 0), (0, 0, 4), material=-1)
    assert _one(quad, (5.0, 1.0, 1.0), (-1.0, 0.5, 0.25))[0] == -1
    got = _one(quad, (5.0, 1.0, 1.0), (-1.0, 0.25, 0.25))
    inv = 1.0 / np.sqrt(144.0)
    assert got[:3] == (0, 5.0, (0.0, 2.25, 2.25)) and got[3] == (12.0 * inv, 0.0, 0.0) and got[4:] == (-1, 1, (0.75, 0.5625))


# ---- properties ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup9", "soup63", "soup64", "soup65", "soup130", "ties", "room"])
def test_c_the_winner_does_not_depend_on_the_visiting_order(name):
    """Any permutation of the table gives the same winner (through the permutation) and the same record, but for the rays whose two
    best patches tie in t: there the LOWER INDEX wins, which a permutation changes -- those rays are told by the tie_high_index
    variant answering differently."""
    c = I.BY_NAME[name]
    args = (c["rays"], c["t_range"], c["mask"])
    a, hi = R.hit(c["table"], *args), R.hit(c["table"], *args, variant="tie_high_index")
    tied = a["patch"] != hi["patch"]
    assert tied.any() == (name == "ties")
    perm = np.random.default_rng(3).permutation(len(c["table"]))
    b = R.hit([c["table"][j] for j in perm], *args)
    back = np.where(b["patch"] >= 0, perm[np.clip(b["patch"], 0, None)], -1)
    keep = ~tied
    assert np.array_equal(back[keep], a["patch"][keep])
    assert not R.mismatches({k: v[keep] for k, v in b.items() if k != "patch"} | {"patch": back[keep]}, {k: v[keep] for k, v in a.items()})
    if name == "ties":                                                           # a tie's record differs in the material alone
        assert np.array_equal(H.fields(a["raw"])["t"], H.fields(b["raw"])["t"])


@pytest.mark.parametrize("name", I.NAMES)
def test_c_occluded_is_some_patch_is_hit(name):
    a = I.answer(name)
    assert np.array_equal(a["occluded"] != 0, a["hit"]["patch"] >= 0)
    c = I.BY_NAME[name]
    n = c["rays"].shape[0]
    for tr in ((0.0, 1.0), (1.0, 3.0), (-5.0, 0.5)):                             # and over other ranges
        t_range = np.tile(np.array(tr), (n, 1))
        assert np.array_equal(R.occluded(c["table"], c["rays"], t_range, c["mask"]) != 0, R.hit(c["table"], c["rays"], t_range, c["mask"])["patch"] >= 0)
    ones = np.ones(n, dtype=np.int32)
    assert np.array_equal(R.occluded(c["table"], c["rays"], c["t_range"], c["mask"], merge=ones), ones)      # an OR never clears a bit
    assert np.array_equal(R.occluded(c["table"], c["rays"], c["t_range"], c["mask"], merge=0 * ones), a["occluded"])


@pytest.mark.parametrize("name", ["soup9", "soup63", "soup130", "room", "one_quad"])
def test_c_merge_is_the_closest_of_spheres_and_patches_spheres_first(name):
    c = I.BY_NAME[name]
    recs = I.ROOM_SPHERES if name == "room" else I.SPHERES
    got, want = R.merge(recs, c["table"], c["rays"], c["t_range"]), R.closest_of_both(recs, c["table"], c["rays"], c["t_range"])
    assert not R.mismatches(got, want)
    if name != "one_quad":
        obj = H.fields(got["raw"])["object"]
        assert ((got["patch"] < 0) & (obj >= 0)).any() and (got["patch"] >= 0).any()      # both kinds of geometry win somewhere


# ---- the variants -----------------------------------------------------------------------------------------------------------------------

TOLD_APART_BY = {"edges_exclusive": "one_quad", "tie_high_index": "ties", "range_inclusive": "range", "merge_tie_to_patch": "ties",
                 "one_sided": "one_quad", "triangle_as_quad": "one_triangle", "triangle_sum_before_flip": "one_triangle",
                 "normal_not_flipped": "materials", "groups_ignored": "masks", "record_t_ignored": "ties", "default_range_zero": "default_range"}


def differing_cases(variant):
    out = []
    for name in I.NAMES:
        got, want = I.answer(name, variant), I.answer(name)
        if any(R.mismatches(got[k], want[k]) for k in want):
            out.append(name)
    return out


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_e_each_variant_is_told_apart_by_a_named_case(variant):
    """Every wrong reading of the header changes at least one output bit of at least one named case (profiles/patch_mutants.txt is
    this table)."""
    assert sorted(TOLD_APART_BY) == sorted(R.VARIANTS) and len(R.VARIANTS) == 11
    seen = differing_cases(variant)
    print(f"{variant:26s} {' '.join(seen)}")
    assert TOLD_APART_BY[variant] in seen


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------

def test_f_the_entries_are_declared_bound_and_built(tor):
    src = open(os.path.join(ROOT, "include", "tor_patches.h")).read()
    render = open(os.path.join(ROOT, "include", "tor_render.h")).read()
    assert render.index('#include "tor_texture.h"') < render.index('#include "tor_patches.h"')
    L = tor.lib()
    assert tor.PATCH_SYMBOLS == ["tor_scene_patches", "tor_patch_info", "tor_patch_hit_device", "tor_patch_hit_host",
                                 "tor_patch_occluded_device", "tor_patch_occluded_host"]
    for name in tor.PATCH_SYMBOLS:
        assert re.search(r"TOR_API\s+int\s+" + name + r"\s*\(", src), f"{name} is not declared in tor_patches.h"
        assert hasattr(L, name) and getattr(L, name).argtypes == tor._patch_signatures()[name]
        assert name not in tor.EXPORTED_SYMBOLS and name not in tor._signatures() and name not in tor.TEXTURE_SYMBOLS
    assert sorted(tor.PATCH_SYMBOLS) == sorted(set(re.findall(r"TOR_API\s+int\s+(tor_\w+)\s*\(", src))) == sorted(tor._PATCH_SIGNATURES)
    # the declared parameter counts are the bound ones
    for name in tor.PATCH_SYMBOLS:
        params = re.search(r"TOR_API\s+int\s+" + name + r"\s*\(([^;]*)\);", src).group(1)
        assert params.count(",") + 1 == len(tor._PATCH_SIGNATURES[name]), name
    assert re.search(r"TOR_PATCH_QUAD = 0, TOR_PATCH_TRIANGLE = 1", src) and re.search(r"TOR_PATCH_MAX = 16384", src)
    assert (tor.PATCH_QUAD, tor.PATCH_TRIANGLE, tor.PATCH_MAX) == (R.QUAD, R.TRIANGLE, R.PATCH_MAX) == (0, 1, 16384)
    P = tor.PatchRecord
    assert C.sizeof(P) == 88 and (P.kind.offset, P.material.offset, P.groups.offset, P.q.offset, P.u.offset, P.v.offset) == (0, 4, 8, 16, 40, 64)
    for name in ("set_patches", "patches", "hit_patches", "occluded_patches", "trace_patches"):
        assert callable(getattr(tor.Context, name))
    mk = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "Makefile")).read()
    assert mk.count("tor_patches.hip") == 2 and mk.count("tor_patches.h ") == 1      # SRCS and ASM_SRCS; HDRS
    assert "-ffp-contract=off" in mk
    for word in ("88 bytes", "THE WINNER", "gives the same winner", "NOT WATERTIGHT", "IN BOUNDS", "rounded once", "both strict"):
        assert word in src, word
    hip = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "tor_patches.hip")).read()
    assert "sizeof(TorPatch) == 88" in hip
    hip = hip.split("#include <hip/hip_runtime.h>")[1]
    assert "__shared__" not in hip and "atomic" not in hip and "listed_ray" in hip and "address_space" not in hip and "qcdptr" in hip
    api = open(os.path.join(ROOT, "trace-of-radiance_amd", "csrc", "tor_api.cpp")).read()
    assert "patches_scene_replaced(ctx)" in api and "patches_context_destroyed(ctx)" in api


def test_f_refusals_that_need_no_device(tor):
    """The checks that come before any device work, in the header's order; nothing is written.  (None of them reads the context, so a
    non-NULL pointer stands in for one; those that do -- no scene, no table, the table's own -- are in the GPU suite.)"""
    L = tor.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.cast((C.c_char * 64)(), C.c_void_p)
    err = lambda: L.tor_last_error().decode()
    assert L.tor_scene_patches(None, 1, p) == -1 and "tor_scene_patches: ctx is NULL" in err()
    assert L.tor_patch_info(None, p) == -1 and "tor_patch_info: NULL argument" in err()
    assert L.tor_patch_info(ctx, None) == -1 and "NULL argument" in err()
    hit = lambda f, tail: (lambda c, n, rays, lst, nl, hits, patch: f(c, n, rays, None, lst, nl, 0, hits, patch, None, *tail, None, 0xFFFFFFFF))
    occ = lambda f, tail: (lambda c, n, rays, lst, nl, out, _unused: f(c, n, rays, None, lst, nl, 1, out, *tail, None, 0xFFFFFFFF))
    for f, name, what in ((hit(L.tor_patch_hit_device, (None,)), "tor_patch_hit_device", "NULL rays, hits or patch"),
                          (hit(L.tor_patch_hit_host, ()), "tor_patch_hit_host", "NULL rays, hits or patch"),
                          (occ(L.tor_patch_occluded_device, (None,)), "tor_patch_occluded_device", "NULL rays or occluded"),
                          (occ(L.tor_patch_occluded_host, ()), "tor_patch_occluded_host", "NULL rays or occluded")):
        assert f(None, 1, p, None, 1, p, p) == -1 and name in err() and "ctx is NULL" in err()
        assert f(ctx, -1, None, None, -1, None, None) == -1 and "n_rays < 0" in err()      # a later fault in every call: the earlier one is reported
        assert f(ctx, 1, None, None, -1, None, None) == -1 and "n_list < 0" in err()
        assert f(ctx, 2, None, None, 1, None, None) == -1 and "without a list" in err()
        assert f(ctx, 1, None, None, 1, p, p) == -1 and what in err()
        assert f(ctx, 1, p, None, 1, None, p) == -1 and what in err()
    assert hit(L.tor_patch_hit_device, (None,))(ctx, 1, p, None, 1, p, None) == -1 and "NULL rays, hits or patch" in err()
    assert all(v == 0.0 for v in buf)


# ---- Python glue on a recording library ---------------------------------------------------------------------------------------------------

class _Recorder:
    """A stand-in for the loaded library (the pattern of tests/test_texture_query.py): every tor_* entry records (name, args) and
    returns 0; tor_patch_info answers with `info`."""

    def __init__(self, info=(0, 0), note=b"patch hit"):
        self.calls, self.info, self.note = [], info, note

    def __getattr__(self, name):
        if not name.startswith("tor_"):
            raise AttributeError(name)
        if name == "tor_last_note":
            return lambda: self.note
        if name == "tor_last_error":
            return lambda: b""

        def entry(*args):
            self.calls.append((name, tuple((a.value or 0) if isinstance(a, C.c_void_p) else a for a in args)))
            if name == "tor_patch_info":
                for k in range(2):
                    C.cast(args[1], C.POINTER(C.c_int64))[k] = self.info[k]
            return 0
        return entry


def test_g_python_glue_on_a_recording_library(tor):
    ctx = object.__new__(tor.Context)
    ctx._h = C.c_void_p(16)
    saved = tor._lib
    try:
        rec = tor._lib = _Recorder()
        seen = {}

        def look(*args):                                                         # read the table while it is alive
            seen["table"] = bytes(C.string_at(args[2], 88 * args[1]))
            seen["n"] = args[1]
            return 0
        rec.tor_scene_patches = look
        tri = tor.Patch.triangle((1, 2, 3), (2, 2, 3), (1, 2, 5), material=4, groups=6)
        ctx.set_patches([tor.Patch.quad((0, 0, 0), (2, 0, 0), (0, 0, 4)), tri] + tor.box_patches((0, 0, 0), (1, 2, 3), 1, 0x1FFFFFFFF))
        t = (tor.PatchRecord * 8).from_buffer_copy(seen["table"])
        assert seen["n"] == 8 and [(r.kind, r.material, r.groups) for r in t[:3]] == [(0, -1, 0xFFFFFFFF), (1, 4, 6), (0, 1, 0xFFFFFFFF)]
        assert (tuple(t[1].q), tuple(t[1].u), tuple(t[1].v)) == ((1.0, 2.0, 3.0), (1.0, 0.0, 0.0), (0.0, 0.0, 2.0))
        want = I.box((0, 0, 0), (1, 2, 3), 1)
        for r, w in zip(t[2:], want):                                            # box_patches is the restated box, outward normals
            assert (tuple(r.q), tuple(r.u), tuple(r.v)) == (tuple(w["q"]), tuple(w["u"]), tuple(w["v"]))
        centre = np.array([0.5, 1.0, 1.5])
        for w in want:
            n, mid = np.array(R.cross(w["u"], w["v"])), w["q"] + 0.5 * w["u"] + 0.5 * w["v"]
            assert np.dot(n, mid - centre) > 0
        del rec.tor_scene_patches
        ctx.set_patches([])                                                      # clears
        assert rec.calls[-1] == ("tor_scene_patches", (16, 0, None))
        with pytest.raises(ValueError):
            ctx.set_patches([object()])
        rec = tor._lib = _Recorder(info=(8, 7))
        assert ctx.patches() == (8, 7)
        # the closest-hit query
        rec = tor._lib = _Recorder()
        rays = I.BY_NAME["one_quad"]["rays"][:6]
        ph = ctx.hit_patches(rays)
        (name, a), = rec.calls
        assert name == "tor_patch_hit_host" and len(a) == 12 and a[:6] == (16, 6, rays.ctypes.data, 0, 0, 6) and a[6] == 0
        assert a[7:] == (ph.raw.ctypes.data, ph.patch.ctypes.data, ph.uv.ctypes.data, 0, 0xFFFFFFFF)
        assert isinstance(ph, tor.PatchHits) and isinstance(ph, tor.HitResult) and ph.mode == "patch hit"
        assert (ph.patch == -1).all() and (ph.object == -1).all() and ph.uv.shape == (6, 2) and ph.patch.dtype == np.int32 and (ph.raw[:, :7] == 0).all()
        # merge: a copy of the records, merge = 1; a result goes where its records go; per-ray masks, ranges and a list
        sphere = I._fabricated(6, [1.0] * 6, [2] * 6)
        rec = tor._lib = _Recorder()
        tr = np.tile(np.array([0.0, 2.0]), (6, 1))
        mg = ctx.hit_patches(rays, t_range=tr, index=[4, 0], mask=np.arange(6, dtype=np.uint32), merge=tor.HitResult(sphere, sphere.view(np.int32), "hit: blocks"))
        (name, a), = rec.calls
        assert a[3] == tr.ctypes.data and a[4] not in (0, 16) and a[5] == 2 and a[6] == 1 and a[10] not in (0, 16) and a[11] == 0
        assert mg.raw is not sphere and np.array_equal(mg.raw, sphere) and a[7] == mg.raw.ctypes.data
        rec = tor._lib = _Recorder()
        again = ctx.hit_patches(rays, mask=5, merge=sphere, out=mg)              # in place
        (name, a), = rec.calls
        assert again.raw is mg.raw and again.patch is mg.patch and again.uv is mg.uv and a[6] == 1 and a[10:] == (0, 5)
        other = tor.PatchHits(np.zeros((5, 8)), np.zeros((5, 8)).view(np.int32), np.zeros(5, dtype=np.int32), np.zeros((5, 2)), "")
        for bad in (lambda: ctx.hit_patches(np.zeros((6, 6))), lambda: ctx.hit_patches(rays, out=other), lambda: ctx.hit_patches(rays, out=sphere),
                    lambda: ctx.hit_patches(rays, merge=np.zeros((5, 8))), lambda: ctx.hit_patches(rays, t_range=np.zeros((6, 3)))):
            with pytest.raises(ValueError):
                bad()
        # the any-hit query
        rec = tor._lib = _Recorder(note=b"patch occluded")
        oc = ctx.occluded_patches(rays)
        (name, a), = rec.calls
        assert name == "tor_patch_occluded_host" and len(a) == 10 and a[:7] == (16, 6, rays.ctypes.data, 0, 0, 6, 0)
        assert a[7:] == (oc.raw.ctypes.data, 0, 0xFFFFFFFF) and isinstance(oc, tor.OccludedResult) and oc.mode == "patch occluded" and not oc.occluded.any()
        bits = np.array([1, 0, 1, 0, 0, 0], dtype=np.int32)
        rec = tor._lib = _Recorder(note=b"patch occluded")
        om = ctx.occluded_patches(rays, merge=tor.OccludedResult(bits, bits.view(np.bool_).reshape(6, 4)[:, 0], "occluded: blocks"), mask=3)
        (name, a), = rec.calls
        assert a[6] == 1 and om.raw is not bits and np.array_equal(om.raw, bits) and a[8:] == (0, 3)
        rec = tor._lib = _Recorder(note=b"patch occluded")
        assert ctx.occluded_patches(rays, merge=bits, out=om).raw is om.raw and rec.calls[0][1][6] == 1
        with pytest.raises(ValueError):
            ctx.occluded_patches(rays, out=np.zeros(5, dtype=np.int32))
        # trace_patches without a table: refused before any launch
        rec = tor._lib = _Recorder()
        with pytest.raises(ValueError, match="needs a patch table"):
            ctx.trace_patches(np.zeros((3, 7)), np.zeros((3, 4), dtype=np.uint64), 4)
        assert [n for n, _ in rec.calls] == ["tor_patch_info"]
    finally:
        tor._lib = saved
        ctx._h = C.c_void_p()


def test_g_bind_keeps_its_tables(tor):
    import types
    assert not set(tor.PATCH_SYMBOLS) & (set(tor._SIGNATURES) | set(tor._PHASE_SIGNATURES) | set(tor._GRID_SIGNATURES) | set(tor._TEXTURE_SIGNATURES))
    older = types.SimpleNamespace(tor_patch_info=types.SimpleNamespace(argtypes=None, restype=C.c_int))
    tor._bind(older, tor.PATCH_SYMBOLS, skip_missing=True, table=tor._PATCH_SIGNATURES)   # an A/B build older than the entries
    assert older.tor_patch_info.argtypes == tor._PATCH_SIGNATURES["tor_patch_info"]
    with pytest.raises(AttributeError):
        tor._bind(older, tor.PATCH_SYMBOLS, table=tor._PATCH_SIGNATURES)


if __name__ == "__main__":                                                       # the table of profiles/patch_mutants.txt
    for v in R.VARIANTS:
        print(f"#   {v:26s} {' '.join(differing_cases(v)):110s} {TOLD_APART_BY[v]}")
