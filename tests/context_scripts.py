"""Scripts over ONE long-lived context, and a model of the context's documented state (tests/test_context_scripts.py on the CPU,
tests/test_gpu_context_scripts.py on the MI355X).

A script is a list of steps -- setters (upload, set_groups, set_lights, set_environment, set_media, set_media_phase,
build_photons, set_media_grid, set_textures, set_patches), queries of every family, renders and the passes of two open accumulations -- as a host that keeps one context alive for a whole animation issues them.  script(name) returns
the steps; Model replays them and says, per step, EITHER the state the answer depends on (records, group words or none, light table
or none, environment map or none, media table with its g or none, photon map or none, the density grids by medium, texture
table or none, patch table or none) OR that the step must be refused (code, a
word of the message).  The model restates include/tor_render.h, tor_lights.h, tor_env.h, tor_media.h, tor_phase.h, tor_photons.h,
tor_grid.h, tor_texture.h, tor_patches.h and the Python docstrings (what an upload resets and what it keeps); inputs() draws a
step's operands and answer() hands them to the family's restatement under a given state.  Nothing here judges an answer.

The inputs are shaped so that a stale cache shows: the edited copy of a scene changes the ground sphere's radius and material and
the centre of object 3, so `probe` rows (segments that end between the two grounds, points a little above the ground, hits and BSDF
items on the ground, lamps that include object 3) answer differently under the old records; `movers` rows are aimed at movers at
times at the far end of the new time range; media rows are aimed at the boundary objects of the media tables, object 3 first
among them; gather points come from the point sets of the current photon map and of the one before it.  numpy only (the restatements of bounce, scatter, radiance and the samplers draw
through the oracle's exported generator, which the caller hands in).

The grids, the textures and the patches: a grid march's rays are aimed at the boundary object of its medium and a lookup's points
lie in and around it (MOVED's grid rides a centre that the edit moves); albedo's records are the hit restatement's on ground
probes, rows aimed at MOVED, back faces and misses (the ground is unbound under texture key A: its material is what the edit
changes); the patch families' probe rows end on the floor the patch tables lie on, between the original's ground and the edited
copy's.  hit_patches_merged is ctx.hit_patches(rays, merge=ctx.hit(rays)) issued as ONE step, occluded_patches merges into
occluded()'s bits where the step says so.  Exempt from the stale-sensitivity rule, with alternatives()'s reasons: hit_patches and
the unmerged occluded_patches behind an upload (they read no scene record); the merged occluded_patches behind another patch
table (the original's ground occludes every probe row; the unmerged steps hold the table); albedo behind set_textures behind a
replacing upload under key B (the ground is bound: key A holds the untextured path); a grid family there when the list before
holds the medium's boundary unchanged (the mover's); media_density never depends on sigma (a stale sigma cannot show in it: the
march holds it); `time` and `words` at all of them.  The host integrators (trace_patches, trace_media, trace_media_direct, trace
with textures, transmittance) stay out of the scripts: they are Python loops over these queries, and their own tests hold them.
"""
import copy

import numpy as np

import bounce_restatement as B
import bsdf_inputs as BI
import bsdf_restatement as BR
import camera_inputs as CI
import camera_restatement as CR
import crossings_restatement as X
import deposit_inputs as DI
import deposit_restatement as D
import env_inputs as EI
import env_restatement as ER
import grid_inputs as GI
import grid_restatement as GR
import hit_restatement as H
import light_inputs as LI
import light_restatement as LR
import masked_restatement as M
import media_inputs as MI
import media_restatement as MR
import nearest_inputs as NI
import nearest_restatement as N
import patch_restatement as PT
import phase_restatement as PR
import photon_inputs as PI
import photon_restatement as PH
import query_regimes as Q
import radiance_restatement as RR
import render_regimes as R
import texture_inputs as TI
import texture_restatement as TR

# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
# name: (the regime of tests/query_regimes.py it is cut from, how many of its records, edited copy?)
SCENES = {"g9": ("groups", 9, False), "g9_e": ("groups", 9, True), "dense": ("dense", None, False), "dense_e": ("dense", None, True),
          "noground": ("noground", None, False), "tiny": ("tiny", None, False), "dense2": ("dense2", None, False),
          "odd_objects": ("odd_objects", None, False)}
DELTA = 0.25                                            # the edited ground is this much (x the regime's scale) smaller
MOVED, OFFSET = 3, np.array([0.37, 0.11, -0.23])        # the object whose centre the edit moves, and by how much (x the scale)
GROUND_EDIT = dict(kind=1.0, albedo=(0.9, 0.3, 0.2), fuzz=0.3)   # Lambertian grey -> a fuzzy red Metal
WHY_RADII = "the block boxes' margin holds for no ray origin (radii too small)"
_records = {}


def regime(name):
    return SCENES[name][0]


def scale(name):
    return R.spread_of(regime(name)) / 12.0


def records(name):
    """(n, 16) float64 records of the named scene: built once, read-only."""
    if name not in _records:
        reg, count, edited = SCENES[name]
        recs = np.array(Q.scene(reg, 0)[:count], dtype=np.float64)
        if edited:
            s = scale(name)
            assert ground(recs) == 0
            recs[0, 9] -= DELTA * s
            recs[0, 10], recs[0, 11:14], recs[0, 14] = GROUND_EDIT["kind"], GROUND_EDIT["albedo"], GROUND_EDIT["fuzz"]
            recs[MOVED, 1:4] += OFFSET * s
            recs[MOVED, 4:7] += OFFSET * s
        recs.setflags(write=False)
        _records[name] = recs
    return _records[name]


def partner(name):
    """The other scene of an (original, edited copy) pair, or None."""
    other = name[:-2] if name.endswith("_e") else name + "_e"
    return other if other in SCENES else None


def placeable(recs):
    """Mask of the objects a row can be placed by: finite, not astronomically far out, with a centre at every time, no ground."""
    recs = np.asarray(recs, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(recs[:, 1:10]).all(axis=1) & (np.abs(recs[:, 1:7]) < 1e100).all(axis=1)
        ok &= (recs[:, 0] == 0) | (recs[:, 7] != recs[:, 8])             # (a mover with time0 == time1 has no centre to aim at)
    if ground(recs) == 0:
        ok[0] = False
    return ok


def has_blocks(name):
    """Does the scene get a culling layout?  Fewer than 32 objects of ordinary size do not (tor_scene.cpp build_accel: the nine
    of g9), and no query of theirs reads `bnd`; the GPU test asserts that the block modes run the blocks on the others."""
    return len(records(name)) > 64


def ground(recs):
    """0 when record 0 is a ground sphere (far larger than the others), else None."""
    r = np.abs(recs[:, 9])
    with np.errstate(invalid="ignore"):
        return 0 if r[0] > 50.0 * np.nanmedian(r) else None


# ---- the other state a step can depend on ------------------------------------------------------------------------------------------------
GROUPS = ("A", "B")
LIGHTS = {"A": ([3, 5, 7], [10.0, 1.0, 1.0]), "B": ([7, 3], None)}     # lamps by object index (every scene has nine objects or more)
ENVS = ("n4", "n16")
_envs = {}


def words(key, n):
    """The group words of `key` for n objects: None (no words), query_regimes.group_words, or the same pattern two bits on."""
    if key is None:
        return None
    w = Q.group_words(n)
    if key == "B":
        j = np.arange(n)
        w = (np.uint32(1) << ((j + 2) % 5).astype(np.uint32)).astype(np.uint32)
        w[5::11] = 0
        w[::13] = Q.ALL
    return w


def light_table(key):
    objects, weights = LIGHTS[key]
    return np.asarray(objects, dtype=np.int32), None if weights is None else np.asarray(weights, dtype=np.float64)


def env_map(key):
    """(rgb, importance, the restatement's table) of an environment map: the 4 x 4 one of env_inputs, or a 16 x 16 one."""
    if key not in _envs:
        rgb, imp = EI.env_map("dyadic4") if key == "n4" else (np.random.RandomState(16).uniform(0.05, 1.0, size=(16, 16, 3)), None)
        _envs[key] = (rgb, imp, ER.table(rgb, imp))
    return _envs[key]


# ---- media tables, asymmetries, photon maps ------------------------------------------------------------------------------------------------
# A media table lists boundary objects of the uploaded scene: boundaries(scene) = [MOVED, a mover where the scene has one, the two
# objects nearest to MOVED] (in the dense scenes they overlap it: several media at once).  name: (which of the four, in table
# order; sigma x the scene's scale; albedo).  B lists three of A's four in another order with other sigma and albedo: a stale
# table shows, and so does a table packed from the previous records (the edit moves MOVED); the counts differ, so the note does too.
MEDIA = {"A": ((0, 1, 2, 3), (2.0, 0.7, 3.0, 1.3), ((0.9, 0.1, 0.5), (0.2, 0.8, 1.0), (0.6, 0.6, 0.3), (1.0, 0.5, 0.25))),
         "B": ((2, 0, 1), (1.1, 2.5, 0.9), ((0.3, 0.6, 0.9), (0.7, 0.7, 0.1), (0.05, 0.4, 0.8)))}
BAD_MEDIA = {"twice": "listed twice", "negative": "sigma"}      # refused tables: an index listed twice, a negative sigma
G = {"P": (0.6, -0.4, 0.0, 0.85), "Q": (-0.7, 0.3, -0.2, 0.0)}   # per medium, cut to the table's count: every sign changes, each has a 0
# name: (the case of tests/photon_inputs.py, directions?, radius, what the powers are multiplied by -- the Python layer's scale
# differs by 2^52 between L and S --, how many of the case's points are near photons)
PHOTON_MAPS = {"L": ("sparse", True, PI.R, 2.0 ** 12, 192), "S": ("dense257", False, 0.2, 2.0 ** -40, 96), "E": ("dense0", True, PI.R, 1.0, 96)}
PATHS = 1000.0                                          # what PhotonGather.irradiance divides by
_boundaries, _maps = {}, {}


def boundaries(name):
    """The four boundary objects of a scene's media tables (see MEDIA)."""
    if name not in _boundaries:
        recs = records(name)
        ok = placeable(recs) & (np.abs(recs[:, 9]) > 0)
        assert ok[MOVED]
        ok[MOVED] = False
        movers = np.flatnonzero(ok & (recs[:, 0] == 1))
        m = int(movers[0]) if movers.size else int(np.flatnonzero(ok)[0])
        ok[m] = False
        rest = np.flatnonzero(ok)
        gap = np.linalg.norm(recs[rest, 1:4] - recs[MOVED, 1:4], axis=1) - np.abs(recs[rest, 9]) - abs(recs[MOVED, 9])
        near = rest[np.argsort(gap, kind="stable")[:2]]
        _boundaries[name] = (MOVED, m, int(near[0]), int(near[1]))
    return _boundaries[name]


def media_table(key, name, bad=None):
    """(objects int32, sigma, albedo (n, 3)) of the named table on the named scene; bad: one of BAD_MEDIA."""
    which, c, albedo = MEDIA[key]
    objects = np.array([boundaries(name)[k] for k in which], dtype=np.int32)
    sigma = np.array(c, dtype=np.float64) / scale(name)
    if bad == "twice":
        objects[-1] = objects[0]
    if bad == "negative":
        sigma[1] = -sigma[1]
    return objects, sigma, np.array(albedo, dtype=np.float64)


def g_vector(key, n):
    """The asymmetries of `key` for a table of n media; None: every medium 0."""
    return np.zeros(n) if key is None else np.array(G[key][:n], dtype=np.float64)


def power_scale(powers):
    """Context.build_photons' docstring: the power of two that puts the largest finite channel in (1/2, 1]."""
    p = np.asarray(powers, dtype=np.float64)
    top = float(np.where(np.isfinite(p), p, 0.0).max()) if p.size else 0.0
    if not top > 0.0:
        return 1.0
    s = 2.0 ** -np.ceil(np.log2(top))
    assert 0.5 < top * s <= 1.0
    return float(s)


def photon_map(key, listed=False):
    """The named map: position, power, direction (or None), radius, index (the build's list or None: `listed` keeps every other photon
    in another order, one of them twice, with two entries outside), scale (the Python layer's) and stored, the
    restatement's map of the scaled powers.  points: the case's query points that lie near photons."""
    if (key, listed) not in _maps:
        case, dirs, radius, factor, n_near = PHOTON_MAPS[key]
        c = PI.BY_NAME[case]
        n = len(c["position"])
        index = None
        if listed and n:
            perm = np.random.default_rng(n).permutation(n)
            index = np.concatenate([perm[:n - n // 2], [-1, n, perm[0]]]).astype(np.int32)
        power = c["power"] * factor
        s = power_scale(power)
        m = dict(position=c["position"], power=power, direction=c["direction"] if dirs else None, radius=radius, index=index, scale=s,
                 has_dir=dirs, points=c["points"][:n_near])
        m["stored"] = PH.store(m["position"], power * s, m["direction"], radius, index)
        _maps[(key, listed)] = m
    return _maps[(key, listed)]


# ---- density grids, texture tables, patch tables -------------------------------------------------------------------------------------------
# A grid is attached to a ROLE of the media table, resolved to a medium index under the table that is set: "moved" is the entry
# that is object MOVED (index 0 of table A, 1 of B), "mover" the entry that is boundaries()[1] (1 of A, 2 of B) -- a medium index
# kept across set_media names another object --; an int is taken as it is (7: outside every table).
# name: (dims, the box as multiples of the boundary's |radius| or None for the sphere's bounding cube, every which cell is 0).
# Every dimension is distinct (a transposed stride shows); G2 has fewer cells than G1 (a smaller grid replaces a larger one); G3 has
# G1's cell count in another shape (strides kept from the grid before would show).
GRIDS = {"G1": ((5, 4, 3), (-0.9, -0.5, -0.7, 0.6, 0.8, 0.75), 7), "G2": ((2, 3, 7), None, 5), "G3": ((3, 5, 4), None, 6)}
BAD_GRIDS = {"dims": "TOR_GRID_MAX_DIM", "nan": "finite and >= 0", "negative": "finite and >= 0"}   # refused grids (no such key is stored)
ROLES = {"moved": 0, "mover": 1}                         # role: which of boundaries()
TEXTURES = ("A", "B")
PATCHES = {"A": 65, "B": 9}                              # one past a wave's worth, and a smaller table behind it
PATCH_MASK = 0x16                                        # the scalar mask of every third patch step: bits 1, 2 and 4
_densities, _textures, _patch_tables = {}, {}, {}


def medium_of(table, who):
    """The medium index `who` names under media table `table`: a role's index in the table (None where it lists no such object), or
    the int itself."""
    if not isinstance(who, str):
        return int(who)
    which = MEDIA[table][0]
    return which.index(ROLES[who]) if ROLES[who] in which else None


def grid_density(key):
    """(nx, ny, nz) densities of a named grid: distinct per cell, with exact zeros; or a refused one: 1025 x 1 x 1 cells, a NaN, a
    negative value."""
    if key not in _densities:
        if key == "dims":
            d = np.ones((GR.GRID_MAX_DIM + 1, 1, 1))
        else:
            dims, _, zero = GRIDS["G1" if key in BAD_GRIDS else key]
            d = GI._distinct(dims, sum(dims)).copy()
            d.reshape(-1)[::zero] = 0.0
            if key in BAD_GRIDS:
                d[1, 1, 1] = np.nan if key == "nan" else -0.5
        d.setflags(write=False)
        _densities[key] = d
    return _densities[key]


def grid_box(key, name, obj):
    """The box of a named grid on object `obj` of the named scene: offsets from the centre, six numbers, or None."""
    box = GRIDS["G1" if key in BAD_GRIDS else key][1]
    return None if box is None else np.array(box, dtype=np.float64) * abs(records(name)[obj, 9])


def _grid(state, medium):
    """grid_restatement's grid of `medium` under `state` (it rides the centre the table was packed with: state.packed's)."""
    objects = media_table(state.media, state.scene)[0]
    key = state.grids[medium]
    return GR.make_grid(records(state.packed or state.scene), objects, medium, grid_density(key), grid_box(key, state.scene, int(objects[medium])))


def texture_table(key, name, bad=None):
    """(textures as texture_restatement's dicts, binding (n_objects,) int32) of the named table on the named scene.  A: a constant,
    a world-space checker (cells in units of the scene's scale), a normal-space checker, an 8 x 8 bilinear image and a 4 x 4 nearest
    image behind it in the atlas; the ground unbound.  B: a constant and a 2 x 2 bilinear image: a smaller table with a smaller
    atlas; the ground bound.  MOVED wears an image in both.  bad: "long" (one binding too many), "outside" (a binding past the table)."""
    if (key, name) not in _textures:
        s, n = scale(name), len(records(name))
        j = np.arange(n)
        if key == "A":
            tex = [TR.constant((0.8, 0.4, 0.1)), TR.checker((0.9, 0.9, 0.2), (0.1, 0.2, 0.7), (1.3 / s, 0.7 / s, 2.1 / s), TR.WORLD),
                   TR.checker((0.2, 0.7, 0.3), (0.6, 0.1, 0.5), (3.0, 2.0, 5.0), TR.NORMAL), TR.image(TI.ramp(8), TR.BILINEAR),
                   TR.image(TI.ramp(4, 100.0), TR.NEAREST)]
            binding = np.array([-1, 0, 1, 3, 2, 4, -1], dtype=np.int32)[j % 7]
            binding[0], binding[MOVED] = -1, 3
        else:
            tex = [TR.constant((0.3, 0.6, 0.9)), TR.image(TI.ramp(2, 7.0), TR.BILINEAR)]
            binding = np.array([-1, 0, 1], dtype=np.int32)[j % 3]
            binding[0], binding[MOVED] = 0, 1
        binding.setflags(write=False)
        _textures[(key, name)] = (tex, binding)
    tex, binding = _textures[(key, name)]
    if bad == "long":
        binding = np.concatenate([binding, [-1]]).astype(np.int32)
    if bad == "outside":
        binding = binding.copy()
        binding[1] = len(tex)
    return tex, binding


def floor_height(name, x, z):
    """The surface the patch tables lie on and the patch families' probe rows end at: the sphere half way between the ground and
    the edited copy's (the same from either scene); without a ground, the plane one scale below the objects."""
    recs = records(name)
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    if ground(recs) == 0:
        return _ground_height(name, recs, x, z, _probe_radius(name, recs))
    return np.full(np.broadcast(x, z).shape, _others_box(records(name[:-2] if name.endswith("_e") else name))[0][1] - scale(name))


def patch_region(name):
    """(x0, x1, z0, z1) the probe rows are drawn over: the box of the ORIGINAL scene's objects (the same from a scene and its copy)."""
    lo, hi = _others_box(records(name[:-2] if name.endswith("_e") else name))
    return float(lo[0]), float(hi[0]), float(lo[2]), float(hi[2])


def patch_table(key, name, bad=None, of=None):
    """The named patch table on the named scene, as patch_restatement's patches: A tiles the lower 60 % of the region's x extent
    8 x 8 (and one more patch across its middle), B the upper 60 % 3 x 3 -- they share no patch --; every patch fills 90 % of its
    tile, every third is a triangle (half of that).  A patch lies along the floor (floor_height at three of its corners), 0.05
    scales above it where the index is 2 of 3 -- between the two grounds: the original's ground wins a merge, in the edited copy
    the patch does -- and 0.3 above it otherwise -- above both grounds: the patch wins in either scene.  Materials by
    turns -1, 0 (the ground), MOVED; visibility words one bit of five, every 7th every group, every 11th none.  bad = "material":
    patch 1 wears the last object of scene `of`, or (of None) one past this scene's last."""
    if (key, name) not in _patch_tables:
        s = scale(name)
        x0, x1, z0, z1 = patch_region(name)
        w = x1 - x0
        (xa, xb), k = ((x0, x0 + 0.6 * w), 8) if key == "A" else ((x0 + 0.4 * w, x1), 3)
        dx, dz = (xb - xa) / k, (z1 - z0) / k
        tiles = [(xa + a * dx, z0 + b * dz, dx, dz) for a in range(k) for b in range(k)]
        if key == "A":
            tiles.append((xa + 0.25 * (xb - xa), z0 + 0.25 * (z1 - z0), 0.5 * (xb - xa), 0.5 * (z1 - z0)))
        table = []
        for j, (tx, tz, ex, ez) in enumerate(tiles):
            up = (0.05 if j % 3 == 2 else 0.3) * s + (0.1 * s if j == 64 else 0.0)
            cx, cz = (tx + 0.05 * ex, tx + 0.95 * ex), (tz + 0.05 * ez, tz + 0.95 * ez)
            q = np.array([cx[0], float(floor_height(name, cx[0], cz[0])) + up, cz[0]])
            pu = np.array([cx[1], float(floor_height(name, cx[1], cz[0])) + up, cz[0]])
            pv = np.array([cx[0], float(floor_height(name, cx[0], cz[1])) + up, cz[1]])
            groups = Q.ALL if j % 7 == 0 else 0 if j % 11 == 5 else 1 << (j % 5)
            material = (-1, 0, MOVED)[(j // 3) % 3]
            table.append(PT.triangle(q, pu, pv, material, groups) if j % 3 == 1 else PT.quad(q, pu - q, pv - q, material, groups))
        assert len(table) == PATCHES[key]
        _patch_tables[(key, name)] = table
    table = _patch_tables[(key, name)]
    if bad == "material":
        table = list(table)
        table[1] = dict(table[1], material=len(records(of)) - 1 if of else len(records(name)))
    return table


# ---- families ---------------------------------------------------------------------------------------------------------------------------
RAY_FAMILIES = ("hit", "occluded", "crossings", "bounce", "radiance")
BLOCK_FAMILIES = RAY_FAMILIES + ("nearest",)            # they take a mode and a time range: `bnd` and what hangs on it
MASKED = tuple(f + "_m" for f in ("hit", "occluded", "crossings", "nearest", "bounce"))
LIGHT_FAMILIES = ("sample_lights", "light_pdf", "emit_lights")
ENV_FAMILIES = ("environment", "sample_environment")
MEDIA_FAMILIES = ("march_media", "scatter_media", "sample_phase", "phase")   # they read the media table
PHASE_FAMILIES = ("sample_phase", "phase")              # ... and word 15 of it
GRID_FAMILIES = ("march_media_grid", "media_density")    # they read ONE medium's density grid (and the media table under it)
PATCH_FAMILIES = ("hit_patches", "hit_patches_merged", "occluded_patches")
TABLE_FAMILIES = GRID_FAMILIES + ("albedo",) + PATCH_FAMILIES   # the grids, the texture table, the patch table
NEW_FAMILIES = ("gather_photons",) + MEDIA_FAMILIES + ("uniform",) + TABLE_FAMILIES
SCENE_FREE = ENV_FAMILIES + ("connect_camera", "deposit", "gather_photons", "uniform")   # they read no scene: no upload can change their answer
QUERY_FAMILIES = BLOCK_FAMILIES + ("scatter", "bsdf") + MASKED + LIGHT_FAMILIES + ENV_FAMILIES + ("connect_camera", "deposit") + NEW_FAMILIES
FAMILIES = QUERY_FAMILIES + ("render",)
ACCUMULATIONS = ("progressive", "pixel_progressive")
SLOW = ("bounce", "bounce_m", "scatter", "radiance", "sample_phase", "march_media_grid")    # their restatements loop in Python: 64 rays
BATCHES = (1, 63, 64, 65, 257)
MODES = ("auto", "brute", "blocks")
TIME_RANGES = ((0.0, 1.0), (0.5, 0.5), (-3.0, 0.5), None)
UPLOAD_EVENTS = ("replace", "cache_hit", "refused")
FILM, RADIANCE_DEPTH = (5, 10), 8


def base(family):
    return family[:-2] if family.endswith("_m") else family


def takes_mode(family):
    return base(family) in BLOCK_FAMILIES


EVENTS = UPLOAD_EVENTS + ("time", "words")
# which setter writes the table a family reads (the `setter` / `behind_queued_work` pair)
SETTER_OF = dict([(f, ("set_lights",)) for f in LIGHT_FAMILIES] + [(f, ("set_environment",)) for f in ENV_FAMILIES]
                 + [(f, ("set_media", "set_media_phase") if f in PHASE_FAMILIES else ("set_media",)) for f in MEDIA_FAMILIES]
                 + [("gather_photons", ("build_photons",))] + [(f, ("set_media_grid",)) for f in GRID_FAMILIES]
                 + [("albedo", ("set_textures",))] + [(f, ("set_patches",)) for f in PATCH_FAMILIES])
TABLE_SETTERS = ("set_media_grid", "set_textures", "set_patches")


def transition_table():
    """The committed table: the cross product of every query and render family with the five events -- a replacing, a cache-hit
    and a refused upload, the time range changed since the last block query (`bnd` rebuilt), the group words changed since the last
    masked query (`grp` rebuilt) -- and the four pairs; then what the media table, its phase word and the photon map add (below).
    The two accumulations have two passes per script and stand in the table as a pair."""
    t = [(f, e) for f in FAMILIES for e in EVENTS]
    t += [(f, "lights_after_upload") for f in LIGHT_FAMILIES] + [(f, "map_kept") for f in ENV_FAMILIES]
    t += [("host_twin", "smaller_after_device"), ("accumulation", "ten_foreign_steps")]
    # media_table / phase_g / photon_map: another table, g or map since the family last ran; media_after_upload: set_media after a
    # replacing upload copies the NEW records; map_kept: a gather behind a replacing upload; a host twin of the new families behind a
    # larger device call of another family; a setter behind a render and a query of the table it writes, no host step between
    t += [(f, "media_table") for f in MEDIA_FAMILIES] + [(f, "phase_g") for f in PHASE_FAMILIES] + [("gather_photons", "photon_map")]
    t += [(f, "media_after_upload") for f in MEDIA_FAMILIES] + [("gather_photons", "map_kept")]
    t += [("new_host_twin", "smaller_after_device"), ("setter", "behind_queued_work")]
    # the density grids, the texture table and the patch table (the five events of every family come with FAMILIES above).
    # grid: another grid on the medium since the family last ran; grid_removed: the medium's grid removed (refused); grids_dropped:
    # a set_media since (the grid march refused, the homogeneous march counts the medium again); grids_kept: behind set_media_phase,
    # set_lights or a cache-hit upload; grid_after_upload: set_media and set_media_grid after a replacing upload (the grid rides the
    # new centre); (march_media, grid): the homogeneous march behind a grid set and behind one removed.  texture_table /
    # patch_table: the other key; *_after_upload: the table set again behind a replacing upload; *_kept: behind another setter or a
    # cache-hit upload.  A host twin of these families behind a larger device call; each of the three setters behind queued work.
    t += [(f, e) for f in GRID_FAMILIES for e in ("grid", "grid_removed", "grids_dropped", "grids_kept", "grid_after_upload")]
    t += [("march_media", "grid"), ("march_media", "grid_removed"), ("march_media", "grids_dropped")]
    t += [("albedo", e) for e in ("texture_table", "textures_after_upload", "textures_kept")]
    t += [(f, e) for f in PATCH_FAMILIES for e in ("patch_table", "patches_after_upload", "patches_kept")]
    t += [("table_host_twin", "smaller_after_device")] + [(op, "behind_queued_work") for op in TABLE_SETTERS]
    return t


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class State:
    """What an answer can depend on: names and keys, resolved by records(), words(), light_table(), env_map()."""

    def __init__(self, scene=None, groups=None, lights=None, env=None, media=None, phase=None, photons=None, grids=None, textures=None,
                 patches=None):
        self.scene, self.groups, self.lights, self.env = scene, groups, lights, env
        self.media, self.phase, self.photons = media, phase, photons   # a key of MEDIA, a key of G, (a key of PHOTON_MAPS, listed?)
        self.grids = dict(grids or {})                    # medium index: a key of GRIDS (never changed in place: but() replaces it)
        self.textures, self.patches = textures, patches   # a key of TEXTURES, a key of PATCHES
        self.packed = None                                # alternatives() alone: the scene whose records a stale table was packed from

    def but(self, **kw):
        s = copy.copy(self)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def key(self):
        return (self.scene, self.groups, self.lights, self.env, self.media, self.phase, self.photons, tuple(sorted(self.grids.items())),
                self.textures, self.patches)


REFUSED = "refused"


def table_refusal(step, s):
    """The refusal of a query of TABLE_FAMILIES under state s, in the headers' order, or None: no scene; then (grids) no media
    table, a medium outside it, a medium without a grid; (albedo) no texture table; (patches) no patch table."""
    f = step["family"]
    if s.scene is None:
        return (-1, "no scene")
    if f in GRID_FAMILIES:
        if s.media is None:
            return (-1, "media table")
        m = medium_of(s.media, step["who"])
        if m is None or not 0 <= m < len(MEDIA[s.media][0]):
            return (-1, "outside the media table")
        return None if m in s.grids else (-1, "has no density grid")
    if f == "albedo":
        return None if s.textures is not None else (-1, "no texture table")
    return None if s.patches is not None else (-1, "no patch table")


class Expect:
    """The model's word on one step: `state` the answer depends on, or `refuse` = (code, a word of the message); `events`: what
    happened since this family last ran, {event: the previous value}."""

    def __init__(self, step, state, refuse, events):
        self.step, self.state, self.refuse, self.events = step, state, refuse, events


class Model:
    """The context's documented state, replayed step by step.

    tor_scene_upload: every call counts in n_uploads; a byte-identical list counts in n_cache_hits and changes nothing; a list with
    an unknown kind is refused (TOR_ERR_INVALID_ARGUMENT, "unknown") and changes nothing; any other list replaces the scene, resets
    the group words (every object 0xFFFFFFFF) and clears the light table.  The environment map belongs to the context and
    survives every upload.  A light query without a table and an environment query without a map are refused (code -1, "light
    table" / "environment map").  Renders and unmasked queries read no words; the time range of a block query is a speed hint.

    tor_scene_media (include/tor_media.h): the table is packed from the scene's records at the call; an empty one clears it, and
    so does every replacing upload (a byte-identical or refused one keeps it); an index listed twice and a negative sigma are
    refused and change nothing; every table starts with g = 0.  tor_scene_media_phase (tor_phase.h): refused without a table
    ("media table") and with another count ("n_media").  The march, the scatter, the phase sampler and its evaluation are refused
    before the first upload ("no scene") and without a table ("media table").  tor_photons_build_device (tor_photons.h): the map
    belongs to the context and survives every upload, a build replaces it and needs no scene; a gather before any build is refused
    ("no photon map"), one with normals on a map built without directions too ("without directions"; a build of no photons holds
    nothing that normals could miss).  tor_rng_uniform_device needs nothing.

    tor_scene_media_grid (include/tor_grid.h): refused with no scene, an empty media table ("media table"), a medium outside the table
    ("outside the media table"), bad dimensions ("TOR_GRID_MAX_DIM"), a density that is NaN or negative ("finite and >= 0"), in
    that order; (0, 0, 0) removes that medium's grid only, a second grid on a medium replaces the first.  EVERY accepted
    tor_scene_media call -- the empty table included -- drops every grid, and so does a replacing upload; a refused table, a
    cache-hit and a refused upload, tor_scene_media_phase, the lights, the environment, the words, the photon map, the textures
    and the patches keep them.  The grid march and the density lookup are refused with no scene, no media table, a medium outside
    it and a medium without a grid ("has no density grid"); a medium with a grid takes no part in the homogeneous march.
    tor_scene_textures (tor_texture.h): refused with no scene, a binding whose length is not the scene's count ("n_objects must
    be"), a binding outside the table ("is outside"); an empty table clears it, as a replacing upload does; every other setter
    leaves it alone.  The query is refused with no scene, then with no table ("no texture table").  tor_scene_patches
    (tor_patches.h): refused with no scene and with a material outside [-1, n_objects) ("material outside"); an empty table clears
    it, as a replacing upload does; every other setter leaves it alone.  The two queries are refused with no scene, then with no
    table ("no patch table")."""

    def __init__(self):
        self.state = State()
        self.n_uploads = self.n_cache_hits = 0
        self.block_range = None                          # the effective time range of the last query that asked for the blocks
        self.masked_words = None                         # (scene, groups) at the last masked query
        self.since = {}                                  # family: {event: previous value}, since that family last ran
        self.passes = {a: [] for a in ACCUMULATIONS}     # accumulation: [(step number, scene)] of its passes
        self.n_steps = 0

    def _note(self, event, value, families=FAMILIES + ACCUMULATIONS):
        for f in families:
            self.since.setdefault(f, {})[event] = value

    def _kept(self, op, families=TABLE_FAMILIES):
        """An accepted setter that must leave the tables of `families` alone: the family's next step could tell."""
        for f in families:
            self.since.setdefault(f, {}).setdefault("kept", set()).add(op)

    def effective_range(self, step, times):
        """The (lo, hi) the library builds block bounds for: the step's range, or the finite min / max of the operand's times."""
        if step.get("time_range") is not None:
            return tuple(float(v) for v in step["time_range"])
        t = np.asarray(times, dtype=np.float64)
        t = t[np.isfinite(t)]
        return (float(t.min()), float(t.max())) if t.size else (0.0, 0.0)

    def apply(self, step, times=None):
        """Replays one step: returns its Expect and moves the state.  `times`: the time column of a block query's operand (for a
        time range of None)."""
        self.n_steps += 1
        op, s = step["op"], self.state
        if op == "upload":
            self.n_uploads += 1
            if step.get("bad"):
                self._note("refused", step["scene"])
                return Expect(step, s, (-1, "unknown"), {})
            if step["scene"] == s.scene:
                self.n_cache_hits += 1
                self._note("cache_hit", True)
                return Expect(step, s, None, {})
            for ev in self.since.values():               # (what an earlier upload left pending is superseded)
                ev.pop("cache_hit", None), ev.pop("refused", None)
            self._note("replace", s.scene)
            self._note("before", s, TABLE_FAMILIES)      # (what the upload cleared: the grids, the textures, the patches)
            self.state = State(step["scene"], None, None, s.env, None, None, s.photons)
            return Expect(step, self.state, None, {})
        if op == "set_media":
            if s.scene is None:
                return Expect(step, s, (-1, "no scene"), {})
            if step.get("bad"):
                return Expect(step, s, (-1, BAD_MEDIA[step["bad"]]), {})
            self._note("media_table", s.media, MEDIA_FAMILIES)
            self._note("phase_g", s.phase, PHASE_FAMILIES)   # (every table starts isotropic)
            if s.grids:                                  # ... and without a grid (the first drop since a family ran is the one that counts)
                for f in GRID_FAMILIES + ("march_media",):
                    self.since.setdefault(f, {}).setdefault("grids_dropped", (s.media, dict(s.grids)))
            self._kept(op, ("albedo",) + PATCH_FAMILIES)
            self.state = s.but(media=step["table"], phase=None, grids={})
            return Expect(step, self.state, None, {})
        if op == "set_media_grid":
            if s.scene is None:
                return Expect(step, s, (-1, "no scene"), {})
            if s.media is None:
                return Expect(step, s, (-1, "media table"), {})
            m = medium_of(s.media, step["who"])
            if m is None or not 0 <= m < len(MEDIA[s.media][0]):
                return Expect(step, s, (-1, "outside the media table"), {})
            if step["grid"] in BAD_GRIDS:
                return Expect(step, s, (-1, BAD_GRIDS[step["grid"]]), {})
            for f in GRID_FAMILIES + ("march_media",):   # (the key the family last saw on that medium)
                self.since.setdefault(f, {}).setdefault("grid", {}).setdefault(m, s.grids.get(m))
            self._kept(op, ("albedo",) + PATCH_FAMILIES)
            grids = {k: v for k, v in s.grids.items() if k != m}
            if step["grid"] is not None:
                grids[m] = step["grid"]
            self.state = s.but(grids=grids)
            return Expect(step, self.state, None, {})
        if op == "set_textures":
            if s.scene is None:
                return Expect(step, s, (-1, "no scene"), {})
            n = len(records(s.scene))
            if step.get("bad") == "long" or (step.get("count_of") and len(records(step["count_of"])) != n):
                return Expect(step, s, (-1, "n_objects must be"), {})
            if step.get("bad") == "outside":
                return Expect(step, s, (-1, "is outside"), {})
            self._note("texture_table", s.textures, ("albedo",))
            self._kept(op, GRID_FAMILIES + PATCH_FAMILIES)
            self.state = s.but(textures=step["table"])
            return Expect(step, self.state, None, {})
        if op == "set_patches":
            if s.scene is None:
                return Expect(step, s, (-1, "no scene"), {})
            n = len(records(s.scene))
            if step.get("bad") == "material" and (len(records(step["of"])) - 1 if step.get("of") else n) >= n:
                return Expect(step, s, (-1, "material outside"), {})
            self._note("patch_table", s.patches, PATCH_FAMILIES)
            self._kept(op, GRID_FAMILIES + ("albedo",))
            self.state = s.but(patches=step["table"])
            return Expect(step, self.state, None, {})
        if op == "set_media_phase":
            if s.scene is None:
                return Expect(step, s, (-1, "no scene"), {})
            if s.media is None:
                return Expect(step, s, (-1, "media table"), {})
            if step.get("wrong_count"):
                return Expect(step, s, (-1, "n_media"), {})
            self._note("phase_g", s.phase, PHASE_FAMILIES)
            self._kept(op)
            self.state = s.but(phase=step["g"])
            return Expect(step, self.state, None, {})
        if op == "build_photons":
            self._note("photon_map", s.photons, ("gather_photons",))
            self._kept(op)
            self.state = s.but(photons=(step["map"], bool(step["listed"])))
            return Expect(step, self.state, None, {})
        if op == "set_groups":
            self._kept(op)
            self.state = s.but(groups=step["words"])
            return Expect(step, self.state, None, {})
        if op == "set_lights":
            self._note("table", s.lights, LIGHT_FAMILIES)
            self._kept(op)
            self.state = s.but(lights=step["table"])
            return Expect(step, self.state, None, {})
        if op == "set_environment":
            self._note("map", s.env, ENV_FAMILIES)
            self._kept(op)
            self.state = s.but(env=step["map"])
            return Expect(step, self.state, None, {})
        family = step["family"]
        events = self.since.pop(family, {})
        if takes_mode(family):                           # (a family that reads `bnd` or `grp` judges the change at its own step)
            events.pop("time", None)
        if family in MASKED:
            events.pop("words", None)
        if op == "pass":
            self.passes[family].append((self.n_steps, s.scene))
            return Expect(step, s, None, events)
        if family in LIGHT_FAMILIES and s.lights is None:
            return Expect(step, s, (-1, "light table"), events)
        if family in ENV_FAMILIES and s.env is None:
            return Expect(step, s, (-1, "environment map"), events)
        if family in MEDIA_FAMILIES and (s.scene is None or s.media is None):
            return Expect(step, s, (-1, "no scene" if s.scene is None else "media table"), events)
        if family == "gather_photons" and s.photons is None:
            return Expect(step, s, (-1, "no photon map"), events)
        if family == "gather_photons" and step.get("normals") and not photon_map(*s.photons)["has_dir"]:
            return Expect(step, s, (-1, "without directions"), events)
        if family in TABLE_FAMILIES and table_refusal(step, s) is not None:
            return Expect(step, s, table_refusal(step, s), events)
        if takes_mode(family) and step["mode"] != "brute":
            now = self.effective_range(step, times)
            if self.block_range is not None and now != self.block_range:
                events["time"] = self.block_range
                self._note("time", self.block_range, [g for g in FAMILIES + ACCUMULATIONS if g != family])
            self.block_range = now
        if family in MASKED:
            now = (s.scene, s.groups)
            if self.masked_words is not None and now[1] != self.masked_words[1]:
                events["words"] = self.masked_words[1]
                self._note("words", self.masked_words[1], [g for g in FAMILIES + ACCUMULATIONS if g != family])
            self.masked_words = now
        return Expect(step, s, None, events)

    def replay(self, steps, oracle=None):
        return [self.apply(st, _times(oracle, st, self.state) if _needs_times(st) else None) for st in steps]


def _needs_times(step):
    return step["op"] == "query" and takes_mode(step["family"]) and step.get("time_range") is None and step["mode"] != "brute"


def _times(oracle, step, state):
    x = inputs(oracle, step, state)
    return x["points"][:, 3] if base(step["family"]) == "nearest" else x["rays"][:, 6]


def _table_alternative(e, event, old):
    """(the stale state | REFUSED | None, why) of one event at a family of TABLE_FAMILIES, or of a grid event at march_media.

    replace, the table gone: the state the upload found -- its grids, textures, patches would still answer.  replace, the table
    set again since: the grid families under a grid that rides the PREVIOUS records' centre (state.packed); albedo under the
    previous records (the untextured path's cold records; under key B the ground is bound and no row reads a record the edit
    changes: key A holds that path); the merged patch queries under the previous records (the sphere records a merge starts from).
    cache_hit / refused / kept: the table cleared, had the upload or the other setter been taken for one that clears it.  grid:
    the keys the family last saw on the media set since.  grids_dropped: the grids before the set_media, at their medium INDICES
    (a stale grid_mask names whatever object the new table lists there).  texture_table / patch_table: the previous key.
    Exempt: hit_patches and the unmerged occluded_patches at `replace` (they read no scene record); the merged occluded_patches at
    patch_table (in a scene with its original ground the ground occludes every probe row whatever the table; unmerged steps hold
    it); `time` and `words` (these families read neither)."""
    f, s, st = e.step["family"], e.state, e.step
    merged = f == "hit_patches_merged" or (f == "occluded_patches" and bool(st.get("merge")))
    if event in ("time", "words"):
        return None, "reads neither the block bounds nor the words"
    if f == "march_media":                               # a grid event at the homogeneous march: which media it leaves out
        if s.media is None or e.refuse is not None:
            return None, "no table either way"
        n = len(MEDIA[s.media][0])
        then = {**s.grids, **old} if event == "grid" else {m: k for m, k in old[1].items() if m < n}
        then = {m: k for m, k in then.items() if k is not None}
        return (None, "the same media have grids") if set(then) == set(s.grids) else (s.but(grids=then), "")
    if event == "replace":
        before = e.events.get("before")
        if e.refuse is not None:
            if before is None or before.scene is None:
                return None, "there was no scene before"
            stale = s.but(media=before.media, grids=before.grids, textures=before.textures, patches=before.patches)
        elif old is None:
            return None, "there was no scene before"
        elif f in GRID_FAMILIES:
            obj = int(media_table(s.media, s.scene)[0][medium_of(s.media, st["who"])])
            if len(records(old)) <= int(media_table(s.media, s.scene)[0].max()):
                return None, "the previous list does not hold these objects"
            if (records(old)[obj] == records(s.scene)[obj]).all():
                return None, "the previous list holds this boundary as it is"
            stale = s.but(packed=old)
        elif f == "albedo" and (s.textures != "A" or ground(records(s.scene)) != 0):
            return None, "under key B (or without a ground) no row reads a record that the edit changes"
        elif f in PATCH_FAMILIES and not merged:
            return None, "reads no scene record"
        else:
            stale = s.but(packed=old)
    elif event in ("cache_hit", "refused", "kept"):
        stale = s.but(grids={}) if f in GRID_FAMILIES else s.but(textures=None) if f == "albedo" else s.but(patches=None)
    elif event == "grid":
        then = {m: k for m, k in {**s.grids, **old}.items() if k is not None}
        m = medium_of(s.media, st["who"]) if s.media else None
        if then.get(m) == s.grids.get(m):
            return None, "this medium's grid is set again to what it was"
        stale = s.but(grids=then)
    elif event == "grids_dropped":
        n = len(MEDIA[s.media][0]) if s.media else 0
        stale = s.but(grids={m: k for m, k in old[1].items() if m < n})
        m = medium_of(s.media, st["who"]) if s.media else None
        if stale.grids.get(m) == s.grids.get(m):
            return None, "this medium's grid is back"
    elif event == "texture_table":
        if old == s.textures:
            return None, "set again to what it was"
        stale = s.but(textures=old)
    elif event == "patch_table":
        if old == s.patches:
            return None, "set again to what it was"
        if f == "occluded_patches" and merged:
            return None, "merged into the spheres' bits: the unmerged steps hold the table"
        stale = s.but(patches=old)
    else:
        return None, "not an event of this family"
    then = table_refusal(st, stale)
    if then is not None:
        return (None, "refused either way") if e.refuse is not None else (REFUSED, "")
    return stale, ""


def alternatives(e):
    """[(event, the state whose answer the step's must differ from | REFUSED | None with the reason it is exempt)] of an Expect.

    replace: the records before the upload.  cache_hit: had the upload been taken for a replacing one, the words and the table
    would be gone -- the masked and the light families can tell, no other answer could change.  refused: the refused list's records,
    had they become the scene.  words / table / map: the previous words, table, map.  The families of SCENE_FREE read no scene and
    are exempt from every upload event; `time` at a block query is judged by time_rows().  `time` and `words` reach every other
    family too (the bounds or the words were rebuilt since it last ran, in buffers that lie beside its own): no restatement of
    theirs can depend on either, so nothing is asked of their inputs, and the GPU test holds their answers all the same.

    The media families: replace with the table gone -- the previous table would answer (REFUSED against an answer); replace with
    the table set again -- the march under a table packed from the PREVIOUS records (the scatter, the sampler and the evaluation
    read sigma, albedo and g alone); cache_hit / refused -- REFUSED, had the upload cleared the table; media_table / phase_g /
    photon_map -- the previous table, g, map (REFUSED where there was none, or where the previous map would refuse the normals).
    `uniform` reads nothing and is exempt from everything; `gather_photons` reads no scene and is exempt from the upload events.

    The grid, texture and patch families, and the grid events at march_media: _table_alternative()."""
    f, s, out = e.step["family"], e.state, []
    for event, old in e.events.items():
        if event == "before":                            # (the state a replacing upload found: `replace` reads it)
            continue
        if f in TABLE_FAMILIES or event in ("grid", "grids_dropped"):
            out.append((event,) + _table_alternative(e, event, old))
        elif event in UPLOAD_EVENTS and f in SCENE_FREE:
            out.append((event, None, "reads no scene"))
        elif f == "uniform":
            out.append((event, None, "reads nothing"))
        elif event in UPLOAD_EVENTS and f in MEDIA_FAMILIES:
            if event == "replace" and s.media is None:   # the table should be gone: the previous one would answer
                out.append((event, REFUSED if e.refuse is None else s.but(media="A"), ""))
            elif event == "replace":                     # set again since: packed from the previous records?
                fits = old is not None and len(records(old)) > int(media_table(s.media, s.scene)[0].max())
                if f != "march_media":
                    out.append((event, None, "reads sigma, albedo and g of the table, no boundary"))
                else:
                    out.append((event, s.but(packed=old) if fits else None, "the previous list does not hold these objects"))
            else:                                        # a cache hit or a refusal taken for a replacing upload clears the table
                out.append((event, REFUSED if s.media is not None else None, "no table either way"))
        elif event == "media_table":
            if f not in MEDIA_FAMILIES or old == s.media:
                out.append((event, None, "set again to what it was"))
            else:
                out.append((event, REFUSED if old is None or s.media is None else s.but(media=old), ""))
        elif event == "phase_g":
            if f not in PHASE_FAMILIES or s.media is None or old == s.phase:
                out.append((event, None, "set again to what it was, or no table"))
            else:
                out.append((event, s.but(phase=old), ""))
        elif event == "photon_map":
            if f != "gather_photons" or old == s.photons:
                out.append((event, None, "built again as it was"))
            else:
                no_dirs = old is not None and e.step.get("normals") and not photon_map(*old)["has_dir"]
                out.append((event, REFUSED if old is None or s.photons is None or no_dirs else s.but(photons=old), ""))
        elif event == "replace":
            if f in LIGHT_FAMILIES and s.lights is None:
                out.append((event, REFUSED if e.refuse is None else s.but(lights="A"), ""))
            elif old is None:
                out.append((event, None, "there was no scene before"))
            else:
                out.append((event, s.but(scene=old), ""))
        elif event == "cache_hit":
            if f in MASKED and s.groups is not None:
                out.append((event, s.but(groups=None), ""))
            elif f in LIGHT_FAMILIES and s.lights is not None:
                out.append((event, REFUSED, ""))
            else:
                out.append((event, None, "a cache hit mistaken for a replacing upload would reset the words and the table alone"))
        elif event == "refused":
            if f in LIGHT_FAMILIES:
                out.append((event, REFUSED if s.lights is not None else None, "no table either way"))
            else:
                out.append((event, s.but(scene=old, groups=None), ""))
        elif event == "words":
            out.append((event, s.but(groups=old) if f in MASKED else None, "reads no words: the restatement cannot depend on them"))
        elif event == "time" and not takes_mode(f):
            out.append((event, None, "reads no block bounds: the restatement cannot depend on the range"))
        elif event == "table":
            out.append((event, None if old == s.lights else REFUSED if old is None else s.but(lights=old), "set again to what it was"))
        elif event == "map":
            out.append((event, None if old == s.env else REFUSED if old is None else s.but(env=old), "set again to what it was"))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _rng(step, salt):
    return np.random.default_rng([int(step["seed"]), salt])


def _states(n, seed):
    return LI.states(n, 0x51A7E + int(seed))


def _tail(make, n):
    """The last n rows of make(k) for k = 0, 1, ... stacked (the input modules put their special rows last)."""
    parts, k = [], 0
    while sum(len(p) for p in parts) < n:
        parts.insert(0, np.asarray(make(k)))
        k += 1
    return np.ascontiguousarray(np.concatenate(parts)[-n:])


def _others_box(recs):
    """The box of the centres of the placeable objects other than a ground sphere."""
    place = recs[placeable(recs)]
    return place[:, 1:4].min(axis=0), place[:, 1:4].max(axis=0)


def _probe_radius(name, recs):
    """Half way between the ground's radius in a scene and in its edited copy (the same number from either)."""
    s = scale(name)
    return abs(recs[0, 9]) + (0.5 if name.endswith("_e") else -0.5) * DELTA * s


def _ground_height(name, recs, x, z, radius):
    c = recs[0, 1:4]
    return c[1] + np.sqrt(radius * radius - (x - c[0]) ** 2 - (z - c[2]) ** 2)


def _isolated(recs, ids):
    """The objects of `ids` with no other of them within three of their radii (by their first centres), if there are eight or more:
    a segment to the centre of one of them is stopped by that object or by none."""
    c, r = recs[ids, 1:4], np.abs(recs[ids, 9])
    gap = np.linalg.norm(c[:, None, :] - c[None, :, :], axis=2) - r[:, None] - r[None, :]
    np.fill_diagonal(gap, np.inf)
    alone = gap.min(axis=1) > 3.0 * r
    return ids[alone] if int(alone.sum()) >= 8 else ids


def _centres(chosen, times):
    """moving_spheres.nim:39-44 per (record, time): center0 + (time - time0) / (time1 - time0) * (center1 - center0)."""
    chosen, times = np.asarray(chosen, dtype=np.float64).reshape(-1, 16), np.asarray(times, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = np.where(chosen[:, 0] == 0, 0.0, (times - chosen[:, 7]) / (chosen[:, 8] - chosen[:, 7]))
        return chosen[:, 1:4] + (chosen[:, 4:7] - chosen[:, 1:4]) * f[:, None]


def _draw_times(rng, step, n):
    lo, hi = step.get("times", (0.0, 1.0))
    return rng.uniform(lo, hi, n)


def _roles(step, recs, n):
    """(probe rows, aimed rows, the object each aimed row aims at) of a step's mix.  "plain": none.  "probe": of every eight rows
    three (0, 2, 4) probe the ground, where the scene has one, and the others aim at an object; "aimed": seven rows of eight aim at
    an object; "movers": three rows of four aim at a mover."""
    i, mix = np.arange(n), step.get("mix", "plain")
    none = np.zeros(0, dtype=np.int64)
    full = np.asarray(recs, dtype=np.float64)
    ok = placeable(full)
    if mix in ("probe", "aimed"):
        probe = np.flatnonzero(np.isin(i % 8, (0, 2, 4))) if ground(full) == 0 and mix == "probe" else none
        aimed = np.setdiff1d(i, probe)
        aimed, pool = (aimed if mix == "probe" else aimed[aimed % 8 != 7]), _isolated(full, np.flatnonzero(ok))
    elif mix == "movers":
        movers = np.flatnonzero(ok & (full[:, 0] == 1))
        probe, aimed, pool = none, np.flatnonzero(i % 4 != 3), movers if movers.size else np.flatnonzero(ok)
    else:
        return none, none, none
    return probe, aimed, pool[_rng(step, 9).integers(0, len(pool), aimed.size)]


def _masks(step, n, recs):
    """One word per row: query_regimes.ray_masks; in a mix the probe and mover rows see every group, and a row aimed at object j has
    by turns (unless the step says full_masks: then it sees every group too) the one-bit mask of j's word under words A, under words B, and a bit that is in neither: whichever words are set or
    were set before, two rows of three see their object under one and not under the other.  Every 16th row keeps its drawn word."""
    m = Q.ray_masks(n, int(step["seed"])).copy()
    probe, aimed, chosen = _roles(step, recs, n)
    keep = np.arange(n) % 16 == 15
    partial = step.get("mix") in ("probe", "aimed") and not step.get("full_masks")
    full = probe if partial else np.concatenate([probe, aimed])
    m[full[~keep[full]]] = Q.ALL
    if partial:
        bit = (chosen + np.array([0, 2, 1])[np.arange(aimed.size) % 3]) % 5
        m[aimed[~keep[aimed]]] = (np.uint32(1) << bit.astype(np.uint32))[~keep[aimed]]
    return m


def ray_inputs(step, name):
    """rays (n, 7) and t_range (n, 2): query_regimes.rays, with the rows of the step's mix (_roles) replaced.  A probe row is a
    vertical segment from above the ground to half way between the original's and the edited copy's ground (range (0.001, 1): one
    of the two stops it); an aimed row starts a few radii from an object's centre at the ray's time and aims at it.  Times are drawn
    from step["times"]."""
    recs, n, rng = records(name), int(step["n"]), _rng(step, 1)
    rays, tr = Q.rays(recs, max(n, 4), int(step["seed"]))
    rays, tr = rays[1:n + 1] if n < 4 else rays[:n], tr[1:n + 1] if n < 4 else tr[:n]     # (row 1 of query_regimes' rays is an aimed one)
    rays[:, 6] = _draw_times(rng, step, n)
    probe, aimed, chosen = _roles(step, recs, n)
    chosen = recs[chosen]
    s = scale(name)
    if probe.size:
        lo, hi = _others_box(recs)
        x, z = rng.uniform(lo[0], hi[0], probe.size), rng.uniform(lo[2], hi[2], probe.size)
        end = _ground_height(name, recs, x, z, _probe_radius(name, recs))
        h = rng.uniform(0.5, 2.0, probe.size) * s
        rays[probe, 0], rays[probe, 1], rays[probe, 2] = x, end + h, z
        rays[probe, 3], rays[probe, 4], rays[probe, 5] = 0.0, -h, 0.0
        tr[probe] = (0.001, 1.0)
    if aimed.size:
        c = _centres(chosen, rays[aimed, 6])
        u = rng.normal(size=(aimed.size, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = c + u * (np.abs(chosen[:, 9]) * rng.uniform(2.0, 3.0, aimed.size))[:, None]
        ok = np.isfinite(o).all(axis=1)
        rays[aimed[ok], 0:3], rays[aimed[ok], 3:6] = o[ok], (c - o)[ok]
        # (a row aimed at an object is the segment to its centre: nothing behind the object answers for it; a mover's ray is open)
        tr[aimed[ok]] = (0.001, np.inf if step.get("mix") == "movers" else 1.0)
    return np.ascontiguousarray(rays), np.ascontiguousarray(tr)


def point_inputs(step, name):
    """points (n, 4): nearest_inputs.points, with the rows of the step's mix replaced.  A probe row lies 0.02 .. 0.2 (x the scale)
    above the ground, an aimed row on or near an object's surface at the point's time."""
    recs, n, rng = records(name), int(step["n"]), _rng(step, 2)
    pts = np.array(NI.points(recs, None, int(step["seed"]), max(n, 8))[:n])
    nan = np.isnan(pts[:, 3])
    pts[:, 3] = np.where(nan, np.nan, _draw_times(rng, step, n))
    probe, aimed, chosen = _roles(step, recs, n)
    chosen = recs[chosen]
    s = scale(name)
    if probe.size:
        lo, hi = _others_box(recs)
        x, z = rng.uniform(lo[0], hi[0], probe.size), rng.uniform(lo[2], hi[2], probe.size)
        pts[probe, 0], pts[probe, 2] = x, z
        pts[probe, 1] = _ground_height(name, recs, x, z, abs(recs[0, 9])) + rng.uniform(0.02, 0.2, probe.size) * s
        pts[probe, 3] = _draw_times(rng, step, probe.size)
    if aimed.size:
        t = _draw_times(rng, step, aimed.size)
        c = _centres(chosen, t)
        u = rng.normal(size=(aimed.size, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        p = c + u * (np.abs(chosen[:, 9]) * rng.choice([0.5, 1.0, 1.25], aimed.size))[:, None]
        ok = np.isfinite(p).all(axis=1)
        pts[aimed[ok], 0:3], pts[aimed[ok], 3] = p[ok], t[ok]
    return np.ascontiguousarray(pts)


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _media_of(state):
    """(records, objects, sigma, albedo, g) a media query reads under `state` (a table packed from state.packed's records)."""
    objects, sigma, albedo = media_table(state.media, state.scene)
    return records(state.packed or state.scene), objects, sigma, albedo, g_vector(state.phase, len(objects))


def media_rays(step, name):
    """rays (n, 7) aimed at the boundary objects of the scene's media tables, as the lamp rows are aimed at lamps: every other row
    at MOVED, every fourth at the mover, the rest at the two others; every fourth origin lies inside its object, the others two
    to three radii out; directions of any length; times in [0, 1].  Without a scene: media_inputs' rays."""
    n, rng = int(step["n"]), _rng(step, 3)
    if name is None:
        return np.ascontiguousarray(MI._rays(int(step["seed"]), n))
    recs, b = records(name), boundaries(name)
    i = np.arange(n)
    chosen = recs[np.where(i % 2 == 0, b[0], np.where(i % 4 == 1, b[1], np.where(i % 8 == 3, b[2], b[3])))]
    t = rng.uniform(0.0, 1.0, n)
    c, r = _centres(chosen, t), np.abs(chosen[:, 9])
    o = c + _unit(rng, n) * (r * np.where(i % 4 == 2, rng.uniform(0.0, 0.8, n), rng.uniform(2.0, 3.0, n)))[:, None]
    d = (c + _unit(rng, n) * (0.3 * r)[:, None]) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * (r * rng.uniform(0.3, 3.0, n))[:, None]
    return np.ascontiguousarray(np.concatenate([o, d, t[:, None]], axis=1))


def _media_inputs(step, state, x):
    """The operands of a media query: rays and tau (media_inputs._taus); for the scatter, the sampler and the evaluation t and
    active of the restated march under the step's state (their infinite budgets made small: more rows collide), 0 where the
    model refuses the step."""
    f, n, seed = step["family"], int(step["n"]), int(step["seed"])
    rays, tau = media_rays(step, state.scene), MI._taus(seed, n)
    if f == "march_media":
        x["rays"], x["tau"] = rays, tau
        return
    t, active = np.zeros(n), np.zeros(n, dtype=np.int64)
    if state.scene is not None and state.media is not None:
        recs, objects, sigma, _, _ = _media_of(state)
        m = MR.march(recs, objects, sigma, rays, np.where(np.isinf(tau), 0.05, tau))
        t, active = m["t"], np.ascontiguousarray(m["active"]).view(np.int64)
    x["active"] = active
    if f == "phase":
        rng = _rng(step, 4)
        out = rays.copy()
        out[:, 3:6] = _unit(rng, n) * rng.uniform(0.3, 3.0, n)[:, None]
        x["rays_in"], x["rays_out"] = rays, out
    else:
        x["rays"], x["t"], x["states"] = rays, np.ascontiguousarray(t), _states(n, seed)


def _gather_inputs(step, x):
    """points (n, 3) drawn by turns from the point sets of the step's maps (those that lie near photons), per-point radii about the
    maps' radius and unit normals where the step asks for them."""
    n, rng = int(step["n"]), _rng(step, 5)
    pools = [photon_map(k)["points"] for k in step["pools"]]
    pts = np.empty((n, 3))
    for k, pool in enumerate(pools):
        rows = np.arange(k, n, len(pools))
        pts[rows] = pool[rng.integers(0, len(pool), rows.size)]
    x["points"] = pts
    if step.get("normals"):
        x["normals"] = _unit(rng, n)
    if step.get("radius"):
        x["radius"] = rng.uniform(0.1, 0.375, n)          # (0.4 .. 1.5 of the larger R: some are clamped to the map's)


def _aim(rng, recs, chosen, t, inside):
    """Origins and directions of rows aimed at the objects `chosen` (indices) at times t: two to three radii out (inside: within
    0.8 radii), towards a point within 0.3 radii of the centre, of any length."""
    n = len(t)
    rec = recs[chosen]
    c, r = _centres(rec, t), np.abs(rec[:, 9])
    o = c + _unit(rng, n) * (r * np.where(inside, rng.uniform(0.0, 0.8, n), rng.uniform(2.0, 3.0, n)))[:, None]
    d = (c + _unit(rng, n) * (0.3 * r)[:, None]) - o
    return o, d / np.linalg.norm(d, axis=1, keepdims=True) * (r * rng.uniform(0.3, 3.0, n))[:, None]


def _grid_inputs(step, state, x):
    """The grid march: rays aimed at the boundary object of the step's medium, every fourth origin inside it, tau finite and (one
    in five) infinite.  The lookup: points within 0.55 (every other row), 1.0 and 1.3 radii of the boundary's centre at the point's
    time, on every axis -- inside and outside the sphere and the box.  Without a scene, a table or such a medium: aimed at MOVED (the call is refused)."""
    n, seed, rng = int(step["n"]), int(step["seed"]), _rng(step, 6)
    if state.scene is None:
        rays = np.ascontiguousarray(MI._rays(seed, n))
        x.update({"rays": rays, "tau": MI._taus(seed, n)} if step["family"] == "march_media_grid" else {"points": np.ascontiguousarray(rays[:, [0, 1, 2, 6]])})
        return
    recs = records(state.scene)
    m = medium_of(state.media, step["who"]) if state.media is not None else None
    obj = int(media_table(state.media, state.scene)[0][m]) if m is not None and 0 <= m < len(MEDIA[state.media][0]) else MOVED
    t = rng.uniform(0.0, 1.0, n)
    if step["family"] == "march_media_grid":
        o, d = _aim(rng, recs, np.full(n, obj), t, np.arange(n) % 4 == 2)
        x["rays"], x["tau"] = np.ascontiguousarray(np.concatenate([o, d, t[:, None]], axis=1)), MI._taus(seed, n) * 2.0
    else:
        c = _centres(recs[np.full(n, obj)], t)
        reach = np.array([0.55, 1.3, 0.55, 1.0])[np.arange(n) % 4] * abs(recs[obj, 9])   # (0.55: every such point lies inside the sphere)
        x["points"] = np.ascontiguousarray(np.concatenate([c + rng.uniform(-1.0, 1.0, (n, 3)) * reach[:, None], t[:, None]], axis=1))


def _albedo_inputs(step, name, x):
    """Hit records of the hit restatement on rows that, of every eight, probe the ground three times (0, 2, 4: vertical rays from
    above it; without a ground they aim at objects), aim at MOVED twice (1, 5), start inside an object once (3: a back face), aim at
    an object once (6) and point away from the scene once (7: a record with no such object)."""
    n, rng = int(step["n"]), _rng(step, 7)
    recs = records(name)
    i = np.arange(n)
    pool = np.flatnonzero(placeable(recs))
    chosen = np.where(np.isin(i % 8, (1, 5)), MOVED, pool[rng.integers(0, len(pool), n)])
    t = rng.uniform(0.0, 1.0, n)
    o, d = _aim(rng, recs, chosen, t, i % 8 == 3)
    away = i % 8 == 7
    d[away] = -d[away]
    if ground(recs) == 0:
        probe = np.flatnonzero(np.isin(i % 8, (0, 2, 4)))
        lo, hi = _others_box(recs)
        px, pz = rng.uniform(lo[0], hi[0], probe.size), rng.uniform(lo[2], hi[2], probe.size)
        h = rng.uniform(0.5, 2.0, probe.size) * scale(name)
        o[probe] = np.stack([px, _ground_height(name, recs, px, pz, abs(recs[0, 9])) + h, pz], axis=1)
        d[probe] = np.stack([np.zeros(probe.size), -h, np.zeros(probe.size)], axis=1)
    ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
    o[~ok], d[~ok] = 0.0, 1.0
    x["hits"] = np.ascontiguousarray(H.world_hit(recs, np.concatenate([o, d, t[:, None]], axis=1)))


def _patch_inputs(step, name, x):
    """rays and t_range: of every eight rows seven probe the floor the patch tables lie on (vertical segments from 0.5 to 2 scales
    above floor_height down to it, range (0.001, 1): a patch, the original's ground or nothing stops them) and one is
    query_regimes' ray; the mask by the step: none, PATCH_MASK, or one word of query_regimes.ray_masks per ray."""
    n, rng = int(step["n"]), _rng(step, 8)
    recs = records(name)
    rays, tr = Q.rays(recs, max(n, 8), int(step["seed"]))
    rays, tr = np.array(rays[:n]), np.array(tr[:n])
    probe = np.flatnonzero(np.arange(n) % 8 != 7)
    x0, x1, z0, z1 = patch_region(name)
    px, pz = rng.uniform(x0, x1, probe.size), rng.uniform(z0, z1, probe.size)
    h = rng.uniform(0.5, 2.0, probe.size) * scale(name)
    rays[probe, 0], rays[probe, 1], rays[probe, 2] = px, floor_height(name, px, pz) + h, pz
    rays[probe, 3], rays[probe, 4], rays[probe, 5] = 0.0, -h, 0.0
    tr[probe] = (0.001, 1.0)
    x["rays"], x["t_range"] = np.ascontiguousarray(rays), np.ascontiguousarray(tr)
    if step.get("masks") == "rays":
        x["masks"] = Q.ray_masks(n, int(step["seed"])).copy()


def patch_mask(step, x):
    """The mask operand of a patch step: None, the scalar, or the per-ray words."""
    return {None: None, "scalar": PATCH_MASK, "rays": x.get("masks")}[step.get("masks")]


def inputs(oracle, step, state):
    """The operands of a query, render or pass step under `state`, as numpy arrays: drawn from the step's seed, the scene's
    records and (scatter, bsdf) the restatement's own hits."""
    f, seed = step["family"], int(step["seed"])
    n = int(step.get("n", 0))
    name = state.scene
    x = {}
    if base(f) in RAY_FAMILIES or f == "scatter":
        x["rays"], x["t_range"] = ray_inputs(step, name)
        if f in ("bounce", "bounce_m", "radiance", "scatter"):
            x["states"] = _states(n, seed)
        if f == "scatter":
            x["hits"] = H.world_hit(records(name), x["rays"])
    elif base(f) == "nearest":
        x["points"] = point_inputs(step, name)
        if step.get("dmax"):
            x["dmax"] = NI.point_d_max(n, 0.3 * scale(name), seed)
    elif f == "bsdf":
        recs = records(name)
        rin, raw, rout = (np.ascontiguousarray(a[:n]) for a in BI.random_items(recs, seed))
        if step.get("mix") == "probe":                  # every even item lies on the ground, whose material the edit changes
            raw.view(np.int32)[0::2, 14] = 0
        x["rays_in"], x["hits"], x["rays_out"] = rin, raw, rout
    elif f in ("sample_lights", "light_pdf"):
        lights, _ = light_table(state.lights or "A")
        x["points"] = _tail(lambda k: LI.points(records(name), lights, seed + k), n)
        x["states"] = _states(n, seed)
        x["objects"] = np.where(np.arange(n) % 5 == 4, 1, lights[np.arange(n) % len(lights)]).astype(np.int32)
    elif f == "emit_lights":
        x["states"] = _states(n, seed)
    elif f == "connect_camera":
        cam24 = CI.camera(oracle, ("pinhole", "lens", "tilted", "wide")[seed % 4])
        x["cam24"], x["frame"] = cam24, CI.FRAMES[seed % 3]
        x["points"] = _tail(lambda k: CI.points(cam24, *CI.FRAMES[seed % 3], seed=seed + k), n)
        x["states"] = _states(n, seed)
    elif f == "environment":
        x["rays"] = _tail(lambda k: EI.directions(None, seed + k), n)
    elif f == "sample_environment":
        x["points"] = _tail(lambda k: EI.points_and_states(seed + k)[0], n)
        x["states"] = _tail(lambda k: EI.points_and_states(seed + k)[1], n)
    elif f == "deposit":
        c, p = DI.case(DI.CASES[seed % len(DI.CASES)], 1.0, seed)
        x["colors"], x["pixels"] = np.ascontiguousarray(c[:n]), np.ascontiguousarray(p[:n])
    elif f in MEDIA_FAMILIES:
        _media_inputs(step, state, x)
    elif f == "gather_photons":
        _gather_inputs(step, x)
    elif f == "uniform":
        x["states"] = _states(n, seed)
    elif f in GRID_FAMILIES:
        _grid_inputs(step, state, x)
    elif f in TABLE_FAMILIES and name is None:           # (refused: no scene)
        x["rays"], x["t_range"] = np.ascontiguousarray(MI._rays(seed, n)), np.tile([0.001, 1.0], (n, 1))
        x["hits"] = TR.make_hits(np.zeros((n, 3)), np.zeros((n, 3)), -1, 0)
    elif f == "albedo":
        _albedo_inputs(step, name, x)
    elif f in PATCH_FAMILIES:
        _patch_inputs(step, name, x)
    elif f in ("render",) + ACCUMULATIONS:
        recs = records(name)                            # (the camera looks at the objects: a ground sphere does not stretch its box)
        x["camera"] = R.camera(regime(name), "outside", recs[1:] if ground(recs) == 0 else recs)
    if f in MASKED:
        x["masks"] = _masks(step, n, records(name))
    return x


# ---- answers ----------------------------------------------------------------------------------------------------------------------------
def _hit_fields(raw, prefix=""):
    f = H.fields(np.ascontiguousarray(raw).reshape(-1, 8))
    lead = np.asarray(raw).shape[:-1]
    return {prefix + k: np.ascontiguousarray(v).reshape(lead + v.shape[1:]) for k, v in f.items()}


def answer(oracle, step, x, state):
    """The family's restatement on the operands x under `state`: a dict of arrays whose first axis is the batch (a render's: the
    canvas).  A deposit answers with what it adds to an empty film."""
    f = step["family"]
    recs = records(state.scene) if state.scene is not None else None
    g = words(state.groups, len(recs)) if recs is not None else None
    masks = x.get("masks")
    if base(f) == "hit":
        raw = M.world_hit(recs, g, x["rays"], masks, x["t_range"]) if f in MASKED else H.world_hit(recs, x["rays"], x["t_range"])
        return _hit_fields(raw)
    if base(f) == "occluded":
        raw = M.world_hit(recs, g, x["rays"], masks, x["t_range"]) if f in MASKED else H.world_hit(recs, x["rays"], x["t_range"])
        return {"occluded": (H.fields(raw)["object"] >= 0).astype(np.int32)}
    if base(f) == "crossings":
        k = int(step["k"])
        w = X.masked_crossings(recs, g, x["rays"], masks, k, x["t_range"]) if f in MASKED else X.crossings(recs, x["rays"], k, x["t_range"])
        out = {q: w[q] for q in ("t", "object", "which", "count")}
        if step.get("records"):
            out.update(_hit_fields(X.records(recs, x["rays"], w), "hits_"))
        return out
    if base(f) == "nearest":
        k, dmax = int(step["k"]), x.get("dmax")
        w = N.masked_nearest(recs, g, x["points"], masks, k, dmax) if f in MASKED else N.nearest(recs, x["points"], k, dmax)
        return {q: w[q] for q in ("distance", "object", "inside", "count")}
    if base(f) == "bounce":
        w = M.step(oracle, recs, g, x["rays"], x["states"], masks) if f in MASKED else B.step(oracle, recs, x["rays"], x["states"])
        out = _hit_fields(w["raw"])
        out.update({q: w[q] for q in ("status", "attenuation", "rays", "states")})
        return out
    if f == "scatter":
        w = B.scatter(oracle, recs, x["rays"], x["hits"], x["states"])
        return {q: w[q] for q in ("status", "attenuation", "rays", "states")}
    if f == "radiance":
        color, st = RR.radiance(oracle, recs, x["rays"], x["states"], RADIANCE_DEPTH)
        return {"color": color, "states": st}
    if f == "bsdf":
        return BR.evaluate(recs, x["rays_in"], x["hits"], x["rays_out"])
    if f in LIGHT_FAMILIES:
        lights, weights = light_table(state.lights)
        if f == "sample_lights":
            w = LR.sample(oracle, recs, lights, weights, x["points"], x["states"], None, LR.BY_SOLID_ANGLE)
            return {q: w[q] for q in ("rays", "pdf", "light", "dist", "states")}
        if f == "light_pdf":
            return {"pdf": LR.pdf(recs, lights, weights, x["points"], x["objects"], None, LR.BY_SOLID_ANGLE)}
        w = CR.emit(oracle, recs, lights, weights, x["states"], *step["shutter"])
        return {q: w[q] for q in ("rays", "normal", "light", "pdf", "states")}
    if f == "connect_camera":
        w = CR.connect(oracle, x["cam24"], *x["frame"], x["points"], x["states"])
        return {q: w[q] for q in ("rays", "pixel", "factor", "lens", "states")}
    if f == "environment":
        w = ER.evaluate(env_map(state.env)[2], x["rays"])
        return {q: w[q] for q in ("color", "pdf", "texel")}
    if f == "sample_environment":
        w = ER.sample(oracle, env_map(state.env)[2], x["points"], x["states"])
        return {q: w[q] for q in ("rays", "pdf", "texel", "color", "states")}
    if f == "deposit":
        w = D.deposit(x["colors"], x["pixels"], FILM[0] * FILM[1], 1.0)
        return {q: w[q] for q in ("sums", "moments", "counts")}
    if f in MEDIA_FAMILIES:
        mrecs, objects, sigma, albedo, gs = _media_of(state)
        if f == "march_media":                          # (a medium with a grid takes no part: grid_restatement's sub-table)
            w = GR.march_with_grids(mrecs, objects, sigma, sorted(state.grids), x["rays"], x["tau"]) if state.grids else \
                MR.march(mrecs, objects, sigma, x["rays"], x["tau"])
            return {q: w[q] for q in ("status", "t", "depth", "rho", "active")}
        if f == "scatter_media":
            w = MR.scatter(oracle, sigma, albedo, x["rays"], x["t"], x["active"], x["states"])
            return {q: w[q] for q in ("rays", "attenuation", "states")}
        if f == "sample_phase":
            w = PR.sample(oracle, sigma, albedo, gs, x["rays"], x["t"], x["active"], x["states"])
            return {q: w[q] for q in ("rays", "attenuation", "pdf", "states")}
        return PR.evaluate(sigma, albedo, gs, x["rays_in"], x["active"], x["rays_out"])
    if f == "uniform":
        u, st = MR.uniforms(oracle, x["states"], int(step["draws"]))
        return {"u": u, "states": st}
    if f in GRID_FAMILIES:
        mrecs, objects, sigma, _, _ = _media_of(state)
        grid = _grid(state, medium_of(state.media, step["who"]))
        if f == "march_media_grid":
            w = GR.march(mrecs, objects, sigma, grid, x["rays"], x["tau"])
            return {q: w[q] for q in ("status", "t", "depth", "rho", "active", "cell")}
        cell, value = GR.density(mrecs, objects, grid, x["points"])
        return {"cell": cell, "density": value}
    if f == "albedo":
        tex, binding = texture_table(state.textures, state.scene)
        return TR.evaluate(records(state.packed or state.scene), tex, binding, x["hits"])
    if f in PATCH_FAMILIES:
        table, mask = patch_table(state.patches, state.scene), patch_mask(step, x)
        srecs = records(state.packed or state.scene)
        if f == "occluded_patches":
            start = (H.fields(H.world_hit(srecs, x["rays"], x["t_range"]))["object"] >= 0).astype(np.int32) if step.get("merge") else None
            return {"occluded": PT.occluded(table, x["rays"], x["t_range"], mask, merge=start)}
        w = PT.merge(srecs, table, x["rays"], x["t_range"], mask) if f == "hit_patches_merged" else PT.hit(table, x["rays"], x["t_range"], mask)
        out = _hit_fields(w["raw"])
        out.update(patch=w["patch"], uv=w["uv"])
        return out
    if f == "gather_photons":
        m = photon_map(*state.photons)
        w = PH.gather(m["stored"], x["points"], x.get("normals"), x.get("radius"), step["kernel"], 1.0)
        # PhotonGather.irradiance: sums / scale times the kernel's normalisation over paths, with r = min(radius, R); 0 where
        # nothing was accepted
        r = np.minimum(x["radius"], m["radius"]) if "radius" in x else np.full(len(x["points"]), m["radius"])
        c = (2.0 if step["kernel"] == "epanechnikov" else 1.0) / (np.pi * PATHS * m["scale"])
        w["irradiance"] = w["sums"] * np.where(w["count"] > 0, c / (r * r), 0.0)[:, None]
        return w
    ocam = R.oracle_camera(oracle, x["camera"])
    if f == "render":
        px = oracle.render(R.H, R.W, R.SPP, ocam, recs, max_depth=R.DEPTH, seeding=int(step["seeding"]), math=oracle.MATH_PORTABLE,
                           accum=int(step["seeding"])).pixels
        return {"pixels": px.reshape(-1, 3)}
    if f == "progressive":                               # one pass: the sums of its three samples
        sums, _ = oracle.accumulate(R.H, R.W, int(step["first"]), 3, ocam, recs, max_depth=R.DEPTH)
        return {"sums": sums.reshape(-1, 3)}
    if f == "pixel_progressive":                         # the canvas after this pass (both passes see one scene: the model checks)
        px = oracle.render(R.H, R.W, int(step["first"]) + 3, ocam, recs, max_depth=R.DEPTH, seeding=0, math=oracle.MATH_PORTABLE, accum=0).pixels
        return {"pixels": px.reshape(-1, 3)}
    raise KeyError(f)


def differing_rows(a, b):
    """Per row of the batch: does any field differ in a bit (float64: a NaN on both sides counts as equal)?"""
    out = None
    for k, va in a.items():
        va, vb = np.ascontiguousarray(va), np.ascontiguousarray(b[k])
        assert va.shape == vb.shape, k
        if va.dtype == np.float64:
            d = (va.view(np.uint64) != np.ascontiguousarray(vb, dtype=np.float64).view(np.uint64)) & ~(np.isnan(va) & np.isnan(vb))
        else:
            d = va != vb
        d = d.reshape(d.shape[0], -1).any(axis=1)
        out = d if out is None else (out | d)
    return out


def time_rows(step, x, want, state, old_range):
    """Rows whose answer a block box built for the OLD time range could lose: the answering object (closest hit, first crossing,
    nearest neighbour) is a mover, the row's time lies outside the old range, and the mover's centre at that time lies further from
    where it is over the old range than its radius -- a necessary condition, restated from moving_spheres.nim's centre alone."""
    recs = records(state.scene)
    f = base(step["family"])
    t = x["points"][:, 3] if f == "nearest" else x["rays"][:, 6]
    if "object" not in want:                             # occluded, radiance: the object of the closest hit
        want = answer(None, dict(step, family="hit_m" if step["family"] in MASKED else "hit"), x, state)
    obj = np.asarray(want["object"]).reshape(len(t), -1)[:, 0]
    lo, hi = old_range
    out = np.zeros(len(t), dtype=bool)
    for i in np.flatnonzero((obj >= 0) & ((t < lo) | (t > hi))):
        rec = recs[obj[i]]
        if rec[0] != 1 or rec[7] == rec[8]:
            continue
        with np.errstate(all="ignore"):
            now, near = _centres([rec, rec], [t[i], min(max(t[i], lo), hi)])
        out[i] = np.linalg.norm(now - near) > abs(rec[9])
    return out


# ---- scripts -----------------------------------------------------------------------------------------------------------------------------
class _Builder:
    """Appends steps (a gather's normals, per-point radius and kernel, a build's operand kind and list go by turns too).  Mode, K and max_distance are drawn independently from the builder's generator, and the
    operand kind (device tensors or numpy arrays) and the batch size go by turns per family; the operands' mix follows from what the model says happened since the family last
    ran."""

    def __init__(self, seed):
        self.rng = np.random.default_rng([seed, 77])
        self.steps, self.model = [], Model()
        self.seed = 1000 * seed
        self.last_range = (0.0, 1.0)                      # the range the library's bounds are keyed on
        self.range_key = (0.0, 1.0)                       # ... and the entry of TIME_RANGES it came from
        self.open, self.turns = {}, {}

    def add(self, **step):
        self.steps.append(step)
        self.model.apply(step)
        return step

    def upload(self, scene, bad=False):
        self.add(op="upload", scene=scene, bad=bad)

    def groups(self, key):
        self.add(op="set_groups", words=key)

    def lights(self, key):
        self.add(op="set_lights", table=key)

    def environment(self, key):
        self.add(op="set_environment", map=key)

    def media(self, key, bad=None):
        """set_media: a named table, None (the empty one), or a refused one (bad: a key of BAD_MEDIA)."""
        self.add(op="set_media", table=key, bad=bad)

    def phase(self, key, wrong_count=False):
        """set_media_phase: a named g vector or None; wrong_count: one value too few."""
        self.add(op="set_media_phase", g=key, wrong_count=wrong_count)

    def photons(self, key):
        """build_photons: from numpy or device tensors by turns, with a list every other pair of turns."""
        t = self.turns["build_photons"] = self.turns.get("build_photons", 0) + 1
        self.add(op="build_photons", map=key, host=bool(t % 2), listed=bool((t // 2) % 2))

    def grid(self, who, key):
        """set_media_grid: a named grid (or one of BAD_GRIDS) on the medium a role names, or on the int itself; None removes it."""
        self.add(op="set_media_grid", who=who, grid=key)

    def textures(self, key, bad=None, count_of=None):
        """set_textures: a named table or None (the empty one); bad: "long", "outside"; count_of: the binding built for that scene."""
        self.add(op="set_textures", table=key, bad=bad, count_of=count_of)

    def patches(self, key, bad=None, of=None):
        """set_patches: a named table or None (the empty one); bad = "material" (of: a material valid for that scene)."""
        self.add(op="set_patches", table=key, bad=bad, of=of)

    def _draw(self, values):
        return values[int(self.rng.integers(len(values)))]

    def query(self, family, **kw):
        self.seed += 1
        m = self.model
        # what the step's rows must be able to tell: an upload, a table or a map since the family last ran, other words
        pending = {k: v for k, v in m.since.get(family, {}).items() if k not in ("time", "words")}
        if family in MASKED and m.masked_words is not None and m.masked_words[1] != m.state.groups:
            pending["words"] = True
        self.turns[family] = self.turns.get(family, int(self.rng.integers(2))) + 1
        step = dict(op="query", family=family, seed=self.seed, host=bool(self.turns[family] % 2))   # (by turns per family)
        step["n"] = 64 if family in SLOW else BATCHES[self.turns[family] % len(BATCHES)]   # (by turns too: five sizes, two kinds)
        near = partner(m.state.scene) if m.state.scene else None   # (the ground probes tell a scene from its edited copy alone)
        scenes = {pending[k] for k in ("replace", "refused") if k in pending}
        step["mix"] = "plain" if not pending else "probe" if near is not None and near in scenes else "aimed"
        if family in MASKED and pending and not {"words", "cache_hit"} & set(pending):
            step["full_masks"] = True                     # (no words to tell apart: every aimed row sees its object)
        if step["n"] == 1 and (pending or "time_range" in kw):   # (a quarter of one row: the batch of one comes at another step)
            step["n"] = 65
        if takes_mode(family):
            step["mode"] = self._draw(MODES)
            step["time_range"] = self.last_range
            step["times"] = (0.0, 1.0)
        if base(family) == "crossings":
            step["k"] = self._draw((4, 16))
        if base(family) == "nearest":
            step["k"] = self._draw((2, 16))
            step["dmax"] = bool(self.rng.random() < 0.4) and not pending and "time_range" not in kw
        if family == "emit_lights":
            step["shutter"] = self._draw(CI.TIME_RANGES)
        if family == "uniform":
            step["draws"] = self._draw((1, 3, 16))
        if family == "gather_photons":                   # by turns: normals, a per-point radius, the kernel
            t, cur, old = self.turns[family], m.state.photons, pending.get("photon_map")
            pools = tuple(dict.fromkeys(k[0] for k in (cur, old) if k is not None and k[0] != "E"))
            step["pools"] = pools or ("L", "S")          # the points of the map and of the one before it (the empty one has none)
            has_dir = cur is None or photon_map(*cur)["has_dir"]
            relisted = cur is not None and old is not None and cur[0] == old[0]   # (the same photons through a list: half are gone)
            step["normals"] = bool((t // 2) % 2) and (has_dir or not pending) and not relisted   # (a refusal settles nothing pending)
            step["radius"], step["kernel"] = t % 3 == 0, ("constant", "epanechnikov")[(t // 4) % 2]
        if family in GRID_FAMILIES:                      # by turns the roles whose medium has a grid; one set or dropped since first
            st, t = m.state, self.turns[family]
            has = [w for w in ROLES if st.media and medium_of(st.media, w) in st.grids]
            was = {**pending.get("grids_dropped", (None, {}))[1], **pending.get("grid", {})}
            first = [w for w in ROLES if st.media and medium_of(st.media, w) in was and was[medium_of(st.media, w)] != st.grids.get(medium_of(st.media, w))]
            if "replace" in pending and "moved" in has:  # (the edit moves MOVED's centre, not the mover's)
                first = ["moved"]
            step["who"] = (first or has or ["moved"])[t % len(first or has or ["moved"])]
        if family in PATCH_FAMILIES:                     # by turns: every group, one scalar mask, a word per ray
            t = self.turns[family]
            step["masks"] = None if {"patch_table", "replace", "refused"} & set(pending) else (None, "scalar", "rays")[t % 3]   # (no words between the row and what it must tell)
            if family == "occluded_patches":             # merged where a scene event is pending, unmerged where a table is, else by turns
                step["merge"] = bool({"replace", "refused"} & set(pending)) or ("patch_table" not in pending and bool((t // 3) % 2))
        step.update(kw)
        if base(family) == "crossings":
            step["records"] = step["k"] == 4
        if takes_mode(family) and "time_range" in kw:     # a change of the range: blocks asked for, rows aimed at movers, timed at the
            new = kw["time_range"]                        # end of the new range that lies furthest from the old one
            step["mode"] = kw.get("mode", self._draw(("auto", "blocks")))
            step["mix"] = "movers"
            lo, hi = self.last_range
            if new is None:
                step["times"] = (hi + 3.0, hi + 4.0)   # (later, not earlier: dense's movers rise with time and would sink into the ground)
            else:
                below, above = lo - new[0], new[1] - hi
                step["times"] = (new[0], new[0] + 0.25 * max(below, 0.0)) if below >= above else (new[1] - 0.25 * max(above, 0.0), new[1])
        self.steps.append(step)
        times = _times(None, step, m.state) if _needs_times(step) else None
        if takes_mode(family) and step["mode"] != "brute":   # (the range the library will key its bounds on: later steps name it)
            self.last_range = m.effective_range(step, times)
        m.apply(step, times)
        return step

    def render(self, seeding, accel):
        self.seed += 1
        self.add(op="render", family="render", seed=self.seed, seeding=seeding, accel=accel)

    def accumulate(self, which):
        """The next pass (three samples) of an accumulation, opened at its first pass."""
        first = self.open.get(which, 0)
        self.open[which] = first + 3
        self.add(op="pass", family=which, seed=0, first=first)

    def every_family(self, skip=()):
        for f in QUERY_FAMILIES:
            if f not in skip:
                self.query(f)
        self.render(self._draw((0, 1)), self._draw((0, 3)))

    def variants(self):
        """Every combination the families name, on device tensors and through the host twins, plain and masked: crossings with
        K = 4 (records) and 16, nearest with K = 2 and 16, with and without max_distance."""
        for f in ("crossings", "crossings_m"):
            for k in (4, 16):
                for host in (False, True):
                    self.query(f, k=k, host=host)
        for f in ("nearest", "nearest_m"):
            for k in (2, 16):
                for dmax in (False, True):
                    for host in (False, True):
                        self.query(f, k=k, dmax=dmax, host=host)

    def singles(self):
        """A batch of one for every family whose restatement does not loop in Python (those run 64 rays)."""
        for f in QUERY_FAMILIES:
            if f not in SLOW:
                self.query(f, n=1)

    def new_range(self, families):
        """A block query of each given family under the next time range."""
        for f in families:
            nxt = TIME_RANGES[(TIME_RANGES.index(self.range_key) + 1) % len(TIME_RANGES)]
            self.range_key = nxt
            m = self.model
            if m.since.get(f) or (f in MASKED and m.masked_words is not None and m.masked_words[1] != m.state.groups):
                self.query(f)                             # (what else is pending for the family is settled first, on its own rows)
            self.query(f, time_range=nxt)

    def new_words(self, families=MASKED):
        """A masked query of each given family under other group words than the masked query before it saw."""
        for f in families:
            keys = [k for k in (None,) + GROUPS if k != self.model.state.groups]
            self.groups(self._draw(keys))
            self.query(f)


    def new_media(self):
        """Every media family under another table than it last saw; the phase families under another g: set where it was 0, reset
        by set_media, and one vector after the other."""
        other = lambda: "B" if self.model.state.media == "A" else "A"
        for f in MEDIA_FAMILIES:
            self.media(other())
            self.query(f)
        for f in PHASE_FAMILIES:
            self.phase("P")
            self.query(f)
            self.media(other())                          # g is 0 again
            self.query(f)
            self.phase("Q")
            self.query(f)
            self.phase("P")
            self.query(f)

    def new_map(self):
        """A gather behind every rebuild: the large map, the smaller one without directions (a gather with normals is refused),
        the empty one, the large one again."""
        for key in ("L", "S", "E", "L"):
            self.photons(key)
            self.query("gather_photons")
            if key == "S":
                self.query("gather_photons", normals=True)

    def new_grids(self):
        """The grid families and the homogeneous march behind every change of the grids: none yet (refused), G1 on MOVED's medium and
        G2 on the mover's, G3 (G1's cell count in another shape) and G2 (fewer cells) in G1's place, kept behind set_media_phase and
        set_lights, MOVED's removed (the mover's stays), the refused setters (each behind a step that could tell), and the other
        media table: every grid dropped, and a medium index names another object.  Leaves G1 and G2 on the other table."""
        other = lambda: "B" if self.model.state.media == "A" else "A"
        both = lambda: [self.query(f, who=w) for f in GRID_FAMILIES for w in ROLES]
        self.media(other())
        both()                                            # refused: no grid yet
        self.grid("moved", "G1"), self.grid("mover", "G2")
        both(), self.query("march_media")
        self.query("media_density", who="moved", n=1)
        for key in ("G3", "G2"):
            self.grid("moved", key)
            for f in GRID_FAMILIES:
                self.query(f, who="moved")
        self.phase("Q" if self.model.state.phase == "P" else "P"), self.lights("B" if self.model.state.lights == "A" else "A")
        both()                                            # kept
        self.grid("moved", None)
        both(), self.query("march_media")                 # MOVED's is refused, the mover's answers, the march counts MOVED again
        self.grid("moved", "G1")
        for f in GRID_FAMILIES:
            self.query(f, who="moved")
        self.grid(7, "G1"), self.grid("moved", "dims"), self.grid("moved", "nan"), self.grid("mover", "negative")   # refused
        both()
        self.media(other())                               # every grid dropped; MOVED's index is the mover's old one
        both(), self.query("march_media")
        self.grid("moved", "G1"), self.grid("mover", "G2")
        both(), self.query("march_media")

    def new_textures(self):
        """albedo behind every change of the table: the other key and back, the refused tables, the empty one (refused), a key again."""
        other = lambda: "B" if self.model.state.textures == "A" else "A"
        for _ in range(2):
            self.textures(other())
            self.query("albedo")
        self.textures(other(), bad="long"), self.textures(other(), bad="outside")   # refused: nothing changes
        self.query("albedo")
        self.textures(None)
        self.query("albedo")                              # refused
        self.textures("B")
        self.query("albedo")
        self.textures("A")
        self.query("albedo")

    def new_patches(self):
        """The patch families behind every change of the table: the other key and back, a refused table, the empty one, a key again."""
        other = lambda: "B" if self.model.state.patches == "A" else "A"
        for _ in range(2):
            self.patches(other())
            for f in PATCH_FAMILIES:
                self.query(f)
        self.patches(other(), bad="material")             # refused: nothing changes
        for f in PATCH_FAMILIES:
            self.query(f)
        self.patches(None)
        for f in PATCH_FAMILIES:
            self.query(f)                                 # refused
        self.patches("B")                                 # the smaller table first: then the larger behind it
        for f in PATCH_FAMILIES:
            self.query(f)
        self.patches("A")
        for f in PATCH_FAMILIES:
            self.query(f)

    def twins(self):
        """Every new family through its host twin, behind a larger device call of another family."""
        for f in NEW_FAMILIES:
            self.query("hit", host=False, n=257)
            self.query(f, host=True, **({} if f in SLOW else {"n": 63}))

    def queued(self):
        """A render, a query on device tensors, then a setter of the table that query reads: no host step in between.  The grid,
        texture and patch setters too: each replaces a device buffer the query in front of it reads."""
        st = self.model.state
        for f, setter in (("march_media", lambda: self.media("B" if st.media == "A" else "A")), ("sample_phase", lambda: self.phase("Q")),
                          ("gather_photons", lambda: self.photons("S")), ("sample_lights", lambda: self.lights("B" if st.lights == "A" else "A")),
                          ("environment", lambda: self.environment("n16" if st.env == "n4" else "n4")),
                          ("march_media_grid", lambda: self.grid("moved", "G2" if st.grids.get(medium_of(st.media, "moved")) == "G1" else "G1")),
                          ("media_density", lambda: self.grid("mover", "G3" if st.grids.get(medium_of(st.media, "mover")) == "G2" else "G2")),
                          ("albedo", lambda: self.textures("B" if st.textures == "A" else "A")),
                          ("hit_patches", lambda: self.patches("B" if st.patches == "A" else "A")),
                          ("occluded_patches", lambda: self.patches("B" if st.patches == "A" else "A"))):
            if f in GRID_FAMILIES and not self.model.state.grids:   # (the media setter above dropped them)
                self.grid("moved", "G1"), self.grid("mover", "G2")
            kw = {"who": "moved" if f == "march_media_grid" else "mover"} if f in GRID_FAMILIES else {}   # (the medium the setter writes)
            self.render(0, 3)
            self.query(f, host=False, **kw)
            st = self.model.state
            setter()
            self.query(f, **kw)


def _settle(b, groups="A", lights="A", env=None):
    """Words, a light table, the media table of the same name with a g vector (P for A, Q for B), the texture and the patch table of
    that name, and an environment map where asked.  No grids: a medium with a grid leaves the homogeneous march, whose rows are
    aimed at MOVED; new_grids() and the steps around the uploads set them."""
    b.groups(groups)
    b.lights(lights)
    b.media(lights)
    b.phase("P" if lights == "A" else "Q")
    b.textures(lights)
    b.patches(lights)
    if env is not None:
        b.environment(env)


def _same_size(b, scene):
    """Uploads that keep the object count: a scene and its edited copy, there and back."""
    other = partner(scene)
    b.query("uniform")                                    # needs no scene
    b.query("gather_photons")                             # refused: no map yet
    b.query("march_media"), b.query("phase")              # refused: no scene yet
    b.media("A"), b.phase("P")                            # refused: no scene yet
    b.grid("moved", "G1"), b.textures("A"), b.patches("A")   # refused: no scene yet
    b.query("march_media_grid"), b.query("albedo"), b.query("hit_patches")   # refused: no scene yet
    b.photons("L")                                        # needs no scene
    b.query("gather_photons")
    b.upload(scene)
    b.query("sample_lights")                              # refused: no table yet
    b.query("environment")                                # refused: no map yet
    b.query("scatter_media"), b.phase("P")                # refused: no table yet
    b.grid("moved", "G1"), b.query("media_density")       # refused: no media table yet
    b.query("albedo"), b.query("occluded_patches"), b.query("hit_patches_merged")   # refused: no table yet
    _settle(b, "A", "A", "n4")
    b.every_family()
    b.singles()
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")
    b.grid("moved", "G1"), b.grid("mover", "G2")
    for f in GRID_FAMILIES:
        b.query(f)
    b.upload(other)                                       # replacing: words, tables and grids gone, the map kept
    b.every_family()                                      # (the light queries are refused; the masked ones see every object)
    _settle(b, "B", "B")
    b.query("march_media")                                # (its rows are aimed at MOVED: before a grid takes MOVED out of it)
    b.grid("moved", "G2"), b.grid("mover", "G1")          # behind the replacing upload: they ride the new centres
    for f in TABLE_FAMILIES:
        b.query(f)
    b.query("march_media")
    b.media("B")                                          # dropped again: the steps below aim the homogeneous march at MOVED
    b.query("sample_lights"), b.query("light_pdf"), b.query("emit_lights")
    b.new_range(BLOCK_FAMILIES + MASKED)
    b.every_family()                                      # every family behind bounds rebuilt for other ranges
    b.variants()
    b.new_media()
    b.new_grids()
    b.new_textures()
    b.new_patches()
    b.new_map()
    b.media("A", bad="twice"), b.media("B", bad="negative"), b.phase("Q", wrong_count=True)   # refused: nothing changes
    for f in MEDIA_FAMILIES:
        b.query(f)
    b.twins()
    b.queued()
    b.upload(other)                                       # a cache hit: everything kept, the grids queued() left too
    b.every_family()
    b.new_words()
    b.every_family()                                      # every family behind words rebuilt
    b.upload(scene, bad=True)                             # the first scene with an unknown kind in it: refused, nothing changes
    b.every_family()
    b.environment("n16")
    b.query("environment"), b.query("sample_environment")
    b.new_range(BLOCK_FAMILIES + MASKED)
    b.every_family()
    b.upload(scene)                                       # back to the first scene: the accumulations go on where they stood
    b.groups(None)
    b.lights("A")                                         # set_lights after the upload: the table copies the new records
    b.media("B")                                          # set_media after the upload: the table is packed from the new records
    b.textures("A"), b.patches("A")                       # ... the binding is in the new list's numbering, the materials name its objects
    b.query("albedo")                                     # (the first reader of the by-object records behind the upload: the ground is unbound)
    b.query("march_media")                                # (before a grid takes MOVED out of it)
    b.grid("moved", "G1"), b.grid("mover", "G2")          # ... and the grids ride the new centres
    b.every_family()
    b.phase(None)
    b.query("sample_phase")
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")
    b.environment(None)
    b.query("sample_environment")                         # refused again
    b.lights(None)
    b.query("light_pdf")                                  # refused again
    b.media(None)                                         # the empty table drops the grids too
    b.query("march_media")                                # refused again
    b.query("march_media_grid")                           # refused again: no media table
    b.phase(None)                                         # refused: the Python layer's count of the table is 0 too
    b.textures(None), b.patches(None)
    b.query("albedo"), b.query("hit_patches")             # refused again
    b.query("occluded")


def _sizes(b):
    """The full scene list, growing and shrinking; every upload event twice before every family."""
    b.environment("n16")
    order = ("g9", "noground", "dense2", "odd_objects", "tiny", "dense", "g9")   # (odd_objects is dense and six more: not neighbours)
    for k, scene in enumerate(order):
        b.upload(scene)
        if k == 0:
            b.accumulate("progressive")
            b.accumulate("pixel_progressive")
        if k in (1, 4):                                   # straight after a replacing upload
            b.every_family()
        if k in (1, 2, 6):                                # a binding of the previous list's count, a material of its last object
            b.textures("A", count_of=order[k - 1]), b.patches("A", bad="material", of=order[k - 1])
            b.query("albedo"), b.query("hit_patches")    # (refused where the setter was: the upload cleared the tables)
        _settle(b, GROUPS[k % 2], tuple(LIGHTS)[k % 2])
        b.query("sample_lights"), b.query("light_pdf"), b.query("emit_lights")
        for f in MEDIA_FAMILIES:
            b.query(f)
        b.grid("moved", "G1"), b.grid("mover", "G2")      # behind the replacing upload
        for f in TABLE_FAMILIES:
            b.query(f)
        b.query("march_media")
        if k not in (2, 5):                               # (dense2 and dense keep them through the cache-hit upload below)
            b.media(tuple(LIGHTS)[k % 2])
        if k == 0:
            b.new_map()
        if k in (2, 5):
            b.upload(scene)
            b.every_family()
        if k == 3:
            b.environment("n4")
        if k in (3, 6):
            b.upload(order[k - 1], bad=True)
            b.every_family()
        b.new_range(BLOCK_FAMILIES + MASKED if k in (2, 5) else ("hit", "nearest", "crossings_m") if k % 2 else ("occluded", "bounce", "nearest_m", "hit_m"))
        if k in (2, 5):                                   # (dense2 and dense: scenes with a culling layout)
            b.every_family()
            b.new_words()
            b.every_family()
        if k == 4:
            b.variants()
            b.new_media()
            b.new_grids()
            b.new_textures()
            b.new_patches()
            b.twins()
        if k == 5:
            b.new_map()
            b.queued()
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")


def _seeded(b, n_steps):
    """Drawn steps.  A cache-hit upload is only drawn while words and a table are set (otherwise the steps behind it could not tell
    it from a replacing one), and an accumulation's second pass only on the scene of its first."""
    rng = b.rng
    names = ("g9", "g9_e", "dense", "dense_e", "noground", "tiny")
    b.photons("L")
    b.upload("g9")
    _settle(b, "A", "A", "n4")
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")
    while len(b.steps) < n_steps:
        s, r = b.model.state, rng.random()
        if r < 0.06:
            scene = names[int(rng.integers(len(names)))]
            if scene == s.scene and (s.groups is None or s.lights is None or s.media is None):
                _settle(b, GROUPS[int(rng.integers(2))], tuple(LIGHTS)[int(rng.integers(2))])
            b.upload(scene)
        elif r < 0.09:
            bad = names[int(rng.integers(len(names)))]
            if bad != s.scene:
                b.upload(bad, bad=True)
                b.query(("hit", "nearest", "scatter", "occluded_m", "bsdf")[int(rng.integers(5))])   # (a step that could tell)
        elif r < 0.14:
            b.groups((None, "A", "B")[int(rng.integers(3))])
        elif r < 0.19:
            b.lights((None, "A", "B")[int(rng.integers(3))])
        elif r < 0.23:
            b.environment((None, "n4", "n16")[int(rng.integers(3))])
        elif r < 0.30:
            f = (BLOCK_FAMILIES + MASKED)[int(rng.integers(len(BLOCK_FAMILIES + MASKED)))]
            b.new_range((f,))
        elif r < 0.36:
            b.render(int(rng.integers(2)), (0, 3)[int(rng.integers(2))])
        elif r < 0.40:
            b.media((None, "A", "B")[int(rng.integers(3))])
        elif r < 0.44:
            b.phase((None, "P", "Q")[int(rng.integers(3))])   # (refused where there is no table)
        elif r < 0.47:
            b.photons(("L", "S", "E")[int(rng.integers(3))])
        elif r < 0.51:                                    # (refused where there is no table; a grid on either role, or none)
            b.grid(("moved", "mover")[int(rng.integers(2))], (None, "G1", "G2", "G3")[int(rng.integers(4))])
        elif r < 0.54:
            b.textures((None, "A", "B")[int(rng.integers(3))])
        elif r < 0.57:
            b.patches((None, "A", "B")[int(rng.integers(3))])
        else:
            b.query(QUERY_FAMILIES[int(rng.integers(len(QUERY_FAMILIES)))])
    b.upload("g9")
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")


SCRIPTS = ("same_size", "same_size_g9", "sizes", "seeded_1", "seeded_2")
_scripts = {}


def script(name):
    """The steps of a named script (a list of dicts; the same list on every call).  `same_size` has a second context of its own,
    `same_size_g9`: the same steps on the nine-object scene and its edited copy."""
    if name not in _scripts:
        b = _Builder(SCRIPTS.index(name))
        if name.startswith("same_size"):
            _same_size(b, "g9" if name.endswith("g9") else "dense")
        elif name == "sizes":
            _sizes(b)
        else:
            _seeded(b, 150)
        _scripts[name] = b.steps
    return _scripts[name]
