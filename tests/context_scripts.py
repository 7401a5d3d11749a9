"""Scripts over ONE long-lived context, and a model of the context's documented state (tests/test_context_scripts.py on the CPU,
tests/test_gpu_context_scripts.py on the MI355X).

A script is a list of steps -- setters (upload, set_groups, set_lights, set_environment, set_media, set_media_phase,
build_photons), queries of every family, renders and the passes of two open accumulations -- as a host that keeps one context alive for a whole animation issues them.  script(name) returns
the steps; Model replays them and says, per step, EITHER the state the answer depends on (records, group words or none, light table
or none, environment map or none, media table with its g or none, photon map or none) OR that the step must be refused (code, a
word of the message).  The model restates include/tor_render.h, tor_lights.h, tor_env.h, tor_media.h, tor_phase.h, tor_photons.h
and the Python docstrings (what an upload resets and what it keeps); inputs() draws a
step's operands and answer() hands them to the family's restatement under a given state.  Nothing here judges an answer.

The inputs are shaped so that a stale cache shows: the edited copy of a scene changes the ground sphere's radius and material and
the centre of object 3, so `probe` rows (segments that end between the two grounds, points a little above the ground, hits and BSDF
items on the ground, lamps that include object 3) answer differently under the old records; `movers` rows are aimed at movers at
times at the far end of the new time range; media rows are aimed at the boundary objects of the media tables, object 3 first
among them; gather points come from the point sets of the current photon map and of the one before it.  numpy only (the restatements of bounce, scatter, radiance and the samplers draw
through the oracle's exported generator, which the caller hands in)."""
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
import hit_restatement as H
import light_inputs as LI
import light_restatement as LR
import masked_restatement as M
import media_inputs as MI
import media_restatement as MR
import nearest_inputs as NI
import nearest_restatement as N
import phase_restatement as PR
import photon_inputs as PI
import photon_restatement as PH
import query_regimes as Q
import radiance_restatement as RR
import render_regimes as R

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


# ---- families ---------------------------------------------------------------------------------------------------------------------------
RAY_FAMILIES = ("hit", "occluded", "crossings", "bounce", "radiance")
BLOCK_FAMILIES = RAY_FAMILIES + ("nearest",)            # they take a mode and a time range: `bnd` and what hangs on it
MASKED = tuple(f + "_m" for f in ("hit", "occluded", "crossings", "nearest", "bounce"))
LIGHT_FAMILIES = ("sample_lights", "light_pdf", "emit_lights")
ENV_FAMILIES = ("environment", "sample_environment")
MEDIA_FAMILIES = ("march_media", "scatter_media", "sample_phase", "phase")   # they read the media table
PHASE_FAMILIES = ("sample_phase", "phase")              # ... and word 15 of it
NEW_FAMILIES = ("gather_photons",) + MEDIA_FAMILIES + ("uniform",)
SCENE_FREE = ENV_FAMILIES + ("connect_camera", "deposit", "gather_photons", "uniform")   # they read no scene: no upload can change their answer
QUERY_FAMILIES = BLOCK_FAMILIES + ("scatter", "bsdf") + MASKED + LIGHT_FAMILIES + ENV_FAMILIES + ("connect_camera", "deposit") + NEW_FAMILIES
FAMILIES = QUERY_FAMILIES + ("render",)
ACCUMULATIONS = ("progressive", "pixel_progressive")
SLOW = ("bounce", "bounce_m", "scatter", "radiance", "sample_phase")    # their restatements loop in Python: 64 rays
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
                 + [("gather_photons", ("build_photons",))])


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
    return t


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class State:
    """What an answer can depend on: names and keys, resolved by records(), words(), light_table(), env_map()."""

    def __init__(self, scene=None, groups=None, lights=None, env=None, media=None, phase=None, photons=None):
        self.scene, self.groups, self.lights, self.env = scene, groups, lights, env
        self.media, self.phase, self.photons = media, phase, photons   # a key of MEDIA, a key of G, (a key of PHOTON_MAPS, listed?)
        self.packed = None                                # alternatives() alone: the scene whose records a stale table was packed from

    def but(self, **kw):
        s = copy.copy(self)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def key(self):
        return (self.scene, self.groups, self.lights, self.env, self.media, self.phase, self.photons)


REFUSED = "refused"


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
    nothing that normals could miss).  tor_rng_uniform_device needs nothing."""

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
            self.state = State(step["scene"], None, None, s.env, None, None, s.photons)
            return Expect(step, self.state, None, {})
        if op == "set_media":
            if s.scene is None:
                return Expect(step, s, (-1, "no scene"), {})
            if step.get("bad"):
                return Expect(step, s, (-1, BAD_MEDIA[step["bad"]]), {})
            self._note("media_table", s.media, MEDIA_FAMILIES)
            self._note("phase_g", s.phase, PHASE_FAMILIES)   # (every table starts isotropic)
            self.state = s.but(media=step["table"], phase=None)
            return Expect(step, self.state, None, {})
        if op == "set_media_phase":
            if s.scene is None:
                return Expect(step, s, (-1, "no scene"), {})
            if s.media is None:
                return Expect(step, s, (-1, "media table"), {})
            if step.get("wrong_count"):
                return Expect(step, s, (-1, "n_media"), {})
            self._note("phase_g", s.phase, PHASE_FAMILIES)
            self.state = s.but(phase=step["g"])
            return Expect(step, self.state, None, {})
        if op == "build_photons":
            self._note("photon_map", s.photons, ("gather_photons",))
            self.state = s.but(photons=(step["map"], bool(step["listed"])))
            return Expect(step, self.state, None, {})
        if op == "set_groups":
            self.state = s.but(groups=step["words"])
            return Expect(step, self.state, None, {})
        if op == "set_lights":
            self._note("table", s.lights, LIGHT_FAMILIES)
            self.state = s.but(lights=step["table"])
            return Expect(step, self.state, None, {})
        if op == "set_environment":
            self._note("map", s.env, ENV_FAMILIES)
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
    `uniform` reads nothing and is exempt from everything; `gather_photons` reads no scene and is exempt from the upload events."""
    f, s, out = e.step["family"], e.state, []
    for event, old in e.events.items():
        if event in UPLOAD_EVENTS and f in SCENE_FREE:
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
        if f == "march_media":
            w = MR.march(mrecs, objects, sigma, x["rays"], x["tau"])
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

    def twins(self):
        """Every new family through its host twin, behind a larger device call of another family."""
        for f in NEW_FAMILIES:
            self.query("hit", host=False, n=257)
            self.query(f, host=True, **({} if f in SLOW else {"n": 63}))

    def queued(self):
        """A render, a query on device tensors, then a setter of the table that query reads: no host step in between."""
        st = self.model.state
        for f, setter in (("march_media", lambda: self.media("B" if st.media == "A" else "A")), ("sample_phase", lambda: self.phase("Q")),
                          ("gather_photons", lambda: self.photons("S")), ("sample_lights", lambda: self.lights("B" if st.lights == "A" else "A")),
                          ("environment", lambda: self.environment("n16" if st.env == "n4" else "n4"))):
            self.render(0, 3)
            self.query(f, host=False)
            st = self.model.state
            setter()
            self.query(f)


def _settle(b, groups="A", lights="A", env=None):
    """Words, a light table, the media table of the same name with a g vector (P for A, Q for B), and an environment map where asked."""
    b.groups(groups)
    b.lights(lights)
    b.media(lights)
    b.phase("P" if lights == "A" else "Q")
    if env is not None:
        b.environment(env)


def _same_size(b, scene):
    """Uploads that keep the object count: a scene and its edited copy, there and back."""
    other = partner(scene)
    b.query("uniform")                                    # needs no scene
    b.query("gather_photons")                             # refused: no map yet
    b.query("march_media"), b.query("phase")              # refused: no scene yet
    b.media("A"), b.phase("P")                            # refused: no scene yet
    b.photons("L")                                        # needs no scene
    b.query("gather_photons")
    b.upload(scene)
    b.query("sample_lights")                              # refused: no table yet
    b.query("environment")                                # refused: no map yet
    b.query("scatter_media"), b.phase("P")                # refused: no table yet
    _settle(b, "A", "A", "n4")
    b.every_family()
    b.singles()
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")
    b.upload(other)                                       # replacing: words and table gone, the map kept
    b.every_family()                                      # (the light queries are refused; the masked ones see every object)
    _settle(b, "B", "B")
    b.query("sample_lights"), b.query("light_pdf"), b.query("emit_lights")
    b.new_range(BLOCK_FAMILIES + MASKED)
    b.every_family()                                      # every family behind bounds rebuilt for other ranges
    b.variants()
    b.new_media()
    b.new_map()
    b.media("A", bad="twice"), b.media("B", bad="negative"), b.phase("Q", wrong_count=True)   # refused: nothing changes
    for f in MEDIA_FAMILIES:
        b.query(f)
    b.twins()
    b.queued()
    b.upload(other)                                       # a cache hit: everything kept
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
    b.every_family()
    b.phase(None)
    b.query("sample_phase")
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")
    b.environment(None)
    b.query("sample_environment")                         # refused again
    b.lights(None)
    b.query("light_pdf")                                  # refused again
    b.media(None)
    b.query("march_media")                                # refused again
    b.phase(None)                                         # refused: the Python layer's count of the table is 0 too
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
        _settle(b, GROUPS[k % 2], tuple(LIGHTS)[k % 2])
        b.query("sample_lights"), b.query("light_pdf"), b.query("emit_lights")
        for f in MEDIA_FAMILIES:
            b.query(f)
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
            _seeded(b, 120)
        _scripts[name] = b.steps
    return _scripts[name]
