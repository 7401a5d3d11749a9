"""Scripts over ONE long-lived context, and a model of the context's documented state (tests/test_context_scripts.py on the CPU,
tests/test_gpu_context_scripts.py on the MI355X).

A script is a list of steps -- setters (upload, set_groups, set_lights, set_environment), queries of every family, renders and the
passes of two open accumulations -- as a host that keeps one context alive for a whole animation issues them.  script(name) returns
the steps; Model replays them and says, per step, EITHER the state the answer depends on (records, group words or none, light table
or none, environment map or none) OR that the step must be refused (code, a word of the message).  The model restates
include/tor_render.h, tor_lights.h, tor_env.h and the Python docstrings (what an upload resets and what it keeps); inputs() draws a
step's operands and answer() hands them to the family's restatement under a given state.  Nothing here judges an answer.

The inputs are shaped so that a stale cache shows: the edited copy of a scene changes the ground sphere's radius and material and
the centre of object 3, so `probe` rows (segments that end between the two grounds, points a little above the ground, hits and BSDF
items on the ground, lamps that include object 3) answer differently under the old records; `movers` rows are aimed at movers at
times at the far end of the new time range.  numpy only (the restatements of bounce, scatter, radiance and the samplers draw
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
import nearest_inputs as NI
import nearest_restatement as N
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


# ---- families ---------------------------------------------------------------------------------------------------------------------------
RAY_FAMILIES = ("hit", "occluded", "crossings", "bounce", "radiance")
BLOCK_FAMILIES = RAY_FAMILIES + ("nearest",)            # they take a mode and a time range: `bnd` and what hangs on it
MASKED = tuple(f + "_m" for f in ("hit", "occluded", "crossings", "nearest", "bounce"))
LIGHT_FAMILIES = ("sample_lights", "light_pdf", "emit_lights")
ENV_FAMILIES = ("environment", "sample_environment")
SCENE_FREE = ENV_FAMILIES + ("connect_camera", "deposit")   # they read no scene: no upload can change their answer
QUERY_FAMILIES = BLOCK_FAMILIES + ("scatter", "bsdf") + MASKED + LIGHT_FAMILIES + ENV_FAMILIES + ("connect_camera", "deposit")
FAMILIES = QUERY_FAMILIES + ("render",)
ACCUMULATIONS = ("progressive", "pixel_progressive")
SLOW = ("bounce", "bounce_m", "scatter", "radiance")    # their restatements loop in Python: 64 rays
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


def transition_table():
    """The committed table: the cross product of every query and render family with the five events -- a replacing, a cache-hit
    and a refused upload, the time range changed since the last block query (`bnd` rebuilt), the group words changed since the last
    masked query (`grp` rebuilt) -- and the four pairs.  The two accumulations have two passes per script and stand in the table as
    the last pair."""
    t = [(f, e) for f in FAMILIES for e in EVENTS]
    t += [(f, "lights_after_upload") for f in LIGHT_FAMILIES] + [(f, "map_kept") for f in ENV_FAMILIES]
    t += [("host_twin", "smaller_after_device"), ("accumulation", "ten_foreign_steps")]
    return t


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class State:
    """What an answer can depend on: names and keys, resolved by records(), words(), light_table(), env_map()."""

    def __init__(self, scene=None, groups=None, lights=None, env=None):
        self.scene, self.groups, self.lights, self.env = scene, groups, lights, env

    def but(self, **kw):
        s = copy.copy(self)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def key(self):
        return (self.scene, self.groups, self.lights, self.env)


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
    table" / "environment map").  Renders and unmasked queries read no words; the time range of a block query is a speed hint."""

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
            self.state = State(step["scene"], None, None, s.env)
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
    theirs can depend on either, so nothing is asked of their inputs, and the GPU test holds their answers all the same."""
    f, s, out = e.step["family"], e.state, []
    for event, old in e.events.items():
        if event in UPLOAD_EVENTS and f in SCENE_FREE:
            out.append((event, None, "reads no scene"))
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
    """Appends steps.  Mode, K and max_distance are drawn independently from the builder's generator, and the
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


def _settle(b, groups="A", lights="A", env=None):
    b.groups(groups)
    b.lights(lights)
    if env is not None:
        b.environment(env)


def _same_size(b, scene):
    """Uploads that keep the object count: a scene and its edited copy, there and back."""
    other = partner(scene)
    b.upload(scene)
    b.query("sample_lights")                              # refused: no table yet
    b.query("environment")                                # refused: no map yet
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
    b.every_family()
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")
    b.environment(None)
    b.query("sample_environment")                         # refused again
    b.lights(None)
    b.query("light_pdf")                                  # refused again
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
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")


def _seeded(b, n_steps):
    """Drawn steps.  A cache-hit upload is only drawn while words and a table are set (otherwise the steps behind it could not tell
    it from a replacing one), and an accumulation's second pass only on the scene of its first."""
    rng = b.rng
    names = ("g9", "g9_e", "dense", "dense_e", "noground", "tiny")
    b.upload("g9")
    _settle(b, "A", "A", "n4")
    b.accumulate("progressive")
    b.accumulate("pixel_progressive")
    while len(b.steps) < n_steps:
        s, r = b.model.state, rng.random()
        if r < 0.06:
            scene = names[int(rng.integers(len(names)))]
            if scene == s.scene and (s.groups is None or s.lights is None):
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
