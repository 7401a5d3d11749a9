"""The scripts of tests/context_scripts.py on the CPU: they cover the transitions a long-lived context goes through, every step
behind such a transition would answer differently from a stale cache, every refusal is followed by a step that could tell, and the
model restates the rules the per-feature lifecycle tests pin.  From the scripts and the restatements alone: no GPU, no library.

Stale-sensitivity is a condition on the INPUTS: the restatement's answer under the previous state (context_scripts.alternatives)
differs from the right one in at least a quarter of the rows.  Exempt, with the reason alternatives() gives:
- environment, sample_environment, connect_camera and deposit after any upload: they read no scene;
- after a cache-hit upload every family but the masked ones (with words set) and the light ones (with a table set): a cache hit
  taken for a replacing upload would reset the words and clear the table, nothing else;
- the light families after a refused upload without a table: refused either way;
- `time` and `words` at a family that reads neither the block bounds nor the words (the event is that they were rebuilt beside
  its own buffers since it last ran): no restatement can depend on them, so there is nothing to ask of the inputs; the coverage
  test still counts these entries of the table, and the GPU test holds the answers;
- a change of the time range on a scene without a culling layout (nine objects): no query reads the bounds, and the coverage test
  does not count it either;
- a change of the time range whose new range lies inside the old one: the old boxes contain the new ones, so stale bounds answer
  right.  org / reach2 / a_min and pt_reach2 only move lanes between two exact paths and change no answer, so nothing is asked of
  them here; for the other changes the rows must be timed outside the old range and answered by a mover that has left the place it
  has over the old range (context_scripts.time_rows);
- `uniform` at every event: it reads nothing;
- gather_photons after any upload: it reads no scene (its own events are photon_map and map_kept);
- scatter_media, sample_phase and phase after set_media behind a replacing upload: they read sigma, albedo and g of the table, no
  boundary, so a table packed from the previous records answers them alike -- march_media is held there;
- march_media there, when the previous list is too short to hold the table's objects: there is no stale table to restate;
- hit_patches and the unmerged occluded_patches after any upload while their table is set: they read no scene record (a table
  that an upload should have cleared and did not, or cleared and should not have, is refused on one side and counts);
- the merged occluded_patches behind another patch table: in a scene with its original ground the ground occludes every probe
  row whatever the table says; the unmerged steps hold the table, and the builder merges only where no table event is pending;
- albedo behind set_textures behind a replacing upload under texture key B, or in a scene without a ground: the ground is bound
  (or absent) and no row reads a record that the edit changes; key A, with the ground unbound, holds the untextured path;
- march_media_grid and media_density behind set_media_grid behind a replacing upload, when the list before holds the medium's
  boundary as it is (the mover's: the edit moves MOVED alone) or is too short to hold it;
- media_density reads no sigma: a stale sigma of the table cannot show in it, and no event asks it to;
- a grid event at a step on another medium than the one whose grid changed: the step's own medium holds what it held."""
import collections

import numpy as np
import pytest

import context_scripts as S

QUARTER = 0.25
_replays, _answers = {}, {}


def _replay(oracle, name):
    if name not in _replays:
        steps = S.script(name)
        _replays[name] = (steps, S.Model().replay(steps, oracle))
    return _replays[name]


def _asks(e):
    return e.step["op"] in ("query", "render", "pass")


def _new_range(step, x):
    t = x["points"][:, 3] if S.base(step["family"]) == "nearest" else x["rays"][:, 6]
    return S.Model().effective_range(step, t)


def _sensitivity(oracle, e):
    """[(event, share of the rows that differ, or None with the reason it is exempt)] of one step."""
    out, x, want = [], None, None
    for event, alt, why in S.alternatives(e):
        if alt is None:
            out.append((event, None, why))
        elif alt is S.REFUSED or e.refuse is not None:
            out.append((event, 1.0, "answered on one side, refused on the other"))
        else:
            if x is None:
                x = S.inputs(oracle, e.step, e.state)
                want = S.answer(oracle, e.step, x, e.state)
            out.append((event, float(S.differing_rows(want, S.answer(oracle, e.step, x, alt)).mean()), ""))
    if "time" in e.events and e.refuse is None and S.takes_mode(e.step["family"]):
        x = S.inputs(oracle, e.step, e.state) if x is None else x
        old, new = e.events["time"], _new_range(e.step, x)
        if not S.has_blocks(e.state.scene):
            out.append(("time", None, "the scene has no culling layout: no query of its reads the bounds"))
        elif old[0] <= new[0] and new[1] <= old[1]:
            out.append(("time", None, "the new range lies inside the old one"))
        else:
            want = S.answer(oracle, e.step, x, e.state) if want is None else want
            out.append(("time", float(S.time_rows(e.step, x, want, e.state, old).mean()), ""))
    return out


def _occurrences(oracle):
    """{table entry: [(script, step number)]} over all scripts."""
    seen = collections.defaultdict(list)
    for name in S.SCRIPTS:
        steps, expects = _replay(oracle, name)
        for i, e in enumerate(expects):
            q, r = (expects[i - 1], expects[i - 2]) if i > 1 else (None, None)
            if q is not None and e.refuse is None and r.step["op"] == "render" and q.step["op"] == "query" and not q.step["host"] \
                    and q.refuse is None and not S._needs_times(q.step) and e.step["op"] in S.SETTER_OF.get(q.step["family"], ()):
                seen[("setter", "behind_queued_work")].append((name, i))   # (a render and a query on tensors: nothing waits)
                if e.step["op"] in S.TABLE_SETTERS:
                    seen[(e.step["op"], "behind_queued_work")].append((name, i))
            if not _asks(e):
                continue
            f = e.step["family"]
            for event in e.events:
                if event in S.UPLOAD_EVENTS or event == "words":
                    seen[(f, event)].append((name, i))
            if "time" in e.events and S.has_blocks(e.state.scene):     # (without a culling layout no bounds were rebuilt)
                if not S.takes_mode(f):
                    seen[(f, "time")].append((name, i))
                else:
                    old, new = e.events["time"], _new_range(e.step, S.inputs(oracle, e.step, e.state))
                    if not (old[0] <= new[0] and new[1] <= old[1]):
                        seen[(f, "time")].append((name, i))
            if f in S.LIGHT_FAMILIES and e.refuse is None and "replace" in e.events:
                seen[(f, "lights_after_upload")].append((name, i))
            if f in S.ENV_FAMILIES and e.refuse is None and "replace" in e.events and "map" not in e.events:
                seen[(f, "map_kept")].append((name, i))
            if f in S.MEDIA_FAMILIES and e.refuse is None and "replace" in e.events:
                seen[(f, "media_after_upload")].append((name, i))
            if f == "gather_photons" and e.refuse is None and "replace" in e.events and "photon_map" not in e.events:
                seen[(f, "map_kept")].append((name, i))
            _grid_and_table_entries(seen, name, i, e)
            for event, alt, _ in S.alternatives(e) if e.refuse is None else ():   # another table, g or map: one that would answer otherwise
                if event in ("media_table", "phase_g", "photon_map") and alt is not None and alt is not S.REFUSED:
                    seen[(f, event)].append((name, i))
            p = expects[i - 1] if i else None
            if p is not None and p.step["op"] == "query" and e.step["op"] == "query" and p.refuse is None and e.refuse is None \
                    and p.step["family"] != f and f != "deposit" and (not p.step["host"] or p.step["family"] == "deposit") \
                    and e.step["host"] and e.step["n"] < p.step["n"]:
                seen[("host_twin", "smaller_after_device")].append((name, i))
                if f in S.NEW_FAMILIES:
                    seen[("new_host_twin", "smaller_after_device")].append((name, i))
                if f in S.TABLE_FAMILIES:
                    seen[("table_host_twin", "smaller_after_device")].append((name, i))
        m = S.Model()
        m.replay(steps, oracle)
        for which, passes in m.passes.items():
            assert len(passes) == 2 and passes[1][0] - passes[0][0] > 10, (name, which, passes)
            seen[("accumulation", "ten_foreign_steps")].append((name, passes[1][0]))
    return seen


def _grid_and_table_entries(seen, name, i, e):
    """The entries of the grids, the texture table and the patch table at one step: each is counted where the step's answer (or
    its refusal) differs from the stale state's that context_scripts.alternatives names for it."""
    f, ev = e.step["family"], e.events
    if f not in S.TABLE_FAMILIES + ("march_media",):
        return
    alts = {event: alt for event, alt, _ in S.alternatives(e)}
    tells = lambda event: alts.get(event) is not None
    if f in S.GRID_FAMILIES + ("march_media",):
        if "grid" in ev and tells("grid"):
            removed = f != "march_media" and e.refuse is not None
            removed |= f == "march_media" and any(m not in e.state.grids for m in ev["grid"])
            seen[(f, "grid_removed" if removed else "grid")].append((name, i))
        if "grids_dropped" in ev and tells("grids_dropped") and (f == "march_media" or e.refuse is not None):
            seen[(f, "grids_dropped")].append((name, i))
    if f == "march_media":
        return
    kept = ("cache_hit" in ev and tells("cache_hit")) or ("kept" in ev and tells("kept") and
                                                          (f not in S.GRID_FAMILIES or ev["kept"] & {"set_media_phase", "set_lights"}))
    which = "grids" if f in S.GRID_FAMILIES else "textures" if f == "albedo" else "patches"
    if e.refuse is None and kept:
        seen[(f, which + "_kept")].append((name, i))
    if e.refuse is None and "replace" in ev:
        seen[(f, "grid_after_upload" if which == "grids" else which + "_after_upload")].append((name, i))
    for event in ("texture_table", "patch_table"):
        if e.refuse is None and event in ev and alts.get(event) is not None and alts[event] is not S.REFUSED:
            seen[(f, event)].append((name, i))


def test_every_transition_occurs_three_times_and_once_in_same_size(oracle):
    seen = _occurrences(oracle)
    missing = {}
    for entry in S.transition_table():
        where = seen.get(entry, [])
        if len(where) < 3 or not any(name.startswith("same_size") for name, _ in where):
            missing[entry] = where
    assert not missing, missing


def test_every_named_combination_occurs_and_in_same_size(oracle):
    """crossings K = 4 (records) and 16, nearest K = 2 and 16 with and without max_distance, each on device tensors and through the
    host twin, plain and masked; every mode per block family on either kind of operand; a batch of one for every family that takes one."""
    for scripts in (S.SCRIPTS, ("same_size",)):
        seen = collections.defaultdict(set)
        for name in scripts:
            for e in _replay(oracle, name)[1]:
                st = e.step
                if st["op"] != "query" or e.refuse is not None:
                    continue
                f = st["family"]
                seen[f, "n"].add(st["n"])
                if S.base(f) == "crossings":
                    seen[f].add((st["k"], bool(st["records"]), st["host"]))
                if S.base(f) == "nearest":
                    seen[f].add((st["k"], bool(st["dmax"]), st["host"]))
                if S.takes_mode(f):
                    seen[f, "mode"].add((st["mode"], st["host"]))
        for f in ("crossings", "crossings_m"):
            assert seen[f] == {(k, k == 4, h) for k in (4, 16) for h in (False, True)}, (scripts, f, seen[f])
        for f in ("nearest", "nearest_m"):
            assert seen[f] == {(k, d, h) for k in (2, 16) for d in (False, True) for h in (False, True)}, (scripts, f, seen[f])
        for f in S.BLOCK_FAMILIES + S.MASKED:
            if len(scripts) > 1:                          # (same_size alone: every mode, both kinds of operand)
                assert seen[f, "mode"] == {(m, h) for m in S.MODES for h in (False, True)}, (scripts, f, seen[f, "mode"])
            assert {m for m, _ in seen[f, "mode"]} == set(S.MODES) and {h for _, h in seen[f, "mode"]} == {False, True}, (scripts, f)
        for f in S.QUERY_FAMILIES:
            if f in S.SLOW:
                assert seen[f, "n"] == {64}
            elif len(scripts) > 1:
                assert seen[f, "n"] == set(S.BATCHES), (scripts, f, seen[f, "n"])
            else:                                         # (same_size alone: the batch of one and three other sizes)
                assert 1 in seen[f, "n"] and len(seen[f, "n"]) >= 4, (scripts, f, seen[f, "n"])


def test_the_accumulations_stay_open_across_foreign_steps_of_every_kind(oracle):
    for name in S.SCRIPTS:
        steps, _ = _replay(oracle, name)
        m = S.Model()
        m.replay(steps, oracle)
        for which in S.ACCUMULATIONS:
            (a, scene_a), (b, scene_b) = m.passes[which]
            between = steps[a:b - 1]
            assert len(between) >= 10, (name, which)
            assert {"upload", "query"} <= {s["op"] for s in between}, (name, which)
            # both passes see one scene (other scenes come and go in between): an accumulation keeps its camera, and a pixel's
            # stream is one chain
            assert scene_a == scene_b, (name, scene_a, scene_b)
        if name.startswith("same_size") or name == "sizes":
            kinds = {s["op"] for s in steps[m.passes["progressive"][0][0]:m.passes["progressive"][1][0]]}
            assert {"upload", "set_groups", "set_lights", "set_environment", "query", "render"} <= kinds, (name, kinds)


@pytest.mark.parametrize("name", S.SCRIPTS)
def test_a_stale_cache_would_show_in_a_quarter_of_the_rows(oracle, name):
    _, expects = _replay(oracle, name)
    weak, n_held = [], 0
    for i, e in enumerate(expects):
        if not _asks(e) or not e.events:
            continue
        for event, share, why in _sensitivity(oracle, e):
            if share is None:
                continue
            n_held += 1
            if share < QUARTER:
                weak.append((i, e.step["family"], event, round(share, 3), e.step.get("n"), e.state.key()))
    print(f"{name}: {n_held} (step, event) pairs held to a quarter of the rows")
    assert n_held > 20 and not weak, weak


def test_every_refusal_is_followed_by_a_step_that_could_tell(oracle):
    """A refused upload is followed, before the next upload, by steps whose answer under the refused list's records differs (the
    sensitivity test holds them to a quarter of the rows); a refused query changes nothing by construction, and the step behind it
    answers from the model's unchanged state."""
    n_refused_uploads = n_refused_setters = 0
    n_refused_tables = collections.Counter()
    for name in S.SCRIPTS:
        steps, expects = _replay(oracle, name)
        for i, e in enumerate(expects):
            if e.refuse is None:
                continue
            words = ("unknown", "light table", "environment map", "no scene", "media table", "n_media", "no photon map", "without directions",
                     "outside the media table", "has no density grid", "no texture table", "n_objects must be", "is outside", "no patch table",
                     "material outside") + tuple(S.BAD_MEDIA.values()) + tuple(S.BAD_GRIDS.values())
            assert e.refuse[0] == -1 and e.refuse[1] in words
            assert i + 1 < len(steps), (name, i)
            if e.step["op"] in ("set_media", "set_media_phase") and e.state.scene is not None:
                # a refused table or g changes nothing: a media query that would answer otherwise follows before the next setter of it
                tellers = []
                for later in expects[i + 1:]:
                    if later.refuse is None and later.step["op"] in ("upload", e.step["op"], "set_media"):
                        break
                    if _asks(later) and later.step["family"] in (S.PHASE_FAMILIES if e.step["op"] == "set_media_phase" else S.MEDIA_FAMILIES):
                        tellers.append(later.step["family"])
                n_refused_setters += bool(tellers)
            if e.step["op"] in S.TABLE_SETTERS and e.state.scene is not None:
                # a refused grid, texture table or patch table changes nothing: a query of its families follows before the next
                # accepted setter of it (or an upload, or -- the grids -- a set_media)
                reads = {"set_media_grid": S.GRID_FAMILIES, "set_textures": ("albedo",), "set_patches": S.PATCH_FAMILIES}[e.step["op"]]
                tellers = []
                for later in expects[i + 1:]:
                    if later.refuse is None and later.step["op"] in ("upload", e.step["op"]) + (("set_media",) if e.step["op"] == "set_media_grid" else ()):
                        break
                    if _asks(later) and later.step["family"] in reads:
                        tellers.append(later.step["family"])
                assert tellers or name.startswith("seeded"), (name, i, e.step)   # (a drawn refusal may stand before a drawn setter)
                n_refused_tables[e.refuse[1]] += bool(tellers)
            if e.step["op"] != "upload":
                continue
            n_refused_uploads += 1
            tellers = []
            for later in expects[i + 1:]:
                if later.step["op"] == "upload":
                    break
                if _asks(later) and any(ev == "refused" and alt is not None for ev, alt, _ in S.alternatives(later)):
                    tellers.append(later.step["family"])
            assert tellers, (name, i)
    assert n_refused_uploads >= 6
    assert n_refused_setters >= 6                         # (the table listed twice, the negative sigma and the short g of both same_size scripts)
    # every refusal of the three new setters that needs a scene, in both same_size scripts and in sizes at the least
    for word in ("media table", "outside the media table", "TOR_GRID_MAX_DIM", "finite and >= 0", "n_objects must be", "is outside", "material outside"):
        assert n_refused_tables[word] >= 3, (word, n_refused_tables)


def test_the_model_restates_the_lifecycle_rules():
    """By hand, the rules the per-feature lifecycle tests pin on the GPU."""
    up = lambda scene, bad=False: dict(op="upload", scene=scene, bad=bad)
    q = lambda family, **kw: dict(op="query", family=family, seed=1, n=64, host=False, **kw)
    m = S.Model()
    m.apply(up("dense"))
    assert (m.n_uploads, m.n_cache_hits) == (1, 0)
    # test_gpu_light_query.py::test_the_light_table_lifecycle: no table yet -> code -1, "light table"
    assert m.apply(q("sample_lights")).refuse == (-1, "light table")
    m.apply(dict(op="set_lights", table="A"))
    assert m.apply(q("light_pdf")).refuse is None
    m.apply(up("dense"))                                  # ... a byte-identical upload keeps the table
    assert m.apply(q("sample_lights")).state.lights == "A" and (m.n_uploads, m.n_cache_hits) == (2, 1)
    m.apply(up("dense_e"))                                # ... a replacing upload clears it
    assert m.apply(q("sample_lights")).refuse == (-1, "light table") and m.apply(q("emit_lights")).refuse is not None
    m.apply(dict(op="set_lights", table="B"))
    m.apply(dict(op="set_lights", table=None))            # ... and so does an empty table
    assert m.apply(q("light_pdf")).refuse is not None
    # test_gpu_masked_query.py::test_reset_replacing_upload_and_identical_upload
    m.apply(dict(op="set_groups", words="A"))
    assert m.apply(q("hit_m", mode="brute")).state.groups == "A"
    assert m.apply(q("hit", mode="brute")).state.groups == "A"          # (the unmasked entry never reads them: answer() ignores them)
    m.apply(up("dense_e"))
    assert m.apply(q("hit_m", mode="brute")).state.groups == "A"
    m.apply(dict(op="set_groups", words=None))
    assert m.apply(q("occluded_m", mode="brute")).state.groups is None
    m.apply(dict(op="set_groups", words="B"))
    m.apply(up("dense"))
    e = m.apply(q("hit_m", mode="brute"))
    assert e.state.groups is None and e.state.scene == "dense" and e.events["replace"] == "dense_e"
    assert "words" not in e.events                        # (None at the last masked query, "B" set and reset by the upload: None again)
    # test_gpu_env_query.py::test_the_maps_lifecycle: no map yet; the map needs no scene and survives uploads; None clears it
    m2 = S.Model()
    assert m2.apply(q("environment")).refuse == (-1, "environment map")
    m2.apply(dict(op="set_environment", map="n4"))
    assert m2.apply(q("sample_environment")).refuse is None
    m2.apply(up("g9")), m2.apply(up("tiny"))
    assert m2.apply(q("sample_environment")).state.env == "n4"
    m2.apply(dict(op="set_environment", map="n16"))
    e = m2.apply(q("environment"))
    assert e.state.env == "n16" and e.events["map"] == "n4"
    m2.apply(dict(op="set_environment", map=None))
    assert m2.apply(q("environment")).refuse is not None
    # test_gpu_round2.py::test_scene_cache_and_host_canvas_region: every upload counts, identical bytes count as hits; and
    # tor_scene_upload's refusal of an unknown kind (it changes nothing, although n_uploads moves)
    before = m2.state.key()
    assert m2.apply(up("dense", bad=True)).refuse == (-1, "unknown")
    assert m2.state.key() == before and (m2.n_uploads, m2.n_cache_hits) == (3, 0)
    m2.apply(up("tiny"))
    assert (m2.n_uploads, m2.n_cache_hits) == (4, 1)
    # test_gpu_media_query.py / test_gpu_phase_query.py / test_gpu_photon_query.py: the lifecycles of the table, its g and the map
    m4 = S.Model()
    sm = lambda table, bad=None: dict(op="set_media", table=table, bad=bad)
    sp = lambda g, wrong=False: dict(op="set_media_phase", g=g, wrong_count=wrong)
    bp = lambda key: dict(op="build_photons", map=key, host=True, listed=False)
    gq = lambda **kw: q("gather_photons", pools=("L",), kernel="constant", **kw)
    assert m4.apply(q("uniform", draws=3)).refuse is None                          # needs nothing
    assert m4.apply(gq()).refuse == (-1, "no photon map")
    assert m4.apply(bp("S")).refuse is None and m4.apply(gq()).refuse is None       # a map needs no scene
    assert m4.apply(gq(normals=True)).refuse == (-1, "without directions")
    for f in S.MEDIA_FAMILIES:
        assert m4.apply(q(f)).refuse == (-1, "no scene")
    assert m4.apply(sm("A")).refuse == (-1, "no scene") and m4.apply(sp("P")).refuse == (-1, "no scene")
    m4.apply(up("dense"))
    for f in S.MEDIA_FAMILIES:
        assert m4.apply(q(f)).refuse == (-1, "media table")
    assert m4.apply(sp("P")).refuse == (-1, "media table") and m4.apply(sp(None)).refuse == (-1, "media table")
    m4.apply(sm("A"))
    assert (m4.state.media, m4.state.phase) == ("A", None)                           # every table starts isotropic
    assert m4.apply(sp("P", True)).refuse == (-1, "n_media") and m4.state.phase is None
    m4.apply(sp("P"))
    assert m4.apply(q("sample_phase")).state.phase == "P"
    before = m4.state.key()
    assert m4.apply(sm("B", "twice")).refuse == (-1, "listed twice") and m4.apply(sm("B", "negative")).refuse == (-1, "sigma")
    assert m4.state.key() == before                                                 # a refused table changes nothing
    m4.apply(up("dense")), m4.apply(up("dense_e", bad=True))                        # a cache hit and a refused upload keep all three
    assert m4.state.key() == before
    m4.apply(sm("B"))                                                               # set_media resets g
    e = m4.apply(q("phase"))
    assert (e.state.media, e.state.phase) == ("B", None) and e.events["phase_g"] == "P" and e.events["media_table"] == "A"
    m4.apply(sp("Q")), m4.apply(bp("L"))
    m4.apply(up("dense_e"))                                                         # a replacing upload clears the table, g with it
    assert (m4.state.media, m4.state.phase, m4.state.photons) == (None, None, ("L", False))   # ... and keeps the map
    assert m4.apply(q("march_media")).refuse == (-1, "media table")
    e = m4.apply(gq(normals=True))
    assert e.refuse is None and e.events["photon_map"] == ("S", False) and e.events["replace"] == "dense"
    m4.apply(sm("A")), m4.apply(sm(None))                                           # the empty table clears it
    assert m4.apply(q("scatter_media")).refuse == (-1, "media table") and m4.apply(sp(None)).refuse == (-1, "media table")
    m4.apply(bp("E"))
    assert m4.apply(gq(normals=True)).refuse is None                                # a build of no photons holds nothing normals could miss
    # test_gpu_grid_query.py::test_the_grids_follow_the_media_tables_lifecycle
    m5 = S.Model()
    sg = lambda who, grid: dict(op="set_media_grid", who=who, grid=grid)
    gm = lambda who: q("march_media_grid", who=who)
    gd = lambda who: q("media_density", who=who)
    assert m5.apply(sg("moved", "G1")).refuse == (-1, "no scene") and m5.apply(gm("moved")).refuse == (-1, "no scene")
    m5.apply(up("dense"))
    assert m5.apply(sg("moved", "G1")).refuse == (-1, "media table") and m5.apply(gd("moved")).refuse == (-1, "media table")
    m5.apply(sm("A"))
    assert m5.apply(gm("moved")).refuse == (-1, "has no density grid") and m5.apply(gd(7)).refuse == (-1, "outside the media table")
    assert m5.apply(sg(7, "G1")).refuse == (-1, "outside the media table") and m5.apply(sg(-1, "G1")).refuse == (-1, "outside the media table")
    assert m5.apply(sg(7, "dims")).refuse == (-1, "outside the media table")           # (the header's order: the medium before the dimensions)
    assert m5.apply(sg("moved", "dims")).refuse == (-1, "TOR_GRID_MAX_DIM")
    assert m5.apply(sg("moved", "nan")).refuse == m5.apply(sg("moved", "negative")).refuse == (-1, "finite and >= 0") and not m5.state.grids
    m5.apply(sg("moved", "G1")), m5.apply(sg("mover", "G2"))
    assert m5.state.grids == {0: "G1", 1: "G2"}                                      # table A lists MOVED first, the mover second
    e = m5.apply(q("march_media"))
    assert e.state.grids == {0: "G1", 1: "G2"} and e.events["grid"] == {0: None, 1: None}   # the homogeneous march depends on them
    m5.apply(sg("moved", "G2"))                                                      # a second grid replaces the first
    assert m5.apply(gm("moved")).state.grids[0] == "G2" and m5.apply(gm("moved")).events == {}
    before = m5.state.key()
    for refused in (sg("moved", "nan"), sg(7, "G3"), sm("B", "twice"), up("dense_e", bad=True)):
        assert m5.apply(refused).refuse is not None and m5.state.key() == before      # every refusal changes nothing
    for kept in (sp("P"), dict(op="set_lights", table="A"), dict(op="set_environment", map="n4"), dict(op="set_groups", words="B"), bp("L"),
                 dict(op="set_textures", table="A"), dict(op="set_patches", table="B"), up("dense")):
        assert m5.apply(kept).refuse is None and m5.state.grids == {0: "G2", 1: "G2"}, kept   # ... phase, lights, ..., a cache hit keep them
    e = m5.apply(gd("mover"))
    assert e.refuse is None and e.events["kept"] >= {"set_media_phase", "set_lights", "set_textures", "set_patches"} and e.events["cache_hit"]
    m5.apply(sg("moved", None))                                                      # (0, 0, 0) removes that medium's grid only
    assert m5.state.grids == {1: "G2"} and m5.apply(gm("moved")).refuse == (-1, "has no density grid") and m5.apply(gm("mover")).refuse is None
    m5.apply(sg("moved", "G3"))
    m5.apply(sm("B"))                                                                # set_media drops every grid ...
    assert m5.state.grids == {} and m5.apply(gm("moved")).refuse == (-1, "has no density grid")
    e = m5.apply(q("march_media"))
    assert e.events["grids_dropped"] == ("A", {0: "G3", 1: "G2"}) and e.state.grids == {}
    m5.apply(sg("moved", "G1"))
    assert m5.state.grids == {1: "G1"}                                               # ... and table B lists MOVED second: another index
    m5.apply(sm(None))                                                               # the empty table drops them too
    assert m5.state.grids == {} and m5.apply(gm("moved")).refuse == (-1, "media table")
    m5.apply(sm("A")), m5.apply(sg("mover", "G2")), m5.apply(up("dense_e"))          # ... and so does a replacing upload
    assert m5.state.grids == {} and m5.state.media is None and m5.apply(sg("mover", "G2")).refuse == (-1, "media table")
    e = m5.apply(gd("mover"))
    assert e.refuse == (-1, "media table") and e.events["before"].grids == {1: "G2"} and e.events["replace"] == "dense"
    # test_gpu_texture_query.py::test_the_table_follows_the_light_tables_lifecycle and ::test_refusals_that_need_a_context
    m6 = S.Model()
    tx = lambda table, **kw: dict(op="set_textures", table=table, bad=kw.get("bad"), count_of=kw.get("count_of"))
    assert m6.apply(tx("A")).refuse == (-1, "no scene") and m6.apply(q("albedo")).refuse == (-1, "no scene")
    m6.apply(up("g9"))
    assert m6.apply(q("albedo")).refuse == (-1, "no texture table")
    assert m6.apply(tx("A", bad="long")).refuse == (-1, "n_objects must be") and m6.apply(tx("A", count_of="dense")).refuse == (-1, "n_objects must be")
    assert m6.apply(tx("A", bad="outside")).refuse == (-1, "is outside") and m6.state.textures is None
    assert m6.apply(tx("A", count_of="g9_e")).refuse is None and m6.state.textures == "A"   # (the same count)
    for kept in (sm("A"), sg("moved", "G1"), sp("P"), dict(op="set_lights", table="B"), dict(op="set_groups", words="A"), bp("S"),
                 dict(op="set_patches", table="A"), up("g9"), up("dense", bad=True), tx("B", bad="outside")):
        m6.apply(kept)
        assert m6.state.textures == "A", kept
    m6.apply(tx("B"))
    e = m6.apply(q("albedo"))
    assert e.state.textures == "B" and e.events["texture_table"] == "A" and m6.state.grids == {0: "G1"} and m6.state.patches == "A"
    m6.apply(tx(None))                                                               # an empty table clears it
    assert m6.apply(q("albedo")).refuse == (-1, "no texture table")
    m6.apply(tx("B")), m6.apply(up("g9_e"))                                          # ... and so does a replacing upload
    assert m6.state.textures is None and m6.state.patches is None and m6.apply(q("albedo")).refuse == (-1, "no texture table")
    # test_gpu_patch_query.py::test_the_table_follows_the_texture_tables_lifecycle and ::test_refusals_that_need_a_context
    m7 = S.Model()
    pa = lambda table, **kw: dict(op="set_patches", table=table, bad=kw.get("bad"), of=kw.get("of"))
    assert m7.apply(pa("A")).refuse == (-1, "no scene")
    for f in S.PATCH_FAMILIES:
        assert m7.apply(q(f)).refuse == (-1, "no scene")
    m7.apply(up("g9"))
    for f in S.PATCH_FAMILIES:
        assert m7.apply(q(f)).refuse == (-1, "no patch table")
    assert m7.apply(pa("A", bad="material")).refuse == (-1, "material outside")         # object 9 of nine
    assert m7.apply(pa("A", bad="material", of="dense")).refuse == (-1, "material outside")   # a table valid for dense: its object 723
    assert m7.apply(pa("A", bad="material", of="g9_e")).refuse is None and m7.state.patches == "A"   # (object 8 of nine is a material)
    for kept in (sm("B"), sg("mover", "G2"), sp("Q"), dict(op="set_lights", table="A"), dict(op="set_environment", map="n16"), bp("E"),
                 tx("B"), dict(op="set_groups", words="B"), up("g9"), up("tiny", bad=True), pa("B", bad="material")):
        m7.apply(kept)
        assert m7.state.patches == "A", kept
    m7.apply(pa("B"))
    e = m7.apply(q("hit_patches_merged"))
    assert e.state.patches == "B" and e.events["patch_table"] == "A" and m7.state.textures == "B" and m7.state.grids == {2: "G2"}
    m7.apply(pa(None))                                                               # an empty table clears it
    assert m7.apply(q("occluded_patches")).refuse == (-1, "no patch table")
    m7.apply(pa("A")), m7.apply(up("tiny"))                                          # ... and so does a replacing upload
    assert m7.state.patches is None and m7.apply(q("hit_patches")).refuse == (-1, "no patch table")
    # the time range is a key of the bounds: a block query under another range is an event, a brute-force one is none
    m3 = S.Model()
    m3.apply(up("dense"))
    assert "time" not in m3.apply(q("hit", mode="blocks", time_range=(0.0, 1.0))).events
    assert "time" not in m3.apply(q("occluded", mode="brute", time_range=(0.5, 0.5))).events
    assert m3.apply(q("nearest", mode="auto", time_range=(-3.0, 0.5))).events["time"] == (0.0, 1.0)
    assert m3.apply(q("hit", mode="auto", time_range=None), times=[0.25, np.nan, 0.75]).events["time"] == (-3.0, 0.5)
    assert m3.block_range == (0.25, 0.75)


def _coverage(oracle):
    """Shares of the rows of the answered steps, over all scripts, through the restatements alone."""
    import grid_restatement as GR
    import patch_restatement as PT
    import phase_restatement as PR
    import texture_restatement as TR
    n = collections.Counter()
    for name in S.SCRIPTS:
        for e in _replay(oracle, name)[1]:
            f = e.step.get("family")
            if e.step["op"] != "query" or e.refuse is not None or f not in ("march_media", "gather_photons", "sample_phase") + S.TABLE_FAMILIES:
                continue
            x = S.inputs(oracle, e.step, e.state)
            if f == "march_media":
                w = S.answer(oracle, e.step, x, e.state)
                n["march"] += len(w["status"])
                n["collided"] += int((w["status"] == 1).sum())
                n["several"] += sum(bin(int(a)).count("1") > 1 for a in w["active"])
                if e.state.grids:                         # rows that answer otherwise than the whole table would
                    n["march_grids"] += len(w["status"])
                    n["grid_changes"] += int(S.differing_rows(w, S.answer(oracle, e.step, x, e.state.but(grids={}))).sum())
            elif f == "march_media_grid":
                recs, objects, sigma, _, _ = S._media_of(e.state)
                steps = np.zeros(len(x["rays"]), dtype=np.int64)
                w = GR.march(recs, objects, sigma, S._grid(e.state, S.medium_of(e.state.media, e.step["who"])), x["rays"], x["tau"], steps=steps)
                n["grid_march"] += len(steps)
                n["grid_collided"] += int((w["status"] == 1).sum())
                n["grid_two_cells"] += int((steps >= 2).sum())
            elif f == "albedo":
                tex, binding = S.texture_table(e.state.textures, e.state.scene)
                obj, front = x["hits"].view(np.int32)[:, 14], x["hits"].view(np.int32)[:, 15]
                bound = np.where((obj >= 0) & (obj < len(binding)), binding[np.clip(obj, 0, len(binding) - 1)], -2)
                n["albedo"] += len(obj)
                n["untextured"] += int((bound == -1).sum())
                n["image"] += sum(1 for b in bound if b >= 0 and tex[b]["kind"] == TR.IMAGE)
                for i in np.flatnonzero(bound >= 0):      # the bilinear footprint: a corner column or row outside the square
                    t = tex[bound[i]]
                    st = TR.encode(tuple(x["hits"][i, 3:6] * (1.0 if front[i] else -1.0))) if t["kind"] == TR.IMAGE and t["option"] == TR.BILINEAR else None
                    if st is not None:
                        side = t["rgb"].shape[0]
                        lo = [np.floor((v + 1.0) * (0.5 * side) - 0.5) for v in st]
                        n["edge"] += any(v < 0 or v + 1 > side - 1 for v in lo)
            elif f in ("hit_patches", "hit_patches_merged"):
                w = S.answer(oracle, e.step, x, e.state)
                if f == "hit_patches":
                    n["patch_rows"] += len(w["patch"])
                    n["patch_hit"] += int((w["patch"] >= 0).sum())
                    if e.step["masks"] is not None:       # the mask takes the closest patch away (another one, or none, answers)
                        free = PT.hit(S.patch_table(e.state.patches, e.state.scene), x["rays"], x["t_range"])
                        n["masked_rows"] += len(w["patch"])
                        n["mask_removes"] += int(((free["patch"] >= 0) & (free["patch"] != w["patch"])).sum())
                else:
                    n["merged"] += len(w["patch"])
                    n["patch_wins"] += int((w["patch"] >= 0).sum())
                    n["sphere_wins"] += int(((w["patch"] < 0) & (w["object"] >= 0)).sum())
            elif f == "gather_photons":
                w = S.answer(oracle, e.step, x, e.state)
                n["gather"] += len(w["count"])
                n["accepted"] += int((w["count"] > 0).sum())
            elif f == "sample_phase":
                _, objects, sigma, albedo, gs = S._media_of(e.state)
                details = {}
                w = PR.sample(oracle, sigma, albedo, gs, x["rays"], x["t"], x["active"], x["states"], details=details)
                n["sample"] += len(w["pdf"])
                n["forward"] += sum(1 for d in details.values() if "chosen" in d and gs[d["chosen"]] != 0)
    return {"collided": n["collided"] / n["march"], "several": n["several"] / n["march"], "accepted": n["accepted"] / n["gather"],
            "forward": n["forward"] / n["sample"], "grid_collided": n["grid_collided"] / n["grid_march"],
            "grid_two_cells": n["grid_two_cells"] / n["grid_march"], "grid_changes": n["grid_changes"] / n["march_grids"],
            "image": n["image"] / n["albedo"], "untextured": n["untextured"] / n["albedo"], "edge": n["edge"] / n["albedo"],
            "patch_hit": n["patch_hit"] / n["patch_rows"], "patch_wins": n["patch_wins"] / n["merged"],
            "sphere_wins": n["sphere_wins"] / n["merged"], "mask_removes": n["mask_removes"] / n["masked_rows"]}


# half of what the restatements measure on the scripts as committed (the measured shares in brackets)
COVERAGE_FLOORS = {"collided": 0.285,      # march rows that collide (0.570)
                   "several": 0.099,       # march rows that collide in more than one medium at once (0.199)
                   "accepted": 0.307,      # gather rows that accept a photon (0.615)
                   "forward": 0.238,       # sampled rows whose chosen medium has |g| > 0 (0.477)
                   # (the four above stand as they were set; with the grid steps among the media steps they measure 0.431, 0.170,
                   # 0.560 and 0.381 on the scripts as grown: among other things a medium with a grid leaves the homogeneous march)
                   "grid_collided": 0.156,  # grid-march rows that collide (0.313)
                   "grid_two_cells": 0.458,  # grid-march rows that visit at least two cells before they stop (0.917)
                   "grid_changes": 0.339,  # march_media rows, under a state with grids, that a grid medium answers otherwise (0.678)
                   "image": 0.148,         # albedo rows that read an image (0.297)
                   "untextured": 0.148,    # albedo rows that take the untextured path (0.296)
                   "edge": 0.060,          # albedo rows whose bilinear footprint crosses the square's edge (0.121)
                   "patch_hit": 0.164,     # hit_patches rows that hit a patch (0.328)
                   "patch_wins": 0.130,    # merged rows won by the patch (0.261)
                   "sphere_wins": 0.229,   # merged rows won by the sphere (0.459)
                   "mask_removes": 0.073}  # masked hit_patches rows where the mask removes the otherwise closest patch (0.146)


def test_the_new_families_rows_do_what_they_are_for(oracle):
    got = _coverage(oracle)
    print({k: round(v, 3) for k, v in got.items()})
    short = {k: (got[k], floor) for k, floor in COVERAGE_FLOORS.items() if not got[k] >= floor}
    assert not short, short


def test_the_named_values_are_what_the_scripts_need():
    """Two tables over the same boundary objects, MOVED and a mover among them, in another order with other sigma and albedo; two g
    vectors with a sign change and a 0; a large map with directions, a smaller one without and with another radius whose powers
    are 2^52 below, and the empty one."""
    for name in S.SCENES:
        (oa, sa, aa), (ob, sb, ab) = S.media_table("A", name), S.media_table("B", name)
        recs = S.records(name)
        assert S.MOVED in oa and S.MOVED in ob and set(ob) < set(oa) and len(set(oa)) == len(oa) == 4
        assert [o for o in oa if o in ob] != list(ob) and not set(sa) & set(sb) and not {tuple(r) for r in aa} & {tuple(r) for r in ab}
        assert (np.abs(recs[oa, 9]) > 0).all() and S.placeable(recs)[oa].all()
        if ((recs[:, 0] == 1) & S.placeable(recs)).any():
            assert (recs[oa, 0] == 1).any() and (recs[ob, 0] == 1).any()
        assert S.media_table("A", name, "twice")[0][-1] == oa[0] and (S.media_table("B", name, "negative")[1] < 0).any()
    for n in (3, 4):
        p, q = S.g_vector("P", n), S.g_vector("Q", n)
        assert (np.sign(p) != np.sign(q)).all() and (p * q < 0).any() and (np.abs(p) <= 0.99).all() and (np.abs(q) <= 0.99).all()
        assert (S.g_vector(None, n) == 0).all()
    assert 0 in S.G["P"] and 0 in S.G["Q"]
    L, Sm, E = S.photon_map("L"), S.photon_map("S"), S.photon_map("E")
    assert L["has_dir"] and not Sm["has_dir"] and L["radius"] != Sm["radius"]
    assert len(L["stored"]["position"]) > 10 * len(Sm["stored"]["position"]) > 0 and len(E["stored"]["position"]) == 0
    assert L["stored"]["n_buckets"] > Sm["stored"]["n_buckets"] > E["stored"]["n_buckets"]      # smaller after larger: stale tails
    assert L["scale"] / Sm["scale"] == 2.0 ** -52 and S.power_scale(np.array([[0.5, 0.25, 0.0]])) == 2.0
    listed = S.photon_map("L", True)
    assert listed["index"].min() < 0 and listed["index"].max() >= len(L["position"]) and len(set(listed["index"])) < len(listed["index"])
    # the grids: every dimension distinct, G2 with fewer cells than G1, G3 with G1's cell count in another shape, an explicit
    # off-centre box and the sphere's cube, distinct densities with exact zeros; the refused ones are refused for one reason each
    import patch_restatement as PT
    import texture_restatement as TR
    dims = {k: v[0] for k, v in S.GRIDS.items()}
    assert dims["G1"] == (5, 4, 3) and dims["G2"] == (2, 3, 7) and all(len(set(d)) == 3 for d in dims.values())
    assert np.prod(dims["G2"]) < np.prod(dims["G1"]) == np.prod(dims["G3"]) and dims["G3"][1:] != dims["G1"][1:]
    box = np.array(S.GRIDS["G1"][1])
    assert S.GRIDS["G2"][1] is None and S.GRIDS["G3"][1] is None and (box[:3] < box[3:]).all() and (box[:3] != -box[3:]).all()
    assert (np.abs(box) < 1).all()                        # (inside the sphere's cube: the box clips, and so does the sphere)
    for key in S.GRIDS:
        d = S.grid_density(key).reshape(-1)
        assert d.shape == (np.prod(dims[key]),) and (d >= 0).all() and 2 <= (d == 0).sum() < d.size // 4
        assert len(set(d[d > 0])) == (d > 0).sum()
    assert S.grid_density("dims").shape[0] > 1024 and np.isnan(S.grid_density("nan")).sum() == 1 and (S.grid_density("negative") < 0).sum() == 1
    for table in S.MEDIA:                                 # a role names another medium index under the other table
        assert [S.MEDIA[table][0][S.medium_of(table, w)] for w in S.ROLES] == [0, 1]
    assert S.medium_of("A", "moved") != S.medium_of("B", "moved") and S.medium_of("A", "mover") == S.medium_of("B", "moved")
    assert S.medium_of("A", 7) == 7 and 7 >= max(len(v[0]) for v in S.MEDIA.values())
    for name in S.SCENES:
        recs, n, s = S.records(name), len(S.records(name)), S.scale(name)
        assert S.boundaries(name)[0] == S.MOVED
        if ((recs[:, 0] == 1) & S.placeable(recs)).any():
            assert recs[S.boundaries(name)[1], 0] == 1     # the "mover" role is a mover where the scene has one
        # the textures: A with all five kinds, the 4 x 4 nearest image at a non-zero atlas offset; B smaller, with a smaller atlas;
        # the ground unbound in A and bound in B, MOVED on an image in both; the refused bindings
        (ta, ba), (tb, bb) = S.texture_table("A", name), S.texture_table("B", name)
        pa, atlas_a = TR.pack(ta)
        pb, atlas_b = TR.pack(tb)
        assert [(t["kind"], t["option"]) for t in ta] == [(TR.CONSTANT, 0), (TR.CHECKER, TR.WORLD), (TR.CHECKER, TR.NORMAL), (TR.IMAGE, TR.BILINEAR),
                                                         (TR.IMAGE, TR.NEAREST)]
        assert (pa[3]["side"], pa[3]["offset"], pa[4]["side"], pa[4]["offset"]) == (8, 0, 4, 64)
        assert [(t["kind"], t["option"]) for t in tb] == [(TR.CONSTANT, 0), (TR.IMAGE, TR.BILINEAR)] and (pb[1]["side"], pb[1]["offset"]) == (2, 0)
        assert len(tb) < len(ta) and len(atlas_b) < len(atlas_a)
        assert len(ba) == len(bb) == n and ba[0] == -1 and bb[0] >= 0 and ta[ba[S.MOVED]]["kind"] == tb[bb[S.MOVED]]["kind"] == TR.IMAGE
        assert set(ba) == set(range(-1, 5)) and set(bb) == {-1, 0, 1}
        assert len(S.texture_table("A", name, "long")[1]) == n + 1 and S.texture_table("B", name, "outside")[1].max() == len(tb)
        # the patches: 65 and 9, quads and triangles, materials -1, 0 and MOVED, words that a one-bit mask excludes, no shared
        # patch; every patch lies between 0 and half a scale above the floor the probe rows end at, some of them below the
        # original's ground (0.125 scales above it) and some above
        ta, tb = S.patch_table("A", name), S.patch_table("B", name)
        assert (len(ta), len(tb)) == (65, 9) and S.PATCHES == {"A": 65, "B": 9}
        for t in (ta, tb):
            assert {p["kind"] for p in t} == {PT.QUAD, PT.TRIANGLE} and {p["material"] for p in t} == {-1, 0, S.MOVED}
            assert PT.refusal(t, n) is None
            words = np.array([p["groups"] for p in t], dtype=np.int64)
            assert (words == 0xFFFFFFFF).any() and ((words & S.PATCH_MASK) == 0).any() and ((words & S.PATCH_MASK) != 0).any()
            heights = []
            for p in t:
                for c in (p["q"], p["q"] + p["u"], p["q"] + p["v"]) + ((p["q"] + p["u"] + p["v"],) if p["kind"] == PT.QUAD else ()):
                    heights.append((c[1] - float(S.floor_height(name, c[0], c[2]))) / s)
            heights = np.array(heights)
            assert (heights > 0.02).all() and (heights < 0.5).all() and (heights < 0.1).sum() >= 3 and (heights > 0.15).sum() >= 3, (name, heights.min(), heights.max())
        assert not {(tuple(p["q"]), tuple(p["u"]), tuple(p["v"])) for p in ta} & {(tuple(p["q"]), tuple(p["u"]), tuple(p["v"])) for p in tb}
        assert PT.refusal(S.patch_table("A", name, "material"), n) == (1, "material")
    assert PT.refusal(S.patch_table("A", "g9", "material", of="dense"), 9) == (1, "material")      # valid for dense, not for the nine
    assert PT.refusal(S.patch_table("A", "dense", "material", of="dense"), 724) is None


def test_the_edited_copies_keep_the_count_and_change_one_radius_one_centre_one_material():
    for name in ("dense", "g9"):
        a, b = S.records(name), S.records(S.partner(name))
        assert a.shape == b.shape and S.ground(a) == 0
        rows = np.flatnonzero((a != b).any(axis=1))
        assert list(rows) == [0, S.MOVED]
        assert a[0, 9] != b[0, 9] and a[0, 10] != b[0, 10] and (a[0, 1:9] == b[0, 1:9]).all()
        assert (a[S.MOVED, 1:4] != b[S.MOVED, 1:4]).all() and (a[S.MOVED, 7:] == b[S.MOVED, 7:]).all()
    assert len(S.records("g9")) == 9 and len(S.records("noground")) == 90 and len(S.records("tiny")) == 200
    assert len(S.records("dense")) == 724 and len(S.records("dense2")) == 1300
