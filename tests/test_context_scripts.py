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
- march_media there, when the previous list is too short to hold the table's objects: there is no stale table to restate."""
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
        m = S.Model()
        m.replay(steps, oracle)
        for which, passes in m.passes.items():
            assert len(passes) == 2 and passes[1][0] - passes[0][0] > 10, (name, which, passes)
            seen[("accumulation", "ten_foreign_steps")].append((name, passes[1][0]))
    return seen


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
    for name in S.SCRIPTS:
        steps, expects = _replay(oracle, name)
        for i, e in enumerate(expects):
            if e.refuse is None:
                continue
            assert e.refuse[0] == -1 and e.refuse[1] in ("unknown", "light table", "environment map", "no scene", "media table", "n_media",
                                                         "no photon map", "without directions") + tuple(S.BAD_MEDIA.values())
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
    import phase_restatement as PR
    n = collections.Counter()
    for name in S.SCRIPTS:
        for e in _replay(oracle, name)[1]:
            f = e.step.get("family")
            if e.step["op"] != "query" or e.refuse is not None or f not in ("march_media", "gather_photons", "sample_phase"):
                continue
            x = S.inputs(oracle, e.step, e.state)
            if f == "march_media":
                w = S.answer(oracle, e.step, x, e.state)
                n["march"] += len(w["status"])
                n["collided"] += int((w["status"] == 1).sum())
                n["several"] += sum(bin(int(a)).count("1") > 1 for a in w["active"])
            elif f == "gather_photons":
                w = S.answer(oracle, e.step, x, e.state)
                n["gather"] += len(w["count"])
                n["accepted"] += int((w["count"] > 0).sum())
            else:
                _, objects, sigma, albedo, gs = S._media_of(e.state)
                details = {}
                w = PR.sample(oracle, sigma, albedo, gs, x["rays"], x["t"], x["active"], x["states"], details=details)
                n["sample"] += len(w["pdf"])
                n["forward"] += sum(1 for d in details.values() if "chosen" in d and gs[d["chosen"]] != 0)
    return {"collided": n["collided"] / n["march"], "several": n["several"] / n["march"], "accepted": n["accepted"] / n["gather"],
            "forward": n["forward"] / n["sample"]}


# half of what the restatements measure on the scripts as committed (the measured shares in brackets)
COVERAGE_FLOORS = {"collided": 0.285,      # march rows that collide (0.570)
                   "several": 0.099,       # march rows that collide in more than one medium at once (0.199)
                   "accepted": 0.307,      # gather rows that accept a photon (0.615)
                   "forward": 0.238}       # sampled rows whose chosen medium has |g| > 0 (0.477)


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
