"""The order inside a segment the reach pass runs on (tor_scene.cpp: a top-down even split of the ground positions, cut at the
sorted list's own word boundaries) against the Morton curve it replaced (TOR_REACH_ORDER=morton), on the host: tighter word boxes
and fewer words reached by single rays on random_scene; the reach pass's implication on the new order; a flagged segment that
begins off a word boundary; ties and non-finite centres; the cost of the build.

The bounds: a numpy model of the split on random_scene's 485 records gave 0.70 x the Morton order's mean half-perimeter (the 0.8
leaves room for the library's outward rounding and the float32 table's error E), a largest box of 0.079 of the field (Morton:
0.307; the bound 2 / 15 is two words' even share) and 0.66 x the reached (ray, word) pairs."""
import contextlib
import os
import time

import numpy as np

from test_reach import _sane_rays, _violations

FIELD = 22.0 * 22.0   # random_scene's field


@contextlib.contextmanager
def reach_order(value):
    """TOR_REACH_ORDER for the layouts built inside (None: the default)."""
    saved = os.environ.get("TOR_REACH_ORDER")
    try:
        if value is None:
            os.environ.pop("TOR_REACH_ORDER", None)
        else:
            os.environ["TOR_REACH_ORDER"] = value
        yield
    finally:
        if saved is None:
            os.environ.pop("TOR_REACH_ORDER", None)
        else:
            os.environ["TOR_REACH_ORDER"] = saved


def two_segments(n_rest=584, n_movers=320, seed=23):
    """Resting spheres at a common height on a 30 x 30 field and movers along y at another common height over the same field (+
    the ground): two segments the reach pass runs on, the second of which begins at slot 584 = 18 words + 8."""
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n_rest):
        x, z = rng.uniform(-15, 15, 2)
        recs.append([0, x, 0.2, z, x, 0.2, z, 0, 1, 0.2, 0, .5, .5, .5, 0, 0])
    for _ in range(n_movers):
        x, z = rng.uniform(-15, 15, 2)
        recs.append([1, x, 0.3, z, x, 0.3 + rng.uniform(0.05, 0.3), z, 0.0, 1.0, 0.2, 0, .5, .5, .5, 0, 0])
    recs.append([0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0])
    return np.asarray(recs, dtype=np.float64)


def _boxed_words(tor, recs, rays=None):
    """(words that carry a box, their boxes, slot per object, word per object, reach[n_rays, boxed words], segments)"""
    o, d, t = rays if rays is not None else (np.zeros((1, 3)), np.ones((1, 3)), np.zeros(1))
    world = tor.Scene.from_records(recs).list()
    reach, word, slot, boxes = tor.debug_reach_scene(world, o, d, t)
    words = np.unique(word[word >= 0])
    first = np.array([np.flatnonzero(word == w)[0] for w in words], dtype=np.int64)
    return words, boxes[words], slot, word, reach[:, first], tor.debug_layout_segments(world)


def _half_perimeter(boxes):
    return (boxes[:, 1] - boxes[:, 0]) + (boxes[:, 3] - boxes[:, 2])


def _words_inside_segments(recs, words, slot, word, segs):
    """Every boxed word lies wholly inside one segment and holds exactly its real slots; returns the segment of each word."""
    assert len(np.unique(slot)) == len(recs) and slot.min() >= 0
    seg_of_word = []
    for w in words:
        members = np.flatnonzero(word == w)
        owners = [s for s, (_, n_obj, n_slots, first) in enumerate(segs) if first <= 32 * w and 32 * (w + 1) <= first + n_slots]
        assert len(owners) == 1, (w, owners)
        _, n_obj, _, first = segs[owners[0]]
        assert np.all(slot[members] // 32 == w)
        assert len(members) == min(32, first + n_obj - 32 * w), (w, len(members))
        assert np.all((slot[members] >= first) & (slot[members] < first + n_obj))
        seg_of_word.append(owners[0])
    return np.asarray(seg_of_word)


def test_random_scene_boxes(tor):
    recs = tor.random_scene(0xFACADE).to_records()
    words, boxes, slot, word, _, segs = _boxed_words(tor, recs)
    with reach_order("morton"):
        m_words, m_boxes, m_slot, _, _, m_segs = _boxed_words(tor, recs)
    assert segs == m_segs == [(12, 481, 488, 0), (10, 4, 8, 488)]
    assert len(words) == len(m_words) == 15
    _words_inside_segments(recs, words, slot, word, segs)
    assert sorted(slot.tolist()) == sorted(m_slot.tolist())                   # the same slots, handed out differently
    assert not np.array_equal(slot, m_slot)
    hp, m_hp = float(_half_perimeter(boxes).mean()), float(_half_perimeter(m_boxes).mean())
    area = (boxes[:, 1] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 2]) / FIELD
    m_area = (m_boxes[:, 1] - m_boxes[:, 0]) * (m_boxes[:, 3] - m_boxes[:, 2]) / FIELD
    print(f"random_scene: mean half-perimeter {hp:.2f} (Morton {m_hp:.2f}: x {hp / m_hp:.3f}); area share of the field "
          f"{area.min():.3f} .. {area.max():.3f}, mean {area.mean():.3f} (Morton {m_area.min():.3f} .. {m_area.max():.3f}, mean {m_area.mean():.3f})")
    assert hp <= 0.8 * m_hp
    assert area.max() <= 2.0 / 15.0


def test_single_rays_reach_fewer_words_and_the_implication_holds(tor):
    rng = np.random.default_rng(81)
    recs = tor.random_scene(0xFACADE).to_records()
    rays = _sane_rays(rng, recs, (0.0, 0.0, 0.0), 400)
    _, _, _, _, reach, _ = _boxed_words(tor, recs, rays)
    with reach_order("morton"):
        _, _, _, _, m_reach, _ = _boxed_words(tor, recs, rays)
    assert reach.shape == m_reach.shape == (1200, 15)
    share, m_share = float(np.mean(reach != 0)), float(np.mean(m_reach != 0))
    print(f"random_scene: {share:.3f} of the (ray, whole word) pairs are reached, {m_share:.3f} in Morton order: x {share / m_share:.3f}")
    assert np.count_nonzero(reach) <= 0.8 * np.count_nonzero(m_reach)
    # not reached => stage two's code is not 2 and the reference misses, on the new order
    for name, scene_recs in (("random_scene", recs), ("two segments", two_segments())):
        o, d, t = _sane_rays(rng, scene_recs, (0.0, 0.0, 0.0), 120)
        bad, unreached, boxed, where = _violations(tor, scene_recs, o, d, t)
        assert bad == 0, (name, bad, where)
        assert boxed > 0 and unreached > 0.5 * boxed, (name, unreached, boxed)


def test_a_flagged_segment_off_a_word_boundary(tor):
    recs = two_segments()
    words, boxes, slot, word, _, segs = _boxed_words(tor, recs)
    with reach_order("morton"):
        m_words, m_boxes, m_slot, m_word, _, m_segs = _boxed_words(tor, recs)
    assert segs == m_segs == [(11, 584, 584, 0), (12, 320, 320, 584), (10, 1, 8, 904)]
    assert segs[1][3] % 32 != 0
    seg_of_word = _words_inside_segments(recs, words, slot, word, segs)
    m_seg_of_word = _words_inside_segments(recs, m_words, m_slot, m_word, m_segs)
    # 18 whole words of the first segment; the second's 8 head slots share word 18 with it, then 9 whole words and 24 tail slots
    assert np.array_equal(words, m_words) and words.tolist() == list(range(18)) + list(range(19, 28))
    for s in (0, 1):
        hp = float(_half_perimeter(boxes[seg_of_word == s]).mean())
        m_hp = float(_half_perimeter(m_boxes[m_seg_of_word == s]).mean())
        print(f"two segments, segment {s}: mean half-perimeter {hp:.2f} (Morton {m_hp:.2f}: x {hp / m_hp:.3f})")
        assert hp < 0.8 * m_hp, s
    # the segments' objects stay in their segments
    assert np.all(slot[:584] < 584) and np.all((slot[584:904] >= 584) & (slot[584:904] < 904))


def test_ties_and_bad_centres(tor):
    """64 spheres at one centre, 8 with a non-finite x or z (equal keys four by four: a non-finite coordinate is cell 0, the other
    coordinate is shared), 40 on a line x = const: the same order on every upload, a permutation, and equal keys in the order of
    appearance."""
    rng = np.random.default_rng(82)
    n = 400
    xz = rng.uniform(-12, 12, (n, 2))
    same = np.sort(rng.choice(np.arange(100, n), 64, replace=False))
    xz[same] = [3.25, -4.5]
    rest = np.setdiff1d(np.arange(n), same)
    line = rng.choice(rest, 40, replace=False)
    xz[line, 0] = 7.125
    rest = np.setdiff1d(rest, line)
    bad = np.sort(rng.choice(rest, 8, replace=False))
    bad_x, bad_z = bad[0::2], bad[1::2]
    xz[bad_x, 0] = [np.nan, np.inf, -np.inf, np.nan]
    xz[bad_x, 1] = 1.5
    xz[bad_z, 1] = [np.inf, np.nan, np.nan, -np.inf]
    xz[bad_z, 0] = -2.25
    recs = np.zeros((n, 16))
    recs[:, 1], recs[:, 2], recs[:, 3] = xz[:, 0], 0.2, xz[:, 1]
    recs[:, 4:7] = recs[:, 1:4]
    recs[:, 8], recs[:, 9] = 1.0, 0.2
    recs[:, 11:14] = 0.5
    one = (np.zeros((1, 3)), np.ones((1, 3)), np.zeros(1))
    slots = []
    for _ in range(2):
        world = tor.Scene.from_records(recs).list()
        assert tor.debug_layout_segments(world) == [(11, 400, 400, 0)]
        slots.append(tor.debug_reach_scene(world, *one)[2])
    slot = slots[0]
    assert np.array_equal(slot, slots[1])
    assert sorted(slot.tolist()) == list(range(n))
    assert not np.array_equal(slot, np.arange(n))                              # (the split ran: not the order of appearance)
    for group in (same, bad_x, bad_z):
        assert np.all(np.diff(slot[group]) > 0), (group, slot[group])
    with reach_order("morton"):
        m_slot = tor.debug_reach_scene(tor.Scene.from_records(recs).list(), *one)[2]
    assert sorted(m_slot.tolist()) == list(range(n))
    assert np.all(np.diff(m_slot[same]) > 0)


def test_upload_cost(tor):
    """A segment of 20 000 objects is ordered within the bound tests/test_accel_layout.py sets for its build (2 s)."""
    rng = np.random.default_rng(83)
    n = 20000
    diag = np.arange(n) * 0.05
    for name, x, z in (("random field", rng.uniform(-300, 300, n), rng.uniform(-300, 300, n)),
                       ("on a diagonal, sorted", diag, diag),
                       ("a few distinct places", rng.integers(0, 12, n) * 5.0, rng.integers(0, 12, n) * 5.0)):
        recs = np.zeros((n, 16))
        recs[:, 1], recs[:, 2], recs[:, 3] = x, 0.2, z
        recs[:, 4:7] = recs[:, 1:4]
        recs[:, 8], recs[:, 9] = 1.0, 0.2
        recs[:, 11:14] = 0.5
        world = tor.Scene.from_records(recs).list()
        t = time.time()
        segs = tor.debug_layout_segments(world)
        dt = time.time() - t
        print(f"{name}: {n} objects, layout built in {dt:.3f} s")
        assert segs == [(11, n, n, 0)]
        assert dt < 2.0, (name, dt)
        reach, word, slot, boxes = tor.debug_reach_scene(world, np.zeros((1, 3)), np.ones((1, 3)), np.zeros(1))
        assert sorted(slot.tolist()) == list(range(n))
        assert np.count_nonzero(word >= 0) == n                                  # 625 whole words, every one boxed
