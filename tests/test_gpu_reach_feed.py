"""The reach pass's skipped words on the GPU (kernel/integrate_loop_plane.inc): NO store to the words nobody reaches -- the
summary's rebuild after stage two leaves them out by a mask (`reach_skip`) instead of finding zeros there.  At 27 x 48, 4 spp,
depth 50, sample streams, brute force, as tests/test_gpu_reach_order.py runs: in every case the canvas and the candidates are those
of the same build without stage one (TOR_PLANE=0), and the canvas is that of the build without the FMA screen (TOR_SCREEN=0).

Where it can go wrong, and the case that goes there:
  * the length of a pass -- flagged segments of 8, 9, 12, 13 and 16 whole words in one pass (two box trips exactly, two and a
    box, three, three and a box, the full pass of four): the mask is cut to the pass's words, moved up by the words stored in
    front of them and turned round against the summary.  (The layout puts the largest segment first and flags a segment from
    288 objects on, so the segment of EIGHT whole words sits in the second pass, behind 520 slots of another);
  * a pass that resumes inside a flagged segment (more than 512 slots): the pass starts at i != 0 and the mask of skipped words
    begins afresh;
  * two flagged segments, the second off a word boundary: the word they share is stored by the block phase and read back by
    stage two's `shared_word` while the mask holds skipped words of both;
  * segments of 1, 2, 3 and 5 whole words under TOR_PLANE=2, which runs the pass in front of every segment that has boxes;
  * stale words: a camera above a wide field looking straight down reaches a few words per query and skips the rest on every
    pass, and random_scene's bounces alternate between queries that reach many words and queries that reach few -- the skipped
    slots then hold the non-zero words of the query before, and only the mask keeps them out of the candidates.  (A build
    without the mask and without the zero stores, -DTOR_REACH_NOZERO=2, fails these: profiles/reach_feed_ab.txt.)
  * random_scene's canvas has the hash tests/test_gpu_reach.py records."""
import hashlib

import numpy as np
import pytest

from test_gpu_plane_feed import _scene
from test_gpu_reach import _RANDOM_SCENE_SHA256
from test_gpu_reach_order import _env
from test_reach_order import two_segments

H, W, SPP = 27, 48, 4


def _run(tor, scene, cam, **env):
    """(candidates, canvas, whole words walked, whole words met) of one strict brute-force frame on a context created under env."""
    import torch
    with _env(**{"TOR_PLANE": None, "TOR_SCREEN": None, **env}):
        ctx = tor.Context(0)
        ctx.upload(scene.list())
        ctx.set_stats(True)
        buf = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        ctx.render_device(cam, H, W, SPP, 2.2, 50, tor.make_options(seeding=tor.SEED_SAMPLE, accel=0), buf.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    st = ctx.last_stats()
    walked, met = ctx.last_reach()
    ctx.close()
    return st.candidates, buf.cpu().numpy(), walked, met


def _same_as_without(tor, name, scene, cam, plane=None):
    """The run under TOR_PLANE=plane against TOR_PLANE=0 (candidates, canvas) and TOR_SCREEN=0 (canvas); returns the run."""
    run = _run(tor, scene, cam, TOR_PLANE=plane)
    off = _run(tor, scene, cam, TOR_PLANE="0")
    bare = _run(tor, scene, cam, TOR_SCREEN="0")
    print(f"{name}: candidates {run[0]} (TOR_PLANE=0: {off[0]}); whole words walked {run[2]} of {run[3]}")
    assert float(np.abs(off[1]).sum()) > 0.0
    assert off[3] == 0 and bare[3] == 0            # no stage one: no whole word met
    assert run[0] == off[0], name
    assert np.array_equal(run[1], off[1]), name
    assert np.array_equal(run[1], bare[1]), name
    return run


# (name, objects per height, the layout, boxed words of the layout, whole words a query meets)
# (eight whole words: the second segment's 24 head slots finish word 16, then words 17 .. 24, then 8 tail slots)
_WORD_CASES = [
    ("8 whole words: two trips", [520, 288], [(11, 520, 520, 0), (11, 288, 288, 520), (10, 1, 8, 808)], 24, 24),
    ("9 whole words: two trips and a box", [300], [(11, 300, 304, 0), (10, 1, 8, 304)], 9, 9),
    ("12 whole words: three trips", [390], [(11, 390, 392, 0), (10, 1, 8, 392)], 12, 12),
    ("13 whole words: three trips and a box", [420], [(11, 420, 424, 0), (10, 1, 8, 424)], 13, 13),
    ("16 whole words: the full pass", [512], [(11, 512, 512, 0), (10, 1, 8, 512)], 16, 16),
]


@pytest.mark.parametrize("name,sizes,layout,n_boxed,n_met", _WORD_CASES, ids=[c[0] for c in _WORD_CASES])
def test_layouts_are_the_shapes_the_cases_mean(tor, name, sizes, layout, n_boxed, n_met):
    scene, _ = _scene(tor, sizes, True)
    assert tor.debug_layout_segments(scene.list()) == layout
    _, word, _, _ = tor.debug_reach_scene(scene.list(), np.zeros((1, 3)), np.ones((1, 3)), np.zeros(1))
    boxed = np.unique(word[word >= 0])
    assert len(boxed) == n_boxed
    if len(sizes) == 2:   # the second segment's whole words: 17 .. 24, all in the second pass
        assert boxed.tolist() == list(range(16)) + list(range(17, 25))


@pytest.mark.gpu
@pytest.mark.parametrize("name,sizes,layout,n_boxed,n_met", _WORD_CASES, ids=[c[0] for c in _WORD_CASES])
def test_box_group_counts(tor, name, sizes, layout, n_boxed, n_met):
    scene, _ = _scene(tor, sizes, True)
    assert tor.debug_layout_segments(scene.list()) == layout
    run = _same_as_without(tor, name, scene, tor.camera())
    # the pass runs by default on these segments, over n_met whole words per query, and skips some
    assert run[3] > 0 and run[3] % n_met == 0 and run[2] < run[3], (name, run[2:])


@pytest.mark.gpu
def test_a_pass_resumes_inside_a_flagged_segment(tor):
    scene, _ = _scene(tor, [600], True)
    assert tor.debug_layout_segments(scene.list()) == [(11, 600, 608, 0), (10, 1, 8, 608)]
    run = _same_as_without(tor, "600: 16 whole words, then 3 more from i = 512", scene, tor.camera())
    assert run[3] > 0 and run[3] % 19 == 0 and run[2] < run[3], run[2:]


@pytest.mark.gpu
def test_two_flagged_segments_share_a_word(tor):
    scene = tor.Scene.from_records(two_segments())
    assert tor.debug_layout_segments(scene.list()) == [(11, 584, 584, 0), (12, 320, 320, 584), (10, 1, 8, 904)]
    run = _same_as_without(tor, "two flagged segments", scene, tor.camera())
    assert run[3] > 0 and run[3] % 27 == 0 and run[2] < run[3], run[2:]    # 18 whole words + 9


@pytest.mark.gpu
@pytest.mark.parametrize("n_words", [1, 2, 3, 5])
def test_small_segments_with_the_pass_forced(tor, n_words):
    scene, _ = _scene(tor, [32 * n_words], True)
    assert tor.debug_layout_segments(scene.list()) == [(11, 32 * n_words, 32 * n_words, 0), (10, 1, 8, 32 * n_words)]
    run = _same_as_without(tor, f"{n_words} whole words, TOR_PLANE=2", scene, tor.camera(), plane="2")
    assert run[3] > 0 and run[3] % n_words == 0 and run[2] <= run[3], run[2:]
    default = _run(tor, scene, tor.camera())
    assert default[3] == 0 and default[0] == run[0] and np.array_equal(default[1], run[1])   # (too small to be flagged)


def _wide_field(tor, n=480, half=40.0, seed=31):
    rng = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        x, z = rng.uniform(-half, half, 2)
        recs.append([0, x, 0.2, z, x, 0.2, z, 0, 1, 0.2, 0, .5, .5, .5, 0, 0])
    recs.append([0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0])
    recs = np.asarray(recs, dtype=np.float64)
    return tor.Scene.from_records(recs), recs


@pytest.mark.gpu
def test_most_words_skipped_on_most_queries(tor):
    """Straight down on an 80 x 80 field of 480 spheres (15 whole words of ~21 x 16 units each): the camera rays reach a word or
    two, their bounces off the ground and the spheres others -- every pass skips most words, over the words of the query before."""
    scene, _ = _wide_field(tor)
    assert tor.debug_layout_segments(scene.list()) == [(11, 480, 480, 0), (10, 1, 8, 480)]
    cam = tor.camera(look_from=(0.5, 30.0, 0.25), look_at=(0.0, 0.0, 0.0), view_up=(0.0, 0.0, -1.0), vertical_field_of_view=60.0,
                     aperture=0.0, focus_distance=30.0)
    run = _same_as_without(tor, "straight down on a wide field", scene, cam)
    assert run[3] > 0 and run[3] % 15 == 0
    assert run[2] < 0.5 * run[3], run[2:]          # most words skipped


@pytest.mark.gpu
def test_random_scene_alternating_queries_and_hash(tor):
    """random_scene: camera rays graze the whole field (many words reached), their bounces leave it or dive into it (few): stale
    non-zero words sit in the skipped slots of almost every query.  The canvas is the recorded one."""
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    run = _same_as_without(tor, "random_scene", scene, cam)
    assert hashlib.sha256(np.ascontiguousarray(run[1]).tobytes()).hexdigest() == _RANDOM_SCENE_SHA256
    assert 0 < run[2] < run[3] and run[3] % 15 == 0
