"""The reach pass and the word skip of the plane-screened object loop (kernel/integrate_loop_plane.inc, tor_screen.hpp reach_ray)
on the GPU.  The ten shapes of tests/test_gpu_plane_feed.py -- the smallest on which the word walk can go wrong: one word, odd and
even counts, a lone last word, a resume inside a segment past 512 slots, back-to-back segments, a segment at the table's end --
and two of its own: a pass whose every word is skipped (the camera looks at the sky above a field) and passes in which only the
first or only the last word is reached.  For each: the canvas is the oracle's bit for bit, and canvas and candidates are the same
without any stage one (TOR_PLANE=0), with a reach pass that culls nothing (3), by default and with stage one forced (2).  A segment
of movers along y -- random_scene's 481 resting spheres -- against the oracle at the same size; and on the field scenes the skip
walks strictly fewer whole words than it meets."""
import os

import numpy as np
import pytest

from test_gpu_plane_feed import _CASES, _scene
from test_gpu_round4 import _exact

H, W, SPP = 27, 48, 4
# sha256 of random_scene's canvas at 27 x 48 x 4 spp (sample streams, depth 50, float64 little-endian, row-major): the oracle's, which
# is the parent commit's too (its brute force is the oracle's bit for bit at this size: tests/test_gpu_plane_feed.py's contract)
_RANDOM_SCENE_SHA256 = "00bd1aa8a0a7f5651f6e337609a270bac4ffbc5061e8e7ba5263618e170b0044"


def _run(tor, scene, cam, plane):
    """(candidates, canvas, whole words walked, whole words met) of one strict brute-force frame on a context created under TOR_PLANE."""
    import torch
    saved = os.environ.get("TOR_PLANE")
    try:
        if plane is None:
            os.environ.pop("TOR_PLANE", None)
        else:
            os.environ["TOR_PLANE"] = plane
        ctx = tor.Context(0)
    finally:
        if saved is None:
            os.environ.pop("TOR_PLANE", None)
        else:
            os.environ["TOR_PLANE"] = saved
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


def _clusters(tor):
    """Three clusters of 32 resting spheres along the ground's diagonal (+ the ground): in Morton order each is one word."""
    rng = np.random.default_rng(17)
    recs = []
    for k in range(3):
        for _ in range(32):
            x, z = rng.uniform(-1.2, 1.2, 2) + (-8.0 + 8.0 * k)
            recs.append([0, x, 0.2, z, x, 0.2, z, 0, 1, 0.2, 0, .5, .5, .5, 0, 0])
    recs.append([0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0])
    recs = np.asarray(recs, dtype=np.float64)
    return tor.Scene.from_records(recs), recs


def _own_cases(tor):
    """(name, scene, records, camera, words the central camera ray must reach: a set, or None for no statement)"""
    field, field_recs = _scene(tor, [96], True)
    sky = tor.camera(look_from=(0.0, 2.0, 0.0), look_at=(0.5, 12.0, 1.0), aperture=0.0)
    cl, cl_recs = _clusters(tor)
    first = tor.camera(look_from=(-7.0, 4.0, -7.0), look_at=(-8.0, 0.2, -8.0), aperture=0.0)
    last = tor.camera(look_from=(9.0, 4.0, 9.0), look_at=(8.0, 0.2, 8.0), aperture=0.0)
    return [("every word skipped: the sky above a field", field, field_recs, sky, ((0.0, 2.0, 0.0), (0.5, 12.0, 1.0)), set()),
            ("only the first word reached", cl, cl_recs, first, ((-7.0, 4.0, -7.0), (-8.0, 0.2, -8.0)), {0}),
            ("only the last word reached", cl, cl_recs, last, ((9.0, 4.0, 9.0), (8.0, 0.2, 8.0)), {2})]


def _check_modes(tor, oracle, name, scene, recs, cam):
    ocam = np.frombuffer(bytes(cam), dtype=np.float64).copy()
    want = oracle.render(H, W, SPP, ocam, recs, seeding=1, math=1, arith=0, accum=1).pixels
    assert float(np.abs(want).sum()) > 0.0
    runs = {plane: _run(tor, scene, cam, plane) for plane in ("0", "3", None, "2")}
    print(f"{name}: " + ", ".join(f"TOR_PLANE={k}: candidates {v[0]}, words walked {v[2]} of {v[3]}" for k, v in runs.items()))
    for plane, (cand, img, walked, met) in runs.items():
        assert cand == runs["0"][0], (name, plane)
        assert np.array_equal(img, runs["0"][1]), (name, plane)
        assert walked <= met
    assert runs["0"][3] == 0                               # no stage one: no whole word met
    assert runs["3"][2] == runs["3"][3]                    # every lane reaches everything: every word met by the pass is walked
    _exact(runs[None][1], want)
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("name,sizes,ground,layout", _CASES, ids=[c[0] for c in _CASES])
def test_word_skip_on_every_loop_shape(tor, oracle, name, sizes, ground, layout):
    scene, recs = _scene(tor, sizes, ground)
    assert tor.debug_layout_segments(scene.list()) == layout
    runs = _check_modes(tor, oracle, name, scene, recs, tor.camera())
    # the skip walks strictly fewer whole words than it meets.  By default the pass runs on segments of at least eight whole words
    # (tor_scene.cpp: the [600] shape); TOR_PLANE=2 runs it on every segment, which is what puts the small shapes through it
    assert runs["2"][3] > 0 and runs["2"][2] < runs["2"][3], (name, runs["2"][2:])
    if sizes == [600]:
        assert runs[None][3] > 0 and runs[None][2] < runs[None][3], (name, runs[None][2:])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1, 2], ids=["sky", "first word", "last word"])
def test_word_skip_own_shapes(tor, oracle, case):
    name, scene, recs, cam, (look_from, look_at), want_words = _own_cases(tor)[case]
    # what the central camera ray reaches, from the host mirror of the same functions
    o = np.asarray([look_from]); d = np.asarray([look_at]) - o
    reach, word, _, _ = tor.debug_reach_scene(scene.list(), o, d, np.zeros(1))
    words = sorted(set(word[word >= 0].tolist()))
    assert len(words) == 3
    reached = {words.index(w) for w in words if reach[0, np.flatnonzero(word == w)[0]] != 0}
    assert reached == want_words, (name, reached)
    runs = _check_modes(tor, oracle, name, scene, recs, cam)
    assert runs["2"][3] > 0 and runs["2"][2] < runs["2"][3]  # (three words: the pass runs when forced, TOR_PLANE=2)
    if case == 0:
        assert runs["2"][2] == 0 and runs["2"][0] == 0      # the sky: nothing walked, no candidate


@pytest.mark.gpu
def test_y_mover_segment_against_the_oracle(tor, oracle):
    """random_scene -- one segment of 481 movers along y and resting statics, xkind 12 -- at 27 x 48: the canvas the oracle gives, in
    every mode, the recorded hash of that canvas, and fewer words walked than met."""
    scene = tor.random_scene(0xFACADE)
    recs, _ = oracle.random_scene(0xFACADE)
    assert tor.debug_layout_segments(scene.list())[0][0] == 12
    runs = _check_modes(tor, oracle, "random_scene", scene, recs, tor.camera())
    assert runs[None][2] < runs[None][3]
    import hashlib
    for plane, run in runs.items():
        assert hashlib.sha256(np.ascontiguousarray(run[1]).tobytes()).hexdigest() == _RANDOM_SCENE_SHA256, plane
