"""Stage one of the plane-screened object loop (kernel/integrate_loop_plane.inc) on every shape its three phases take: blocks of 8 up
to a word boundary, whole words two per trip (odd and even counts, the lone last word), blocks to the segment's end (a full block,
a half-real one), a pass that resumes inside a segment, a plane-screened segment at the very end of the plane table and two of them
back to back.  Whatever feeds the loop its records, every case must leave the canvas and the resolve pass's candidates as they are
without any stage one (TOR_PLANE=0), and the canvas must be the oracle's bit for bit.

Scenes: statics of radius 0.2 at one common height per segment (+ a ground sphere): tor_scene.cpp lays one segment per height,
largest first.  A segment below 48 objects is plane-screened only when the screen is forced (TOR_PLANE=2): the one-word case."""
import numpy as np
import pytest

from test_gpu_round4 import _exact
from test_plane32 import _candidates

H, W, SPP = 27, 48, 4


def _scene(tor, sizes, ground=True, seed=11):
    rng = np.random.default_rng(seed)
    recs = []
    for k, n in enumerate(sizes):
        y = 0.2 + 0.01 * k
        for _ in range(n):
            x, z = rng.uniform(-9, 9, 2)
            recs.append([0, x, y, z, x, y, z, 0, 1, 0.2, 0, .5, .5, .5, 0, 0])
    if ground:
        recs.append([0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0])
    recs = np.asarray(recs, dtype=np.float64)
    return tor.Scene.from_records(recs), recs


# (name, objects per height, ground sphere, the layout debug_layout_segments must show: (xkind, objects, slots, first slot))
_CASES = [
    ("one whole word", [32], True, [(11, 32, 32, 0), (10, 1, 8, 32)]),
    ("two whole words: one trip", [64], True, [(11, 64, 64, 0), (10, 1, 8, 64)]),
    ("three whole words: a trip and the lone word", [96], True, [(11, 96, 96, 0), (10, 1, 8, 96)]),
    ("four whole words: two trips", [128], True, [(11, 128, 128, 0), (10, 1, 8, 128)]),
    ("second segment starts off a word boundary", [72, 64], True, [(11, 72, 72, 0), (11, 64, 64, 72), (10, 1, 8, 136)]),
    ("tail of one block", [72], True, [(11, 72, 72, 0), (10, 1, 8, 72)]),
    ("tail of a half-real block", [68], True, [(11, 68, 72, 0), (10, 1, 8, 72)]),
    ("more than 512 slots: a pass resumes inside the segment", [600], True, [(11, 600, 608, 0), (10, 1, 8, 608)]),
    ("plane-screened segment at the end of the table", [96], False, [(11, 96, 96, 0)]),
    ("two plane-screened segments back to back", [104, 100], True, [(11, 104, 104, 0), (11, 100, 104, 104), (10, 1, 8, 208)]),
]


@pytest.mark.parametrize("name,sizes,ground,layout", _CASES, ids=[c[0] for c in _CASES])
def test_layouts_are_the_shapes_the_cases_mean(tor, name, sizes, ground, layout):
    scene, _ = _scene(tor, sizes, ground)
    assert tor.debug_layout_segments(scene.list()) == layout


def test_table_slack_covers_the_read_ahead():
    """One constant states both: the whole-word loop reads kPlaneAhead groups of kPlaneGroupFloats floats behind a segment's last
    record (tor_screen.hpp), and the host keeps kPlaneSlackFloats behind the float32 plane table (tor_scene.cpp)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "trace-of-radiance_amd", "csrc")
    hdr = open(os.path.join(csrc, "tor_screen.hpp")).read()
    ahead = int(re.search(r"#else\s*\nconstexpr int kPlaneAhead = (\d+);", hdr).group(1))
    group = int(re.search(r"constexpr int kPlaneGroupFloats = (\d+);", hdr).group(1))
    slack = int(re.search(r"constexpr int kPlaneSlackFloats = (\d+);", hdr).group(1))
    assert group == 16                      # one s_load_dwordx16: 8 float32 records
    assert slack >= ahead * group and slack >= 2   # (the block phases request one record of 2 floats ahead)
    assert "static_assert(kPlaneSlackFloats >= kPlaneAhead * kPlaneGroupFloats" in hdr
    scene = open(os.path.join(csrc, "tor_scene.cpp")).read()
    assert "out.xpl32.assign(n_xpl + kPlaneSlackFloats," in scene
    loop = open(os.path.join(csrc, "kernel", "integrate_loop_plane.inc")).read()
    assert "kPlaneAhead == 1" in loop       # the loop takes its distance from the same constant


@pytest.mark.gpu
@pytest.mark.parametrize("name,sizes,ground,layout", _CASES, ids=[c[0] for c in _CASES])
def test_stage_one_on_every_loop_shape(tor, oracle, name, sizes, ground, layout):
    scene, recs = _scene(tor, sizes, ground)
    assert tor.debug_layout_segments(scene.list()) == layout
    cam = tor.camera()
    ocam = np.frombuffer(bytes(cam), dtype=np.float64).copy()
    want = oracle.render(H, W, SPP, ocam, recs, seeding=1, math=1, arith=0, accum=1).pixels
    assert float(np.abs(want).sum()) > 0.0
    got, img = _candidates(tor, scene, cam, H, W, SPP, None)
    off, img_off = _candidates(tor, scene, cam, H, W, SPP, "0")
    forced, img_forced = _candidates(tor, scene, cam, H, W, SPP, "2")
    print(f"{name}: candidates default {got}, TOR_PLANE=0 {off}, TOR_PLANE=2 {forced}")
    assert got == off == forced
    assert np.array_equal(img, img_off) and np.array_equal(img_forced, img_off)
    _exact(img, want)
