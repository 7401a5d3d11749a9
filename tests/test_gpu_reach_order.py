"""The even-split order of the segments the reach pass runs on (tor_scene.cpp) on the GPU, at 27 x 48, 4 spp, depth 50, sample
streams, brute force: on the [600] field of tests/test_gpu_plane_feed.py and on the two flagged segments of
tests/test_reach_order.py (the second begins off a word boundary) the canvas and the candidates are the same under the default
order, under TOR_REACH_ORDER=morton and without stage one (TOR_PLANE=0), and the canvas is the oracle's bit for bit; the default
order walks no more whole words than the Morton order on the field and meets as many; random_scene's canvas has the hash
tests/test_gpu_reach.py records, under both orders."""
import contextlib
import hashlib
import os

import numpy as np
import pytest

from test_gpu_plane_feed import _scene
from test_gpu_reach import _RANDOM_SCENE_SHA256
from test_gpu_round4 import _exact
from test_reach_order import two_segments

H, W, SPP = 27, 48, 4


@contextlib.contextmanager
def _env(**values):
    saved = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(tor, scene, cam, order=None, plane=None):
    """(candidates, canvas, whole words walked, whole words met) of one strict brute-force frame.  TOR_PLANE is read when the context
    is created, TOR_REACH_ORDER when the layout is built, which is at the first launch after the upload."""
    import torch
    with _env(TOR_PLANE=plane, TOR_REACH_ORDER=order):
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


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["field of 600", "two segments"])
def test_the_order_changes_no_candidate_and_no_pixel(tor, oracle, case):
    if case == "field of 600":
        scene, recs = _scene(tor, [600], True)
        assert tor.debug_layout_segments(scene.list()) == [(11, 600, 608, 0), (10, 1, 8, 608)]
    else:
        recs = two_segments()
        scene = tor.Scene.from_records(recs)
        assert tor.debug_layout_segments(scene.list()) == [(11, 584, 584, 0), (12, 320, 320, 584), (10, 1, 8, 904)]
    cam = tor.camera()
    ocam = np.frombuffer(bytes(cam), dtype=np.float64).copy()
    want = oracle.render(H, W, SPP, ocam, recs, seeding=1, math=1, arith=0, accum=1).pixels
    assert float(np.abs(want).sum()) > 0.0
    split = _run(tor, scene, cam)
    morton = _run(tor, scene, cam, order="morton")
    off = _run(tor, scene, cam, plane="0")
    print(f"{case}: candidates {split[0]}; whole words walked {split[2]} of {split[3]}, Morton order {morton[2]} of {morton[3]}")
    assert split[0] == morton[0] == off[0]
    assert np.array_equal(split[1], off[1]) and np.array_equal(morton[1], off[1])
    _exact(split[1], want)
    assert off[3] == 0                                       # no stage one: no whole word met
    assert split[3] == morton[3] > 0                         # the pass runs, in front of the same words
    assert split[2] < split[3]
    if case == "field of 600":
        assert split[2] <= morton[2]


@pytest.mark.gpu
def test_random_scene_hash_under_both_orders(tor):
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    for order in (None, "morton"):
        cand, img, walked, met = _run(tor, scene, cam, order=order)
        print(f"random_scene, TOR_REACH_ORDER={order}: candidates {cand}, whole words walked {walked} of {met}")
        assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == _RANDOM_SCENE_SHA256, order
        assert 0 < walked < met
