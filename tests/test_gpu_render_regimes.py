"""The render kernels across scene regimes on the MI355X: integrate_kernel<SEEDING, ARITH, W, F32, BLOCKS> in every loop family, the
wave-per-pixel kernel and the chain servers against the CPU oracle (PORTABLE math, the accumulation of the stream mode), on the frames
of tests/render_regimes.py -- tiny, far from the world origin, huge, dense clusters, duplicates whose material tells which copy won,
two-level layouts with one and with several time groups, every time group, no ground, non-finite and overflowing objects; cameras
outside and inside the scene, close to the densest spot, 1e6 .. 1e9 units away, and 1e9 units away behind the world origin.  NaNs must sit where the oracle's sit, every
other value is compared as uint64.  tests/test_render_regimes.py shows on the CPU that these frames scatter, tie and overflow enough
to mean something.

Per (regime, camera), 20 x 34 x 6 spp at depth 12, in both stream modes: the lane kernel with accel 0, 1, 2, 3 (and the build it
launched is the one the layout calls for), the brute force without the FMA screen (TOR_SCREEN=0) and with stage one of the plane
screen forced (TOR_PLANE=2), and the wave-per-pixel kernel.  On dense_ties/closeup and groups/outside also the chain hand-off under
"nearly every chain is hot" at 48 spp, a resumed render (3 + 3 samples) and accumulate_device with moments over samples [2, 8).  The
last test asserts that every loop family met the oracle on at least three regimes.

Measured wall time on an MI355X (oracle renders included): the whole module 5.7 s for 49 tests.  test_frame_is_the_oracles: 0.23 s
(dense2/closeup) and 0.22 s (dense/closeup) the slowest, 0.01 .. 0.20 s the others, 3.6 s over its 42 cases;
test_chain_handoff_is_the_oracles 0.06 s and 0.03 s; test_resumed_frame_is_the_oracles and
test_accumulated_sums_and_moments_are_the_oracles 0.01 .. 0.02 s per case; test_every_loop_family_met_the_oracle_on_three_regimes
under 0.005 s.  tests/test_gpu_parity.py::test_accel_fuzz_dense_oracle beside them: 5 s.

What it found when it was written: `tele` at 1e9 failed on dense and groups with TOR_ACCEL_BLOCKS (and groups with both accelerations)
-- the float64 block loop culled rays from origins far beyond the reach within which its boxes cover the reference's rounding -- and
on dense in the wave-per-pixel kernel, whose padding slots (centre 0, r^2 = -1) the reference's rounding "hits" from that far away;
`behind` then failed with TOR_ACCEL_BLOCKS and with TOR_ACCEL_F32 alone (123 .. 312 values): the same padding records behind a ray
that enters every box, or that the float32 filter calls wild.  profiles/render_regimes_mutants.txt: what the sweep fails on."""
import os

import numpy as np
import pytest
import torch

import render_regimes as R

pytestmark = pytest.mark.gpu
SEED = 0
EXTRA_CASES = (("dense_ties", "closeup"), ("groups", "outside"))
HOT = {"TOR_PUSH_THETA": "0.01", "TOR_CHAIN_THETA": "0.01", "TOR_FLOOR_THETA": "0.01"}   # test_chain_handoff_never_changes_a_pixel's
HANDOFF_SPP = 48
KNOBS = ("TOR_MIGRATE", "TOR_SRV_FRAC", "TOR_SRV_MIN_FRAC", "TOR_SRV_PATIENCE_US", "TOR_PUSH_THETA", "TOR_CHAIN_THETA", "TOR_FLOOR_THETA",
         "TOR_TAIL_LANES", "TOR_TAIL_REST", "TOR_MIG_FLAGS", "TOR_SCREEN", "TOR_PLANE", "TOR_WAVES_PER_SIMD")

_held = {f: set() for f in R.FAMILIES}                    # family: the regimes on which it equalled the oracle
_ran = set()
_scenes, _wanted = {}, {}


def _context_under(tor, env):
    """A context created with exactly `env` of the library's launch knobs set (they are read when a context is made)."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        return tor.Context(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def contexts(tor):
    made = {"default": _context_under(tor, {}), "unscreened": _context_under(tor, {"TOR_SCREEN": "0"}),
            "forced": _context_under(tor, {"TOR_PLANE": "2"})}
    yield made
    for ctx in made.values():
        ctx.close()


def _scene(tor, name):
    """(records, Scene, layout over the cameras' ray-time range): built once per regime, never changed."""
    if name not in _scenes:
        recs = R.scene(name, SEED)
        recs.setflags(write=False)
        sc = tor.Scene.from_records(recs)
        lay = tor.debug_accel_layout(sc.list(), min(0.0, R.SHUTTER[0]), max(0.0, R.SHUTTER[1]))
        assert lay is not None
        _scenes[name] = (recs, sc, lay)
    return _scenes[name]


def _camera(tor, oracle, name, cam):
    kw = R.camera(name, cam, _scene(tor, name)[0])
    tcam, ocam = tor.camera(**kw), R.oracle_camera(oracle, kw)
    assert np.array_equal(tcam.as_array(), ocam)
    return tcam, ocam


def _want(tor, oracle, name, cam, seeding, spp=R.SPP):
    """The oracle's canvas: computed once, shared, never changed."""
    key = (name, cam, seeding, spp)
    if key not in _wanted:
        _, ocam = _camera(tor, oracle, name, cam)
        px = oracle.render(R.H, R.W, spp, ocam, _scene(tor, name)[0], max_depth=R.DEPTH, seeding=seeding, math=oracle.MATH_PORTABLE,
                           accum=seeding).pixels
        px.setflags(write=False)
        _wanted[key] = px
    return _wanted[key]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _render(tor, ctx, tcam, spp, **opt):
    buf = torch.zeros((R.H, R.W, 3), dtype=torch.float64, device="cuda")
    ctx.render_device(tcam, R.H, R.W, spp, 2.2, R.DEPTH, tor.make_options(**opt), buf.data_ptr(), _stream())
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _assert_is_the_oracles(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaNs in {int(gn.sum())} places, the oracle's in {int(wn.sum())}; {int((gn != wn).sum())} places differ"
    differ = (got.view(np.uint64) != want.view(np.uint64)) & ~wn
    if differ.any():
        pixels = int(differ.any(axis=2).sum()) if differ.ndim == 3 else int(differ.sum())
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(got - want)))
        raise AssertionError(f"{what}: {int(differ.sum())} values in {pixels} pixels differ from the oracle, max |difference| {worst:.3e}")


def _hold(name, lay, recs, variant, accel):
    for fam in R.families_of(variant, accel, lay[3], len(R.time_groups_in_blocks(recs, lay))):
        _held[fam].add(name)


@pytest.mark.parametrize("name,cam", R.CASES)
def test_frame_is_the_oracles(tor, oracle, contexts, name, cam):
    recs, sc, lay = _scene(tor, name)
    tcam, _ = _camera(tor, oracle, name, cam)
    for ctx in contexts.values():
        ctx.upload(sc.list())
    for seeding in (tor.SEED_PIXEL, tor.SEED_SAMPLE):
        want = _want(tor, oracle, name, cam, seeding)
        ctx = contexts["default"]
        for accel in (0, 1, 2, 3):
            got = _render(tor, ctx, tcam, R.SPP, seeding=seeding, accel=accel, pixel_kernel=tor.PIXEL_KERNEL_LANE)
            v = ctx.last_variant()
            expect = R.expected_variant(recs, lay, accel, seeding)
            assert (v[0], v[1], v[3], v[4]) == expect, f"{name}/{cam} seeding {seeding} accel {accel}: launched {v}, the layout calls for {expect}"
            _assert_is_the_oracles(got, want, f"{name}/{cam} seeding {seeding} accel {accel} (build {v})")
            _hold(name, lay, recs, v, accel)
        for key, screen in (("unscreened", False), ("forced", True)):
            ctx = contexts[key]
            got = _render(tor, ctx, tcam, R.SPP, seeding=seeding, accel=0, pixel_kernel=tor.PIXEL_KERNEL_LANE)
            v = ctx.last_variant()
            expect = R.expected_variant(recs, lay, 0, seeding, screen=screen)
            assert (v[0], v[1], v[3], v[4]) == expect, f"{name}/{cam} seeding {seeding} {key}: launched {v}, expected {expect}"
            _assert_is_the_oracles(got, want, f"{name}/{cam} seeding {seeding} brute force, {key} context")
            _hold(name, lay, recs, v, 0)
    got = _render(tor, contexts["default"], tcam, R.SPP, seeding=tor.SEED_PIXEL, accel=0, pixel_kernel=tor.PIXEL_KERNEL_WAVE)
    _assert_is_the_oracles(got, _want(tor, oracle, name, cam, tor.SEED_PIXEL), f"{name}/{cam} wave-per-pixel kernel")
    _ran.add((name, cam))


@pytest.mark.parametrize("name,cam", EXTRA_CASES)
def test_chain_handoff_is_the_oracles(tor, oracle, name, cam):
    """48 spp through the library's own choice of kernel with nearly every chain hot.  A fresh context: its last_variant says
    whether a lane build ran at all (all -1: the wave-per-pixel kernel took the frame)."""
    recs, sc, lay = _scene(tor, name)
    tcam, _ = _camera(tor, oracle, name, cam)
    ctx = _context_under(tor, HOT)
    try:
        ctx.upload(sc.list())
        got = _render(tor, ctx, tcam, HANDOFF_SPP, seeding=tor.SEED_PIXEL, accel=3)
        v, c = ctx.last_variant(), ctx.last_handoff_counters()
    finally:
        ctx.close()
    _assert_is_the_oracles(got, _want(tor, oracle, name, cam, tor.SEED_PIXEL, HANDOFF_SPP), f"{name}/{cam} hand-off (build {v})")
    print(f"{name}/{cam}: build {v}, pushed {c['pushed']}, served {c['served']}")
    if name == "dense_ties":    # single-level, float32 block records, 73 boxes, 48 spp, 680 pixels: the build with the chain servers must run
        assert R.migrate_variant(v[0], v[3], v[4]), v
    if R.migrate_variant(v[0], v[3], v[4]):
        assert (v[0], v[1], v[3], v[4]) == R.expected_variant(recs, lay, 3, 0)
        assert c["pushed"] > 0 and c["served"] == c["pushed"], (v, c)
    else:
        assert c["pushed"] == 0, (v, c)


@pytest.mark.parametrize("name,cam", EXTRA_CASES)
def test_resumed_frame_is_the_oracles(tor, oracle, contexts, name, cam):
    recs, sc, lay = _scene(tor, name)
    tcam, _ = _camera(tor, oracle, name, cam)
    ctx = contexts["default"]
    ctx.upload(sc.list())
    pp = tor.PixelProgressive(ctx, tcam, R.H, R.W, R.DEPTH, tor.make_options(seeding=tor.SEED_PIXEL, accel=3, pixel_kernel=tor.PIXEL_KERNEL_LANE))
    pp.add(3)
    first = ctx.last_variant()
    pp.add(3)
    v = ctx.last_variant()
    got = pp.image(2.2)
    torch.cuda.synchronize()
    assert first == v and (v[1], v[3], v[4]) == R.expected_variant(recs, lay, 3, 0)[1:] and v[0] not in (0, 1), v   # (a resume build)
    _assert_is_the_oracles(got.cpu().numpy(), _want(tor, oracle, name, cam, tor.SEED_PIXEL), f"{name}/{cam} resumed 3 + 3 (build {v})")


@pytest.mark.parametrize("name,cam", EXTRA_CASES)
def test_accumulated_sums_and_moments_are_the_oracles(tor, oracle, contexts, name, cam):
    recs, sc, lay = _scene(tor, name)
    tcam, ocam = _camera(tor, oracle, name, cam)
    ctx = contexts["default"]
    ctx.upload(sc.list())
    want_s, want_m = oracle.accumulate(R.H, R.W, 2, 6, ocam, recs, max_depth=R.DEPTH)
    assert want_s.std() > 0 and want_m.std() > 0
    for accel in (0, 3):
        sums = torch.zeros((R.H, R.W, 3), dtype=torch.float64, device="cuda")
        mom = torch.zeros_like(sums)
        ctx.accumulate_device(tcam, R.H, R.W, 2, 6, R.DEPTH, tor.make_options(seeding=tor.SEED_SAMPLE, accel=accel, pixel_kernel=tor.PIXEL_KERNEL_LANE),
                              sums.data_ptr(), mom.data_ptr(), _stream())
        torch.cuda.synchronize()
        v = ctx.last_variant()
        assert (v[1], v[3], v[4]) == R.expected_variant(recs, lay, accel, 1)[1:], (accel, v)
        _assert_is_the_oracles(sums.cpu().numpy(), want_s, f"{name}/{cam} accel {accel}: sums of samples [2, 8) (build {v})")
        _assert_is_the_oracles(mom.cpu().numpy(), want_m, f"{name}/{cam} accel {accel}: moments of samples [2, 8) (build {v})")


def test_every_loop_family_met_the_oracle_on_three_regimes():
    """Runs last: counts what test_frame_is_the_oracles held to the oracle (a frame that failed there counts for nothing)."""
    missing = [c for c in R.CASES if c not in _ran]
    for fam in R.FAMILIES:
        print(f"{fam}: {len(_held[fam])} regimes -- {', '.join(sorted(_held[fam]))}")
    assert not missing, f"the count needs every case of test_frame_is_the_oracles to have passed in this run; missing: {missing}"
    for fam in R.FAMILIES:
        assert len(_held[fam]) >= 3, (fam, sorted(_held[fam]))
