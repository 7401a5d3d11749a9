"""Stage one of the plane screen in FLOAT32 (tor_screen.hpp plane_seg32 / plane_word32; xkinds 10 / 11 / 12 / 14): on the host,
against the float64 plane screen it stands for -- it must keep every object that one keeps (a superset: everything behind stage one
is unchanged), stay as thin, keep everything where the float64 screen does or its own guarded range ends, and never keep the
table's padding for a ray that has a ground track.  On the GPU: a scene far from the origin against the oracle, and the resolve
pass's candidate count against the float64 stage one's."""
import numpy as np
import pytest

from test_filter32 import _unit


def _sphere(x, y, z, r):
    return [0, x, y, z, x, y, z, 0, 1, r, 0, .5, .5, .5, 0, 0]


def _scenes(tor, rng):
    """random_scene, the host walk's two synthetic scenes (three heights and time groups; a 3-D cloud), as records."""
    out = [("random_scene", tor.random_scene(0xFACADE).to_records())]
    extra = []
    def add(n, y, mover, t0=0.0, t1=1.0):
        for _ in range(n):
            x, z = rng.uniform(-9, 9, 2)
            r = float(rng.choice([0.1, 0.2, 0.4]))
            if mover == 0:
                extra.append(_sphere(x, y, z, r))
            elif mover == 1:
                extra.append([1, x, y, z, x, y + rng.uniform(0, .5), z, t0, t1, r, 0, .5, .5, .5, 0, 0])
            else:
                extra.append([1, x, y, z, x + .3, y, z - .2, t0, t1, r, 0, .5, .5, .5, 0, 0])
    add(41, 0.2, 0); add(7, 0.9, 0); add(19, 0.4, 0); add(53, 0.2, 1); add(12, 0.4, 1, 0.25, 0.75); add(5, 0.3, 1); add(9, 0.2, 2)
    extra.append(_sphere(0, -1000, 0, 1000))
    mixed = np.asarray(extra, dtype=np.float64)
    out.append(("mixed", mixed[rng.permutation(len(mixed))]))
    cloud = [_sphere(0, -1000, 0, 1000)]
    for i in range(240):
        x, z = rng.uniform(-8, 8, 2); y = rng.uniform(0.2, 6.0); r = rng.uniform(0.12, 0.3)
        if i % 3 == 0: cloud.append(_sphere(x, y, z, r))
        elif i % 3 == 1: cloud.append([1, x, y, z, x, y + rng.uniform(0, .5), z, 0.0, 1.0, r, 0, .5, .5, .5, 0, 0])
        else: cloud.append([1, x, y, z, x + rng.uniform(-.4, .4), y + rng.uniform(-.3, .3), z + rng.uniform(-.4, .4), 0.0, 1.0, r, 0, .5, .5, .5, 0, 0])
    out.append(("cloud", np.asarray(cloud, dtype=np.float64)))
    return out


def _translated(recs, shift):
    """The scene moved by `shift` (x, y, z): both centres of every record."""
    t = recs.copy()
    t[:, 1:4] += shift
    t[:, 4:7] += shift
    return t


def _rays(rng, recs, n_rays):
    """Rays that start on or near objects, half of them aimed at another object, over scales of |d|."""
    n_obj = len(recs)
    pick = rng.integers(0, n_obj, n_rays)
    c = recs[pick, 1:4]
    o = c + _unit(rng, n_rays) * (np.minimum(np.abs(recs[pick, 9]), 5.0)[:, None] * rng.choice([1.0, 1.0, 3.0, 40.0], size=(n_rays, 1)))
    d = _unit(rng, n_rays) * rng.choice([1.0, 1e-3, 1e3], size=(n_rays, 1))
    aim = rng.random(n_rays) < 0.5
    tgt = recs[rng.integers(0, n_obj, n_rays), 1:4] + rng.normal(0, 0.1, (n_rays, 3))
    d[aim] = (tgt - o)[aim]
    t = rng.uniform(-0.2, 1.2, n_rays)
    return o, d, t


def _check_superset(keep, name):
    on = keep >= 0
    k64, k32 = (keep & 1) != 0, (keep & 2) != 0
    lost = on & k64 & ~k32
    assert np.count_nonzero(lost) == 0, (name, np.count_nonzero(lost), np.argwhere(lost)[:5])
    return on, k64, k32


def test_float32_stage_one_keeps_what_the_float64_one_keeps(tor):
    """Superset, for every ray x object, on the host walk's scenes and random_scene -- where they are and moved far from the
    origin (centres around +-1e4 and +-1e7: the offsets from the segment's origin stay small, the float64 margins grow)."""
    rng = np.random.default_rng(61)
    for name, recs in _scenes(tor, rng):
        for shift in ((0.0, 0.0, 0.0), (1e4, 0.0, -1e4), (-1e7, 3.0, 1e7)):
            moved = _translated(recs, np.asarray(shift))
            scene = tor.Scene.from_records(moved)
            o, d, t = _rays(rng, moved, 3000)
            keep, _, _ = tor.debug_plane32_scene(scene.list(), o, d, t)
            on, k64, k32 = _check_superset(keep, (name, shift))
            assert np.count_nonzero(on) > 100 * len(t), (name, shift)     # most objects are on float32 segments
            assert np.count_nonzero(k64 & on) > 1000, (name, shift)        # ... and the walk keeps some of them


def test_float32_stage_one_on_the_float64_band_edge(tor):
    """Rays whose ground track passes a sphere at the float64 band's edge, sqrt(R^2 + 2^-45 B^2), to within a relative 2^-16 --
    cut as test_screen.py's test_plane_screen_on_its_own_boundary cuts them (tangent at the equator, any slope) -- on a field of
    statics where it is and far from the origin.  The float64 screen keeps some and drops some of the aimed-at pairs: the rays sit
    on its decision boundary, and the float32 screen still keeps all it keeps."""
    rng = np.random.default_rng(62)
    R = 0.2
    xs, zs = np.meshgrid(np.linspace(-10, 10, 9), np.linspace(-10, 10, 9))
    base = np.asarray([_sphere(x, 0.2, z, R) for x, z in zip(xs.ravel(), zs.ravel())], dtype=np.float64)
    n = 6000
    for shift in (np.zeros(3), np.asarray([1e4, 0.0, -1e4]), np.asarray([-1e7, 0.0, 1e7])):
        recs = _translated(base, shift)
        scene = tor.Scene.from_records(recs)
        pick = rng.integers(0, len(recs), n)
        c = recs[pick, 1:4]
        ang = rng.uniform(0, 2 * np.pi, n)
        u = np.column_stack([np.cos(ang), np.zeros(n), np.sin(ang)])
        nn = np.column_stack([-np.sin(ang), np.zeros(n), np.cos(ang)])
        back = rng.uniform(0.5, 30.0, (n, 1))
        reach = np.max(np.linalg.norm(recs[:, 1:4], axis=1)) + R
        # the ray starts `back` before the tangent point; B = |o|_1 + reach as the screen computes it (near enough: the edge is
        # sampled over a relative 2^-16, the estimate is good to ~1e-15)
        p0 = c + nn * R - u * back
        B = np.abs(p0).sum(axis=1) + reach
        edge = np.sqrt(R * R * (1 + 2.0 ** -40) + B * B * 2.0 ** -45)
        dist = edge * (1.0 + rng.uniform(-1, 1, n) * 2.0 ** -16)
        target = c + nn * dist[:, None]
        slope = rng.choice([0.0, 1e-3, 0.5, 3.0, 1e3], size=(n, 1)) * rng.choice([-1.0, 1.0], size=(n, 1))
        dirn = u + slope * np.array([0.0, 1.0, 0.0])
        o = target - dirn / np.linalg.norm(dirn, axis=1, keepdims=True) * back
        d = (target - o) * rng.choice([1.0, 1e-6, 1e6], size=(n, 1))
        keep, _, _ = tor.debug_plane32_scene(scene.list(), o, d, np.zeros(n))
        _check_superset(keep, shift)
        aimed = keep[np.arange(n), pick]
        assert np.all(aimed >= 0)
        k64 = (aimed & 1) != 0
        assert 0.2 * n < np.count_nonzero(k64) < 0.8 * n, (shift, np.count_nonzero(k64))   # on the float64 boundary


def test_float32_stage_one_keeps_everything_where_it_must(tor):
    """Vertical rays (no ground track), wild rays (|d|^2 out of range), huge or tiny horizontal directions, origins beyond the
    guarded 2^60: every object and every padding slot is kept."""
    rng = np.random.default_rng(63)
    recs = tor.random_scene(0xFACADE).to_records()
    scene = tor.Scene.from_records(recs)
    m = 64
    base_o = np.column_stack([rng.uniform(-11, 11, m), rng.uniform(0.5, 3.0, m), rng.uniform(-11, 11, m)])
    tilt = rng.choice([0.0, 1e-300, 1e-120, 1e-40], size=(m, 2)) * rng.choice([-1.0, 1.0], size=(m, 2))
    vertical = np.column_stack([tilt[:, 0], -np.ones(m), tilt[:, 1]])
    horiz = _unit(rng, m) * np.array([1.0, 0.0, 1.0])
    cases = [("vertical", base_o, vertical), ("tiny |d|", base_o, horiz * 1e-200), ("huge |d|", base_o, horiz * 1e200),
             ("wild", base_o, _unit(rng, m) * 1e-310), ("origin beyond 2^60", base_o + np.array([3e18, 0.0, -3e18]), _unit(rng, m))]
    for name, o, d in cases:
        keep, pad_kept, n_pad = tor.debug_plane32_scene(scene.list(), o, d, rng.uniform(0, 1, m))
        on = keep >= 0
        assert np.count_nonzero(on) > 0 and n_pad > 0
        assert np.all((keep[on] & 2) != 0), name
        assert np.all(pad_kept == n_pad), (name, pad_kept, n_pad)


def test_float32_table_padding_and_band_width(tor):
    """On random_scene: the padding is never kept by a ray with a ground track, and the float32 band keeps on average within 2 %
    of what the float64 band keeps."""
    rng = np.random.default_rng(64)
    recs = tor.random_scene(0xFACADE).to_records()
    scene = tor.Scene.from_records(recs)
    n = 4000
    o = np.column_stack([rng.uniform(-13, 13, n), rng.uniform(0.0, 3.0, n), rng.uniform(-13, 13, n)])
    d = _unit(rng, n)
    d[:, 1] *= 0.9                                          # (no ray closer than ~25 degrees to vertical)
    o[: n // 4] = [13.0, 2.0, 3.0]                          # camera-like rays (scenes.nim's look_from)
    keep, pad_kept, n_pad = tor.debug_plane32_scene(scene.list(), o, d, rng.uniform(0, 1, n))
    on, k64, k32 = _check_superset(keep, "random_scene")
    assert n_pad > 0 and np.all(pad_kept == 0), (n_pad, np.count_nonzero(pad_kept))
    small = np.abs(recs[:, 9]) < 5.0
    n64, n32 = np.count_nonzero(k64[:, small] & on[:, small]), np.count_nonzero(k32[:, small] & on[:, small])
    assert n64 > 5 * n and n32 <= 1.02 * n64, (n64, n32)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

# resolve-pass candidates of random_scene at 54 x 96 x 8 spp (sample streams, depth 50, brute force) with the float64 stage one
# (measured with the library before stage one ran in float32): the float32 stage one must leave exactly as many to the resolve pass
_CANDIDATES_F64_STAGE_ONE = 167645


def _candidates(tor, scene, cam, h, w, spp, plane):
    import os
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
    buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    ctx.render_device(cam, h, w, spp, 2.2, 50, tor.make_options(seeding=tor.SEED_SAMPLE, accel=0), buf.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = ctx.last_stats()
    ctx.close()
    return st.candidates, buf.cpu().numpy()


@pytest.mark.gpu
def test_float32_stage_one_candidates_on_the_gpu(tor):
    """The candidates left to the resolve pass on random_scene: the same with the float32 stage one as without any stage one
    (TOR_PLANE=0) and as with it forced on every segment (TOR_PLANE=2), and the float64 stage one's recorded count."""
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    got, img = _candidates(tor, scene, cam, 54, 96, 8, None)
    off, img_off = _candidates(tor, scene, cam, 54, 96, 8, "0")
    forced, img_forced = _candidates(tor, scene, cam, 54, 96, 8, "2")
    print(f"candidates: default {got}, TOR_PLANE=0 {off}, TOR_PLANE=2 {forced}")
    assert got == off == forced
    assert np.array_equal(img, img_off) and np.array_equal(img, img_forced)
    assert got == _CANDIDATES_F64_STAGE_ONE


@pytest.mark.gpu
def test_far_translated_scene_against_the_oracle(tor, oracle):
    """random_scene moved to (1e4, 0, -1e4) and its camera with it: the canvas is the oracle's bit for bit, with the float32 stage
    one on every segment (TOR_PLANE=2), by default and without it."""
    from test_gpu_round3 import _render_with_env
    from test_gpu_round4 import _exact
    shift = np.array([1e4, 0.0, -1e4])
    recs = _translated(tor.random_scene(0xFACADE).to_records(), shift)
    scene = tor.Scene.from_records(recs)
    cam = tor.camera(look_from=tuple(np.array([13.0, 2.0, 3.0]) + shift), look_at=tuple(shift), aperture=0.1)
    ocam = np.frombuffer(bytes(cam), dtype=np.float64).copy()
    for seeding in (0, 1):
        want = oracle.render(54, 96, 8, ocam, recs, seeding=seeding, math=1, arith=0, accum=seeding).pixels
        assert float(np.abs(want).sum()) > 0.0
        for env in ({}, {"TOR_PLANE": "2"}, {"TOR_PLANE": "0"}):
            got, _ = _render_with_env(tor, scene, cam, 54, 96, 8, env, seeding=seeding, accel=0)
            _exact(got.cpu().numpy(), want)
