"""GPU parity: the HIP integrator (through the C ABI) against the CPU oracle on the same
inputs.  The oracle's PORTABLE math mode is the bit-level twin of the kernel's math (the
oracle's LIBM mode is what the golden PNG pins; tests/test_oracle_* tie the two together).

Stated tolerance (BASELINE.json north_star): per-channel |delta| <= 1e-5 on the float64 canvas.
The kernel is built to do better -- bit-exact -- and the tests assert that too."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _render(tor, scene, cam, h, w, spp, depth=50, **opt):
    # small TOR_SEED_PIXEL frames would run the wave-per-pixel kernel, which ignores `accel`: a test that names an
    # acceleration means the lane kernel (the wave kernel has its own tests and is what every accel-less call below runs)
    if "accel" in opt and opt.get("seeding", tor.SEED_PIXEL) == tor.SEED_PIXEL and "pixel_kernel" not in opt:
        opt["pixel_kernel"] = tor.PIXEL_KERNEL_LANE
    cv = tor.new_canvas(h, w, spp, 2.2)
    tor.render(cv, cam, scene.list(), depth, tor.make_options(**opt) if opt else None)
    return cv


def _assert_parity(got, want, exact=True):
    assert np.all(np.isfinite(got))
    err = float(np.max(np.abs(got - want)))
    assert err <= TOL, f"max per-channel error {err} > {TOL}"
    if exact:
        assert np.array_equal(got, want), f"not bit-exact (max err {err}, {(got != want).sum()} values differ)"


def test_device_math_is_bit_identical_to_oracle(tor, oracle):
    L = oracle.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.random(400000) * (2.0 * 3.141592653589793),
                        np.array([0.0, 1e-300, np.pi / 2, np.pi, np.nextafter(2 * np.pi, 0)])])
    s, c = tor.selftest_math(0, a)
    s2 = np.empty_like(a); c2 = np.empty_like(a)
    L.oracle_port_sincos(dp(a), dp(s2), dp(c2), a.size)
    assert np.array_equal(s, s2) and np.array_equal(c, c2)
    x = rng.random(400000) * 2.0
    p, _ = tor.selftest_math(1, x)
    p2 = np.empty_like(x); L.oracle_port_pow5(dp(x), dp(p2), x.size)
    assert np.array_equal(p, p2)
    g = 1.0 / float(np.float32(2.2))
    xx = np.concatenate([rng.random(200000), rng.random(200000) * 1e-7, np.array([0.0, 1.0, 2.0 ** -48])])
    p, _ = tor.selftest_math(2, xx, np.full_like(xx, g))
    p2 = np.empty_like(xx); L.oracle_port_pow(dp(xx), g, dp(p2), xx.size)
    assert np.array_equal(p, p2)
    # IEEE correctly rounded sqrt and division on the device (the path relies on both)
    y = np.concatenate([rng.random(300000) * 1e3, 10.0 ** rng.uniform(-300, 300, 100000)])
    r, _ = tor.selftest_math(3, y)
    assert np.array_equal(r, np.sqrt(y))
    num = rng.standard_normal(400000) * 10.0 ** rng.uniform(-100, 100, 400000)
    den = rng.standard_normal(400000) * 10.0 ** rng.uniform(-100, 100, 400000)
    r, _ = tor.selftest_math(4, num, den)
    assert np.array_equal(r, num / den)
    q, _ = tor.selftest_math(5, x)
    assert np.array_equal(q[:2000], np.array([L.oracle_quantize36(float(v)) for v in x[:2000]]))
    from output_restatement import quantize36
    assert np.array_equal(q, quantize36(x))                   # all 400 000 against the restatement (held to the rational statement on the CPU)
    u, ux = tor.selftest_math(6, x, x[::-1].copy())
    uh, uxh = tor.selftest_math(6, x, x[::-1].copy(), where="host")
    assert np.array_equal(u, uh) and np.array_equal(ux, uxh)
    uo, uxo = oracle.unit_vector_probe(x, x[::-1].copy())      # ... and against the oracle's unit vector (vec3s.nim:106-107)
    assert np.array_equal(u, uo) and np.array_equal(ux, uxo)


@pytest.mark.parametrize("arith", [0])   # (round 5: TOR_ARITH_FUSED removed)
def test_pixel_seeding_matches_oracle(tor, oracle, ref_scene, ref_camera, golden_dir, arith):
    """TOR_SEED_PIXEL = the reference's stream layout (render.nim:59-67)."""
    objs, _ = ref_scene
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    cv = _render(tor, scene, cam, 36, 64, 16, seeding=tor.SEED_PIXEL, arith=arith)
    want = np.load(os.path.join(golden_dir, "small_canvases.npz"))[f"c_0_1_{arith}_0"]
    _assert_parity(cv.pixels, want)
    live = oracle.render(36, 64, 16, ref_camera, objs, seeding=0, math=1, arith=arith).pixels
    _assert_parity(cv.pixels, live)


@pytest.mark.parametrize("arith", [0])   # (round 5: TOR_ARITH_FUSED removed)
def test_sample_seeding_matches_oracle(tor, oracle, ref_scene, ref_camera, golden_dir, arith):
    """TOR_SEED_SAMPLE: one lane per pixel-sample, counter-based streams, exact accumulation."""
    objs, _ = ref_scene
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    cv = _render(tor, scene, cam, 36, 64, 16, seeding=tor.SEED_SAMPLE, arith=arith)
    z = np.load(os.path.join(golden_dir, "small_canvases.npz"))
    _assert_parity(cv.pixels, z[f"c_1_1_{arith}_1"])                 # quantised accumulation: exact
    _assert_parity(cv.pixels, z[f"c_1_1_{arith}_0"], exact=False)    # sequential float64 sum: 1e-5
    assert float(np.max(np.abs(cv.pixels - z[f"c_1_1_{arith}_0"]))) < 1e-8
    _assert_parity(cv.pixels, z[f"c_1_0_{arith}_0"], exact=False)    # libm oracle: 1e-5


def _png_budget(oracle, ref_scene, ref_camera, golden):
    """How many 8-bit channels the oracle's two math modes differ in at C1 ON THIS BOX, and whether its pinned
    (LIBM) mode reproduces the reference PNG here.  The GPU is bit-identical to the PORTABLE mode, so this -- not
    a fixed allowance -- is what its image may differ from the PNG by (measured: 0 and True)."""
    objs, _ = ref_scene
    libm = oracle.render(216, 384, 100, ref_camera, objs, seeding=0, math=0, arith=0).pixels
    port = oracle.render(216, 384, 100, ref_camera, objs, seeding=0, math=1, arith=0).pixels
    q_libm, q_port = oracle.quantize_ppm(libm), oracle.quantize_ppm(port)
    return libm, port, bool(np.array_equal(q_libm, golden)), int((q_libm != q_port).sum())


def test_c1_reference_image(tor, oracle, ref_scene, ref_camera, golden_dir):
    """BASELINE config C1 (384x216, 100 spp, depth 50) == trace_of_radiance.nim main(), through tor_render() (the
    reference's signature; exact accelerations on by default) and with the float64 brute force.
      GPU float64 canvas == oracle(PORTABLE) bit for bit;
      GPU float64 canvas vs the PINNED oracle mode (LIBM, the one that reproduces the PNG): <= 1e-5 stated,
        and in fact within a few ulp (the max is printed);
      GPU 8-bit image vs the reference's PNG: 0 differing channels whenever oracle(LIBM) reproduces the PNG on
        this box, never more than the oracle's own LIBM-vs-PORTABLE count."""
    g = np.array(Image.open(os.path.join(golden_dir, "book2_motion_blur.png")).convert("RGB"))
    libm, port, libm_is_png, budget = _png_budget(oracle, ref_scene, ref_camera, g)
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    for opts in (None, dict(seeding=tor.SEED_PIXEL, accel=0)):
        cv = tor.new_canvas(216, 384, 100, 2.2)
        tor.render(cv, cam, scene.list(), 50, tor.make_options(**opts) if opts else None)
        _assert_parity(cv.pixels, port)
        err = float(np.max(np.abs(cv.pixels - libm)))
        print(f"C1 GPU vs oracle(LIBM): max |delta| = {err:.3e}")
        assert err <= TOL and err < 1e-12
        rgb = tor.export_rgb8(cv)
        differ = int((rgb != g).sum())
        assert differ <= budget, f"{differ} 8-bit channels differ from the reference PNG (oracle LIBM-vs-PORTABLE: {budget})"
        if libm_is_png:
            assert differ == 0, f"{differ} of {g.size} 8-bit channels differ from the reference PNG"
        # the DEVICE quantiser (io/ppm.nim:15-16) on the same canvas against the PNG and the oracle's quantiser
        import torch
        ctx = tor.Context()
        dev = torch.from_numpy(cv.pixels).cuda()
        out = torch.empty((216, 384, 3), dtype=torch.uint8, device="cuda")
        ctx.quantize_rgb8_device(dev.data_ptr(), dev.numel(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dq = out.cpu().numpy()[::-1]                       # canvas row 0 = bottom scanline (io/ppm.nim:20)
        assert np.array_equal(dq, oracle.quantize_ppm(cv.pixels))
        assert int((dq != g).sum()) <= budget and (not libm_is_png or np.array_equal(dq, g))
        ctx.close()


def test_pixel_seeding_cost_ordered_schedule(tor, oracle, ref_scene, ref_camera):
    """spp >= 32 switches SEED_PIXEL to the probe + cost-ordered (LPT) tile schedule; the schedule must
    never change a pixel.  37x45 = 1665 pixels = 26 tiles + a partial one."""
    objs, _ = ref_scene
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    cv = _render(tor, scene, cam, 37, 45, 32, seeding=tor.SEED_PIXEL)
    want = oracle.render(37, 45, 32, ref_camera, objs, seeding=0, math=1, arith=0).pixels
    _assert_parity(cv.pixels, want)
    cv = _render(tor, scene, cam, 37, 45, 33, seeding=tor.SEED_PIXEL, shard_index=1, shard_count=2, row_tile=4)
    want = oracle.render(37, 45, 33, ref_camera, objs, seeding=0, math=1, arith=0).pixels
    rows = tor.shard_rows(37, 4, 1, 2)
    _assert_parity(cv.pixels[rows], want[rows])


def test_high_spp_sums_stay_exact(tor, oracle, ref_scene, ref_camera):
    """BASELINE config C4 uses 4096 spp: the 2^-36-quantised per-pixel sums must stay exact (sum < 2^17)."""
    objs, _ = ref_scene
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    cv = _render(tor, scene, cam, 6, 10, 4096, seeding=tor.SEED_SAMPLE)
    want = oracle.render(6, 10, 4096, ref_camera, objs, seeding=1, math=1, arith=0, accum=1).pixels
    _assert_parity(cv.pixels, want)


ACCELS = (1, 2, 3)   # TOR_ACCEL_BLOCKS, TOR_ACCEL_F32, both


@pytest.mark.parametrize("accel", ACCELS)
def test_block_culling_never_changes_a_pixel(tor, oracle, ref_scene, ref_camera, accel):
    """TOR_ACCEL_BLOCKS (spatial blocks of 8 objects behind conservative boxes) and
    TOR_ACCEL_F32 (conservative packed-float32 pre-filter in front of the float64 test).  Closest hit is
    order independent (hittables_lists.nim:48-55) and every kept object goes through the float64 test, so
    the canvases must be bit-identical to the brute-force path and to the oracle -- random_scene (395
    moving + 90 static spheres), an animated frame (1601 static spheres), and a scene with several time
    groups, general movers, overlapping, duplicate and negative-radius spheres."""
    objs, _ = ref_scene
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    for seeding in (tor.SEED_PIXEL, tor.SEED_SAMPLE):
        for arith in (0,):
            base = _render(tor, scene, cam, 36, 64, 16, seeding=seeding, arith=arith)
            acc = _render(tor, scene, cam, 36, 64, 16, seeding=seeding, arith=arith, accel=accel)
            assert np.array_equal(acc.pixels, base.pixels), (seeding, arith)
        want = oracle.render(36, 64, 16, ref_camera, objs, seeding=seeding, math=1, arith=0, accum=seeding).pixels
        acc = _render(tor, scene, cam, 36, 64, 16, seeding=seeding, accel=accel)
        _assert_parity(acc.pixels, want)
    # animated frame
    cam2, scene2, _ = next(iter(tor.Animation(27, 48, 0.005, 0.3, 2.0).scenes(6)))
    base = _render(tor, scene2, cam2, 27, 48, 8, seeding=tor.SEED_SAMPLE)
    acc = _render(tor, scene2, cam2, 27, 48, 8, seeding=tor.SEED_SAMPLE, accel=accel)
    assert np.array_equal(acc.pixels, base.pixels)
    # synthetic: 300 objects, 3 time groups (one general mover group), duplicates, hollow spheres, big ones
    rng = np.random.default_rng(5)
    recs = [[0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0]]
    for i in range(300):
        x, z = rng.uniform(-9, 9, 2)
        kind = i % 4
        mat = [0, 1, 2][i % 3]
        r = 0.25 if i % 17 else -0.25
        if kind == 0:
            recs.append([0, x, .25, z, x, .25, z, 0, 1, r, mat, .6, .5, .4, 0.2, 1.5])
        elif kind == 1:
            recs.append([1, x, .25, z, x, .25 + rng.uniform(0, .6), z, 0.0, 1.0, r, mat, .3, .7, .4, 0.1, 1.5])
        elif kind == 2:
            recs.append([1, x, .25, z, x + rng.uniform(-.5, .5), .4, z + rng.uniform(-.5, .5), 0.25, 0.75, r, mat, .3, .3, .8, 0.0, 1.4])
        else:
            recs.append([1, x, .25, z, x, .25, z + .3, -1.0, 2.0, r, mat, .8, .3, .3, 0.4, 1.3])
    recs.append(recs[5])                                                    # exact duplicate
    recs.append([0, 0, 1, 0, 0, 1, 0, 0, 1, 1.0, 2, 0, 0, 0, 0, 1.5])       # big glass sphere
    recs.append([1, 3, .3, 3, 3, .9, 3, 0.5, 0.5, 0.3, 0, .1, .9, .1, 0, 0])  # time0 == time1: never hit
    scene3, recs3 = _custom_scene(tor, oracle, recs)
    for seeding in (0, 1):
        base = _render(tor, scene3, cam, 30, 52, 12, seeding=seeding)
        acc = _render(tor, scene3, cam, 30, 52, 12, seeding=seeding, accel=accel)
        assert np.array_equal(acc.pixels, base.pixels), seeding
        want = oracle.render(30, 52, 12, ref_camera, recs3, seeding=seeding, math=1, arith=0, accum=seeding).pixels
        _assert_parity(acc.pixels, want)


def test_row_sharding_is_exact(tor):
    """Any row partition gives the same pixels: shards written in place."""
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    for seeding in (tor.SEED_PIXEL, tor.SEED_SAMPLE):
        full = _render(tor, scene, cam, 45, 80, 8, seeding=seeding).pixels
        for count, tile in ((2, 1), (3, 4), (8, 2), (4, 16)):
            cv = tor.new_canvas(45, 80, 8, 2.2)
            cv.pixels[:] = -1.0
            for k in range(count):
                tor.render(cv, cam, scene.list(), 50,
                           tor.make_options(seeding=seeding, shard_index=k, shard_count=count, row_tile=tile))
            assert np.array_equal(cv.pixels, full), (seeding, count, tile)


def _custom_scene(tor, oracle, recs):
    recs = np.asarray(recs, dtype=np.float64)
    return tor.Scene.from_records(recs), recs


def test_edge_cases_match_oracle(tor, oracle, ref_camera):
    cam = tor.camera()
    # kind c0 c1 t0 t1 radius mat albedo fuzz ri
    recs = [
        [0, 0, -1000, 0, 0, -1000, 0, 0, 1, 1000, 0, .5, .5, .5, 0, 0],
        [1, 0, 1, 0, 0, 1.5, 0, 0.0, 1.0, 1.0, 0, .8, .3, .3, 0, 0],       # group (0,1)
        [1, -4, 1, 0, -4, 1, 1, 0.25, 0.75, 1.0, 1, .7, .6, .5, 0.3, 0],   # group (.25,.75), moves in z
        [1, 4, 1, 0, 5, 1, 0, 0.25, 0.75, 1.0, 2, 0, 0, 0, 0, 1.5],        # same group, glass, moves in x
        [1, 2, .5, 2, 2, .5, 2, 0.5, 0.5, 0.5, 0, .1, .9, .1, 0, 0],       # time0 == time1: never hit
        [0, 1, .4, 3, 1, .4, 3, 0, 1, 0.4, 1, .9, .9, .9, 0.0, 0],
        [0, 1, .4, 3, 1, .4, 3, 0, 1, 0.4, 0, .2, .2, .9, 0.0, 0],         # exact duplicate: tie -> lowest index
        [0, -1, .3, 2, -1, .3, 2, 0, 1, -0.3, 2, 0, 0, 0, 0, 1.5],         # negative radius (hollow glass)
    ]
    scene, recs = _custom_scene(tor, oracle, recs)
    for (h, w, spp, depth) in ((24, 40, 8, 50), (2, 2, 4, 50), (7, 13, 3, 1), (9, 5, 2, 2), (16, 16, 1, 50)):
        for seeding in (0, 1):
            cv = _render(tor, scene, cam, h, w, spp, depth, seeding=seeding)
            want = oracle.render(h, w, spp, ref_camera, recs, max_depth=depth, seeding=seeding, math=1,
                                 arith=0, accum=seeding).pixels
            _assert_parity(cv.pixels, want)
    # empty world: sky only (HittableList of length 0)
    empty = tor.Scene()
    cv = _render(tor, empty, cam, 8, 8, 4, seeding=0)
    want = oracle.render(8, 8, 4, ref_camera, np.zeros((0, 16)), seeding=0, math=1).pixels
    _assert_parity(cv.pixels, want)
    # max_depth = 0: the bounce loop never runs -> black canvas (render.nim:25,47)
    cv = _render(tor, scene, cam, 8, 8, 4, 0)
    assert np.array_equal(cv.pixels, np.zeros((8, 8, 3)))
    # queue overflow path: every sphere encloses the camera -> all 300 are candidates -> 38 mask entries
    # per lane against a queue of 16: the object loop has to stop, resolve and resume (twice)
    big = [[0, 13, 2, 3, 13, 2, 3, 0, 1, 5.0 + 0.01 * i, 2, 0, 0, 0, 0, 1.5] for i in range(300)]
    scene2, recs2 = _custom_scene(tor, oracle, big)
    want = oracle.render(6, 6, 2, ref_camera, recs2, max_depth=8, seeding=1, math=1, accum=1).pixels
    for accel in (0, 1, 2, 3):
        cv = _render(tor, scene2, cam, 6, 6, 2, 8, seeding=1, accel=accel)
        _assert_parity(cv.pixels, want)


def test_invalid_arguments_fail_loudly(tor):
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    for (h, w, spp) in ((1, 8, 1), (8, 1, 1), (8, 8, 0)):
        cv = tor.new_canvas(h, w, spp, 2.2)
        cv.pixels[:] = 7.0
        with pytest.raises(tor.TorError):
            tor.render(cv, cam, scene.list(), 50)
        assert np.all(cv.pixels == 7.0)  # never a partial canvas
    with pytest.raises(tor.TorError):
        tor.render(tor.new_canvas(4, 4, 1), cam, scene.list(), 50, tor.make_options(shard_index=3, shard_count=2))


def test_full_size_rows_match_oracle(tor, oracle, ref_scene, ref_camera):
    """BASELINE config C2 (1920x1080x100 spp) on the GPU; the oracle renders 5 of its rows (bottom, the
    sphere field, the glass ball, horizon, sky) and those rows must match bit for bit."""
    import torch
    objs, _ = ref_scene
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context()
    ctx.upload(scene.list())
    h, w, spp = 1080, 1920, 100
    rows = [0, 377, 540, 731, 1079]
    for seeding in (tor.SEED_SAMPLE, tor.SEED_PIXEL):
        buf = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        ctx.render_device(cam, h, w, spp, 2.2, 50, tor.make_options(seeding=seeding), buf.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        for r in rows:
            want = oracle.render(h, w, spp, ref_camera, objs, seeding=seeding, math=1, arith=0, accum=seeding,
                                 rows=(r, r + 1)).pixels[r]
            _assert_parity(got[r], want)
    ctx.close()


def test_full_size_properties(tor):
    """BASELINE config C2 geometry (1920x1080), size-independent properties: determinism,
    shard invariance of the device path, finite values in range, quantiser idempotence."""
    import torch
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context()
    ctx.upload(scene.list())
    h, w, spp = 1080, 1920, 8
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    for rep in range(2):
        buf = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        ctx.render_device(cam, h, w, spp, 2.2, 50, tor.make_options(seeding=tor.SEED_SAMPLE), buf.data_ptr(), stream)
        torch.cuda.synchronize()
        outs.append(buf)
    assert torch.equal(outs[0], outs[1])                      # atomics order does not matter
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].min()) >= 0.0 and float(outs[0].max()) <= 1.0 + 1e-12
    parts = torch.full((h, w, 3), -1.0, dtype=torch.float64, device="cuda")
    for k in range(4):
        rows = torch.from_numpy(tor.shard_rows(h, 8, k, 4)).long().cuda()
        shard = torch.empty((len(rows), w, 3), dtype=torch.float64, device="cuda")
        ctx.render_device(cam, h, w, spp, 2.2, 50,
                          tor.make_options(seeding=tor.SEED_SAMPLE, shard_index=k, shard_count=4, row_tile=8),
                          shard.data_ptr(), stream)
        torch.cuda.synchronize()
        parts[rows] = shard
    assert torch.equal(parts, outs[0])
    rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    ctx.quantize_rgb8_device(outs[0].data_ptr(), outs[0].numel(), rgb.data_ptr(), stream)
    torch.cuda.synchronize()
    ref = (256 * outs[0].clamp(0.0, 0.999)).to(torch.int32).to(torch.uint8)
    assert torch.equal(rgb, ref)
    from oracle import oracle as O
    assert np.array_equal(rgb.cpu().numpy()[::-1], O.quantize_ppm(outs[0].cpu().numpy()))   # io/ppm.nim:14-27 restated in C
    ms, n = ctx.last_kernel_ms()
    assert n == (h // 4 + 0) * 0 + len(tor.shard_rows(h, 8, 3, 4)) * w * spp and ms > 0
    ctx.close()


def test_host_canvas_rate(tor):
    """tor_render_opt on host buffers (what a Nim caller pays: scene upload + kernel + sync + D2H of
    the canvas).  Records the PCIe-inclusive rate next to the resident-buffer rate in
    gpurun_out/host_canvas_rate.json; it is never the bench value."""
    import json
    import time
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    h, w, spp = 1080, 1920, 20
    opt = tor.make_options(seeding=tor.SEED_SAMPLE)
    cv = tor.new_canvas(h, w, spp, 2.2)
    tor.render(cv, cam, scene.list(), 50, opt)  # warm-up: context creation, first launch
    t = time.perf_counter()
    tor.render(cv, cam, scene.list(), 50, opt)
    dt = time.perf_counter() - t
    rate = h * w * spp / dt / 1e6
    assert np.all(np.isfinite(cv.pixels)) and rate > 50.0
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "host_canvas_rate.json"), "w") as f:
            json.dump({"workload": f"{w}x{h}x{spp}spp", "seconds": dt, "msamples_per_s_pcie_inclusive": rate}, f)


def test_c_host_example_reproduces_reference_image(tor, golden_dir, tmp_path):
    """examples/trace_of_radiance_main.cpp is the reference's main() (trace_of_radiance.nim:26-71) on the
    bare C ABI -- no Python, no torch, the system HIP runtime.  Its PPM must be the reference's image."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler on this box")
    exe = str(tmp_path / "trace_of_radiance")
    libdir = os.path.dirname(tor.LIB_PATH)
    subprocess.run(["g++", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "trace_of_radiance_main.cpp"),
                    "-L", libdir, "-ltor_mi355x", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    tok = r.stdout.split()
    assert tok[0] == b"P3" and (int(tok[1]), int(tok[2]), int(tok[3])) == (384, 216, 255)
    rgb = np.array(tok[4:], dtype=np.int64).reshape(216, 384, 3)
    g = np.array(Image.open(os.path.join(golden_dir, "book2_motion_blur.png")).convert("RGB")).astype(np.int64)
    differ = int((rgb != g).sum())
    assert differ == 0, f"{differ} 8-bit channels differ from the reference PNG"


def _random_records(rng, n, spread, with_big):
    recs = []
    if with_big:
        recs.append([0, 0, -500, 0, 0, -500, 0, 0, 1, 500, 0, .5, .5, .5, 0, 0])
    groups = [(0.0, 1.0), (-0.5, 0.5), (0.25, 2.0), (1.0, 0.0)]          # the last one runs backwards
    while len(recs) < n:
        x, y, z = rng.uniform(-spread, spread), rng.uniform(0.0, 0.3 * spread), rng.uniform(-spread, spread)
        r = float(rng.choice([0.15, 0.2, 0.3, 0.45])) * (1 if rng.random() > 0.05 else -1)
        mat = int(rng.integers(0, 3))
        alb = rng.uniform(0.1, 0.95, 3)
        fuzz, ri = rng.uniform(0, 0.6), rng.uniform(1.2, 1.8)
        k = rng.random()
        if k < 0.4:
            recs.append([0, x, y, z, x, y, z, 0, 1, r, mat, *alb, fuzz, ri])
        else:
            t0, t1 = groups[int(rng.integers(0, len(groups)))]
            d = rng.uniform(-0.6, 0.6, 3) if k < 0.8 else np.array([0.0, rng.uniform(0, 0.7), 0.0])
            recs.append([1, x, y, z, x + d[0], y + d[1], z + d[2], t0, t1, r, mat, *alb, fuzz, ri])
    if with_big:
        recs.append([0, 1, 2.5, -1, 1, 2.5, -1, 0, 1, 2.5, 2, 0, 0, 0, 0, 1.5])
    return np.asarray(recs, dtype=np.float64)


def test_block_culling_randomised_scenes(tor, oracle):
    """Property test for TOR_ACCEL_BLOCKS: on random scenes (64..420 objects, static / y-only / general
    movers in four time groups incl. time1 < time0, hollow spheres, optional huge objects), cameras
    outside and INSIDE the object cloud, and shutters that reach outside every [time0, time1], the
    culled render is bit-identical to the brute-force render; one configuration per scene is also
    checked against the oracle."""
    rng = np.random.default_rng(20260928)
    for trial in range(16):
        # the last two scenes are large enough (> 96 blocks) for the second box level
        n = int(rng.integers(64, 420)) if trial < 14 else int(rng.integers(900, 1300))
        spread = float(rng.choice([3.0, 6.0, 12.0]))
        recs = _random_records(rng, n, spread, with_big=bool(trial % 2))
        scene = tor.Scene.from_records(recs)
        inside = trial % 3 == 0
        look_from = tuple(rng.uniform(-0.5, 0.5, 3) * spread + (0, 0.2 * spread, 0)) if inside else (spread * 1.8, spread * 0.7, spread * 1.1)
        shutter = [(0.0, 1.0), (-1.0, 3.0), (0.5, 0.5), (2.0, 1.0)][trial % 4]
        ck = dict(look_from=look_from, look_at=(0.0, 0.1 * spread, 0.0), vertical_field_of_view=float(rng.uniform(20, 70)),
                  aperture=float(rng.uniform(0, 0.3)), focus_distance=float(rng.uniform(1, 2) * spread),
                  shutter_open=shutter[0], shutter_close=shutter[1])
        cam = tor.camera(**ck)
        h, w, spp = 20, 34, 6
        seeding = trial % 2
        base = _render(tor, scene, cam, h, w, spp, 12, seeding=seeding)
        for accel in ACCELS:
            acc = _render(tor, scene, cam, h, w, spp, 12, seeding=seeding, accel=accel)
            assert np.array_equal(acc.pixels, base.pixels), f"trial {trial} accel {accel}: changed {(acc.pixels != base.pixels).sum()} values"
        ocam = oracle.camera(look_from=ck["look_from"], look_at=ck["look_at"], vfov=ck["vertical_field_of_view"],
                             aperture=ck["aperture"], focus_dist=ck["focus_distance"], shutter_open=shutter[0],
                             shutter_close=shutter[1])
        assert np.array_equal(cam.as_array(), ocam)
        want = oracle.render(h, w, spp, ocam, recs, max_depth=12, seeding=seeding, math=1, arith=0, accum=seeding).pixels
        _assert_parity(base.pixels, want)


def test_full_c2_frame_matches_oracle(tor, oracle, ref_scene, ref_camera):
    """BASELINE configs[1] in full: 1920x1080, 100 spp, depth 50 with the reference's per-pixel streams
    (tor_render semantics, cost-ordered tiles) -- all 6 220 800 float64 channel values against the oracle
    (about a minute of CPU on the GPU box), plus the culled variant on the same frame."""
    import torch
    objs, _ = ref_scene
    scene, cam = tor.random_scene(0xFACADE), tor.camera()
    ctx = tor.Context()
    ctx.upload(scene.list())
    h, w, spp = 1080, 1920, 100
    want = oracle.render(h, w, spp, ref_camera, objs, seeding=0, math=1, arith=0).pixels
    for accel in (0, 1, 2, 3):
        buf = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        ctx.render_device(cam, h, w, spp, 2.2, 50, tor.make_options(seeding=tor.SEED_PIXEL, accel=accel), buf.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _assert_parity(buf.cpu().numpy(), want)
    ctx.close()


def test_bench_multi_rank_path_on_one_gpu(tor):
    """bench.py's N > 1 path (row-cyclic shards, per-rank render, all_gather of the shards, row assembly,
    max-over-ranks timing) with 2 ranks sharing this box's single GPU over gloo; --verify makes every rank
    compare the gathered frame with the frame it renders alone.  (The real run is one rank per GPU, RCCL.)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29600 + os.getpid() % 300
    env = dict(os.environ, TOR_BENCH_BACKEND="gloo", OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1",
                        "--warmup", "1", "--spp", "4", "--width", "640", "--height", "360", "--verify", "--full"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["gathered_frame_identical_to_single_process"] is True
    # strong scaling is the default: the frame -- and its spp -- do not depend on N
    assert d["scaling"] == "strong" and "640x360, 4 spp" in d["config"]["workload"] and d["value"] > 0
    # round 4: with --full the N > 1 line is self-contained -- CPU baseline (timed once the ranks are gone), kernel-level roofline
    # (slowest rank's HIP-event kernel time, live PMC traffic of one shard's launch), the gather's rank count, the N = 1 value of the same run
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["c1"]["ppm_equals_reference_png"] is True
    assert d["roofline"]["kernel_ms"] > 0 and len(d["roofline"]["kernel_ms_per_rank"]) == 2 and d["roofline"]["frac"] > 0
    assert "traffic" in d["roofline"] and "traffic_scope" in d["roofline"]
    assert d["rccl_ranks"] == 0 and d["gather"]["world"] == 2          # gloo on one GPU: no RCCL communicator in this run
    assert d["single_gpu_same_run"]["value"] > 0 and d["single_gpu_same_run"]["frame_identical_to_gathered"] is True
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port + 1), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1",
                        "--warmup", "0", "--spp", "4", "--width", "640", "--height", "360", "--scaling", "weak", "--no-stats", "--no-pmc"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["scaling"] == "weak" and "640x360, 8 spp" in d["config"]["workload"]


def test_f32_filter_extreme_scenes(tor):
    """TOR_ACCEL_F32 where float32 is weakest: the whole scene 5-8 thousand units away from the world origin
    (the filter works relative to its own origin), a scene three orders of magnitude smaller, and one so
    spread out that part of the objects fall outside the filter's range and stay on the float64 loop.
    Bit-identical canvases in every case."""
    rng = np.random.default_rng(77)
    for case in range(3):
        recs = _random_records(rng, 260, 6.0, with_big=case != 1)
        shift = np.zeros(3)
        scale = 1.0
        if case == 0:
            shift = np.array([5000.0, -3000.0, 8000.0])
        elif case == 1:
            scale = 1e-3
        else:
            far = rng.random(len(recs)) < 0.3           # a third of the objects 100x farther out
            recs[far, 1:4] *= 100.0
            recs[far, 4:7] *= 100.0
        recs[:, 1:4] = recs[:, 1:4] * scale + shift
        recs[:, 4:7] = recs[:, 4:7] * scale + shift
        recs[:, 9] *= scale
        scene = tor.Scene.from_records(recs)
        cam = tor.camera(look_from=tuple(np.array([11.0, 4.0, 7.0]) * scale + shift), look_at=tuple(np.array([0.0, 0.6, 0.0]) * scale + shift),
                         vertical_field_of_view=40.0, aperture=0.05 * scale, focus_distance=12.0 * scale)
        for seeding in (0, 1):
            base = _render(tor, scene, cam, 24, 40, 8, 12, seeding=seeding)
            for accel in (2, 3):
                acc = _render(tor, scene, cam, 24, 40, 8, 12, seeding=seeding, accel=accel)
                assert np.array_equal(acc.pixels, base.pixels), (case, seeding, accel, int((acc.pixels != base.pixels).sum()))
        assert base.pixels.std() > 0.01          # the frames are not trivially empty


def test_accel_fuzz_short(tor):
    """tools/fuzz_accel.py for 15 s: ~250 random scenes (40..1300 objects, 0.02..3000 units wide, up to 1e5 from
    the world origin, static / y-only / general movers in 1-4 time groups, hollow spheres, cameras inside the
    cloud, degenerate shutters), every accel mode against the float64 brute-force canvas, bit for bit.
    (Round 1 ran it for 7 minutes: 7831 scenes, 62 648 renders, 0 mismatches.)"""
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([_sys.executable, os.path.join(root, "tools", "fuzz_accel.py"), "15", "2026"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]
    assert b"0 mismatches" in r.stdout


def test_accel_fuzz_dense_oracle(tor):
    """tools/fuzz_accel.py on a fixed count of scenes, so that what it covers does not depend on the box: six `dense` scenes (1-3
    clusters of nearly coincident spheres, the worst case of the pooled lists and of every candidate queue), every one of them also
    rendered by the CPU oracle in both stream modes -- 12 oracle checks -- and every accel mode, both knob contexts, the wave-per-pixel
    kernel and the library's own choice of kernel against the brute force."""
    import re
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([_sys.executable, os.path.join(root, "tools", "fuzz_accel.py"), "--scenes", "6", "2026", "dense", "--oracle", "1"],
                       capture_output=True, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-2000:] + r.stderr.decode()[-2000:]
    assert "0 mismatches" in out and "heights: dense" in out
    m = re.search(r"(\d+) scenes, (\d+) renders, (\d+) of them checked against the CPU oracle", out)
    assert m and int(m.group(1)) == 6 and int(m.group(3)) == 12, out[-500:]


def test_default_accel_from_environment(tor, monkeypatch):
    """tor_render() keeps the reference's signature (no options); TOR_DEFAULT_ACCEL opts it into the exact
    accelerations.  Same canvas, and explicit options are never overridden."""
    scene, cam = tor.random_scene(0xFACADE), tor.camera()

    # (a frame above TOR_COOP_MAX_PIXELS, so that tor_render() really runs the accelerated LANE kernel: a small frame takes the
    # wave-per-pixel kernel, which has no accel variants, and the comparison would test nothing -- ADVICE r2)
    h, w, spp = 300, 400, 2

    def plain():
        cv = tor.new_canvas(h, w, spp, 2.2)
        tor.render(cv, cam, scene.list(), 50)            # options=None -> tor_render(), the reference's signature
        return cv.pixels.copy()
    monkeypatch.delenv("TOR_DEFAULT_ACCEL", raising=False)
    base = plain()                                        # unset: both exact accelerations (the drop-in's default)
    brute = tor.new_canvas(h, w, spp, 2.2)
    tor.render(brute, cam, scene.list(), 50, tor.make_options(accel=0, pixel_kernel=tor.PIXEL_KERNEL_LANE))
    assert np.array_equal(base, brute.pixels)
    for v in ("0", "3", "2", "1"):
        monkeypatch.setenv("TOR_DEFAULT_ACCEL", v)
        assert np.array_equal(plain(), base), v
    for v in ("17", "x", ""):                             # a malformed value is an error, not a silent default
        monkeypatch.setenv("TOR_DEFAULT_ACCEL", v)
        with pytest.raises(tor.TorError) as e:
            plain()
        assert e.value.code == -1 and "TOR_DEFAULT_ACCEL" in str(e.value)
