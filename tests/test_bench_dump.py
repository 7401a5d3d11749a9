"""bench.py --dump-outputs: what the timed path computed in its last step, as DIR/<name>.npy in float64, at most 64 MB in all
(a larger frame: a fixed, seeded sample of its pixels), and --steps is the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_output_is_written_whole(tmp_path):
    a = np.arange(64 * 96 * 3, dtype=np.float64).reshape(64, 96, 3)
    bench.dump_outputs(str(tmp_path / "d"), {"frame": a})
    got = np.load(str(tmp_path / "d" / "frame.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, a)


def test_large_output_is_a_fixed_sample_within_the_budget(tmp_path):
    # 3840x2160 (BASELINE configs[3]): 199 MB of float64 -- more than the budget
    a = np.random.default_rng(1).random((2160, 3840, 3))
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"frame": a})
    paths = [str(tmp_path / d / "frame.npy") for d in ("x", "y")]
    assert all(os.path.getsize(p) <= 64 * 1000 * 1000 for p in paths)
    x, y = (np.load(p) for p in paths)
    assert x.dtype == np.float64 and x.shape[1] == 3 and x.shape[0] * 3 * 8 > 60 * 1000 * 1000
    assert np.array_equal(x, y)                                    # the same pixels in every run
    px = a.reshape(-1, 3)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(px.shape[0], x.shape[0], replace=False))
    assert np.array_equal(x, px[idx])                              # the pixels the documented seed picks


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--workload", "c5", "--frames", "3", "--steps", "2"]])
def test_bad_step_counts_are_refused(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr, (r.returncode, r.stderr[-500:])


@pytest.mark.gpu
def test_bench_dumps_the_frame_of_its_last_timed_step(tor, tmp_path):
    """The dumped frame is the frame the timed path renders (same scene, camera and options, rendered here directly), and the
    line reports the requested number of steps."""
    import torch
    out = str(tmp_path / "dump")
    h, w, spp = 108, 192, 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--width", str(w), "--height", str(h), "--spp", str(spp), "--no-cpu-baseline", "--no-pmc", "--no-stats",
                        "--no-host-leg", "--no-accel-leg", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 2
    got = np.load(os.path.join(out, "frame.npy"))
    ctx = tor.Context()
    ctx.upload(tor.random_scene(0xFACADE).list())
    want = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    ctx.render_device(tor.camera(), h, w, spp, 2.2, 50, tor.make_options(seeding=tor.SEED_SAMPLE, arith=tor.ARITH_STRICT),
                      want.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.close()
    assert got.dtype == np.float64 and got.shape == (h, w, 3)
    assert np.array_equal(got, want.cpu().numpy())
