"""bench.py: a plain run measures the headline figure only (set-up, warm-up, the timed steps, the line); --full adds the secondary
legs -- CPU baseline, workload and live counters, host-canvas region, acceleration and pixel-seeding legs -- as before."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SECONDARY = ("host_canvas", "value_survey_8d", "unscreened", "second_form_only", "accel_f32", "accel_blocks", "accel_blocks_f32",
             "pixel_seeding", "pixel_seeding_default_accel")


def _args(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse_args()


def test_full_is_off_by_default(monkeypatch):
    a = _args(["--gpus", "1", "--steps", "3", "--warmup", "1"], monkeypatch)
    assert a.full is False and (a.steps, a.warmup) == (3, 1)
    assert bench.skipped(a, "--no-pmc") == bench.PLAIN_NOTE
    a = _args(["--full"], monkeypatch)
    assert a.full is True and a.steps == 5
    assert bench.skipped(a, "--no-pmc") == "skipped (--no-pmc)"


def _run(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--width", "192", "--height", "108", "--spp", "4"] + argv, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_legs(tmp_path):
    plain = _run(["--dump-outputs", str(tmp_path / "plain")])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 2 and plain["dtype"] == "f64"
    assert not any(k in plain for k in SECONDARY), [k for k in SECONDARY if k in plain]
    assert plain["cpu_baseline"] == {"value": None, "note": bench.PLAIN_NOTE}
    assert plain["roofline"]["workload_live"] is None and plain["roofline"]["traffic_detail"] == bench.PLAIN_NOTE
    assert plain["roofline"]["kernel_ms"] > 0 and plain["roofline"]["launches_averaged"] == 2

    full = _run(["--full", "--no-pmc", "--cpu-seconds", "1", "--aux-steps", "1", "--dump-outputs", str(tmp_path / "full")])
    assert [full[k] for k in ("metric", "unit", "higher_is_better", "dtype")] == [plain[k] for k in ("metric", "unit", "higher_is_better", "dtype")]
    assert all(k in full for k in SECONDARY), [k for k in SECONDARY if k not in full]
    assert full["host_canvas"]["canvas_identical_to_resident_frame"] is True
    assert all(full["accel_" + n]["canvas_identical_to_brute_force"] is True for n in ("f32", "blocks", "blocks_f32"))
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["c1"]["ppm_equals_reference_png"] is True
    assert full["roofline"]["workload_live"]["samples"] == 108 * 192 * 4
    assert full["roofline"]["traffic_detail"] == "skipped (--no-pmc)"
    # the timed path is the same either way: the same frame from its last step
    a, b = (np.load(str(tmp_path / d / "frame.npy")) for d in ("plain", "full"))
    assert np.array_equal(a, b)
