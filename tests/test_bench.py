"""bench.py's own contract: a plain run reports the headline over exactly --steps timed callbacks and nothing that needs
passes of its own (those are --full), and --dump-outputs writes what the last timed callback handed its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_cuts_large_arrays_to_a_fixed_sample(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 4096)
    mix = np.ones((1, 512, 2), np.float64)  # exactly its 4096-byte share once in float32: kept whole
    peaks = np.arange(2000 * 2, dtype=np.float32).reshape(2000, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"mix": mix, "peaks": peaks})
    got = np.load(tmp_path / "a" / "peaks.npy")
    assert got.dtype == np.float32 and got.shape == (512, 2)
    assert np.all(got[:, 1] == got[:, 0] + 1) and np.all(np.diff(got[:, 0]) > 0)  # whole rows of the input, in order
    np.testing.assert_array_equal(got, np.load(tmp_path / "b" / "peaks.npy"))  # the same rows every time
    m = np.load(tmp_path / "a" / "mix.npy")
    assert m.dtype == np.float32 and m.shape == (1, 512, 2) and np.all(m == 1)


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--sources-per-gpu", "1024", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_callback(gas, tmp_path):
    """7 steps: not a whole number of 10-callback batches, so the dump reads a callback completed by the closing join.
    The ordered mode runs the same callbacks on the same inputs one launch pair at a time: its last mix and
    its draining sources' peaks are the same."""
    line = _bench(tmp_path / "head")
    assert line["steps"] == 7 and line["warmup"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["metric"] == "mixed AudioFrames/s" and line["unit"] == "AudioFrames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert "roofline" not in line and "cpu_baseline" not in line and "ordered" not in line
    mix, peaks = np.load(tmp_path / "head" / "mix.npy"), np.load(tmp_path / "head" / "peaks.npy")
    # GAS_FLAG_PEAKS_DRAINING_ONLY: the peaks the caller reads are the draining sources' (1 in 64); the others are +inf
    # ("not measured") in the library's buffer and stay out of the dump
    assert mix.dtype == peaks.dtype == np.float32 and mix.shape == (1, 512, 2) and peaks.shape == (1024 // 64, 2)
    assert np.all(np.isfinite(mix)) and np.all(np.isfinite(peaks)) and np.abs(mix).max() > 0 and peaks.min() > 0
    _bench(tmp_path / "ordered", "--no-pipelined-mix")
    assert rel_rms(mix, np.load(tmp_path / "ordered" / "mix.npy")) <= 1e-5
    np.testing.assert_allclose(peaks, np.load(tmp_path / "ordered" / "peaks.npy"), rtol=2e-5, atol=1e-7)
    exact = _bench(tmp_path / "exact", "--exact-peaks")  # every source's peak is measured: every row is dumped
    assert exact["steps"] == 7
    pe = np.load(tmp_path / "exact" / "peaks.npy")
    assert pe.shape == (1024, 2) and np.all(np.isfinite(pe))
    np.testing.assert_allclose(pe[::64], peaks, rtol=2e-5, atol=1e-7)
