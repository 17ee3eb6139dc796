"""bench.py's command line: a plain run is the timed steps and the result line only (every other leg sits behind --full), and
--dump-outputs writes what the last timed step computed, the same arrays from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline_mfma", "op_us_per_slide", "sustained", "allreduce", "prepared_pipelined", "prepared_resident", "batched", "ingest",
             "per_slide", "dropin", "cpu_baseline", "speedup_vs_cpu")


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_write_outputs_float32_and_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 4096 + 2 * 40_000)     # 40,000 bytes per array
    big = torch.arange(50_000, dtype=torch.float32).reshape(500, 100)
    small = torch.tensor([1, 2, 3], dtype=torch.int64)
    bench.write_outputs(str(tmp_path / "a"), {"big": big, "small": small})
    bench.write_outputs(str(tmp_path / "b"), {"big": big, "small": small})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.tolist() == [1.0, 2.0, 3.0]
    b1, b2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert b1.dtype == np.float32 and b1.nbytes <= 40_000 and b1.size == 10_000
    assert np.array_equal(b1, b2)                                            # same elements every run
    assert np.all(np.diff(b1) > 0) and np.all(np.isin(b1, big.numpy()))      # distinct elements of the array, in order
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BUDGET_BYTES


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_is_lean_and_dumps_reproducible_outputs(cuda, tmp_path):
    def run(tag):
        out_dir = tmp_path / tag
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--patches", "8192", "--steps", "3", "--warmup", "1",
               "--dump-outputs", str(out_dir)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0]), out_dir

    line, d1 = run("a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "slides/s" and line["higher_is_better"] is True
    assert line["value"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    assert not [k for k in FULL_ONLY if k in line], [k for k in FULL_ONLY if k in line]
    _, d2 = run("b")
    names = sorted(os.listdir(d1))
    assert names == ["grad.npy", "loss.npy", "params.npy"] and sorted(os.listdir(d2)) == names
    for f in names:
        a, b = np.load(d1 / f), np.load(d2 / f)
        assert a.dtype == np.float32 and a.shape == b.shape and np.all(np.isfinite(a)), f
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7, err_msg=f)
    loss = np.load(d1 / "loss.npy")
    assert loss.shape == (1, 3) and abs(float(loss[0, 0]) - line["last_loss"]) <= 1e-4
    assert np.load(d1 / "params.npy").size == np.load(d1 / "grad.npy").size > 1_000_000
