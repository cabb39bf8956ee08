"""bench.py's plain run and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_large_arrays(tmp_path):
    import bench
    cap = bench.DUMP_ARRAY_BYTES // 4
    big = torch.arange(cap + 1000, dtype=torch.float64)
    arrays = {"small": torch.tensor([1.5, -2.0]), "big": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.dtype == np.float32 and small.tolist() == [1.5, -2.0]
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (cap,)
    assert np.array_equal(a, b)                       # the same fixed sample every run
    assert np.all(np.diff(a) > 0)                     # distinct elements, in index order


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "2", "--frames", "4", "--size", "64", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "clips/s"
    assert "cpu_baseline" not in d and "roofline" not in d and "value_exact_fp32" not in d   # --full only
    files = {f: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(files) == {"loss.npy", "logits.npy", "params.npy", "grad.npy"}
    assert all(a.dtype == np.float32 and np.all(np.isfinite(a)) for a in files.values())
    assert files["logits.npy"].shape == (2, 400, 1)
    assert files["params.npy"].shape == files["grad.npy"].shape == (3794322,)     # flat X3D-M parameters
    assert np.abs(files["loss.npy"] - d["config"]["loss"]).max() < 1e-3
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
