"""bench.py's output dump (--dump-outputs) and the split between a plain run and --full.  The dump lets two builds be
compared output for output, so the same arguments must give the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_large_arrays_at_fixed_positions(tmp_path):
    import bench
    big = torch.randn(3000, 1000, generator=torch.Generator().manual_seed(1))
    small = torch.randn(4, 5, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "a"), {"big": big, "small": small, "f64": torch.zeros(3, dtype=torch.float64)})
    bench.dump_outputs(str(tmp_path / "b"), {"big": big.clone()})
    a = np.load(tmp_path / "a" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(a, np.load(tmp_path / "b" / "big.npy"))
    assert np.isin(a, big.numpy()).all()
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.float().numpy())
    assert np.load(tmp_path / "a" / "f64.npy").dtype == np.float64


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    import bench
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "d"), {"a%d" % i: torch.zeros(bench.DUMP_SAMPLE) for i in range(17)})
    assert not (tmp_path / "d").exists()


def _bench(args, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_last_step_whatever_the_prewarm(tmp_path):
    """The clock pre-warm runs for a time, not a number of steps; the dump of the last timed step must not depend on it."""
    args = ["--batch", "8", "--steps", "3", "--warmup", "2"]
    lines = [_bench(args + ["--dump-outputs", str(tmp_path / "a")], EA_BENCH_PREWARM_MS="0"),
             _bench(args + ["--dump-outputs", str(tmp_path / "b")])]
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert not {"cpu_baseline", "other_workloads", "roofline", "eager_ms_per_step"} & set(line)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"y.npy", "dx.npy", "grad.qkv.weight.npy", "param.qkv.weight.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n


@pytest.mark.gpu
def test_full_run_adds_the_extra_measurements():
    line = _bench(["--batch", "8", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-other-workloads"])
    assert line["eager_ms_per_step"] > 0 and line["ms_per_step_blocks"]["n"] == 5
    assert line["roofline"]["all_kernels_avg_us"] and line["hbm_measured_copy_gbs"] > 0
