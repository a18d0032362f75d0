"""bench.py's plain / --full split and --dump-outputs: the dump helper on CPU tensors (whole vector, seeded sample)
and, on the GPU, a tiny cavity run through the command line: the plain line carries the headline keys only,
--full adds the measurements that take runs of their own, and two runs dump identical arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATS = dict(newton_iterations=1, linear_iterations=7, residual_evaluations=2, final_residual=1.5e-4, linear_failures=0)
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("kernel_ms", "roofline")


def test_dump_outputs_whole_vector_and_seeded_sample(tmp_path, monkeypatch):
    import torch

    import bench
    x = torch.arange(1000, dtype=torch.float64) * 0.5
    bench.dump_outputs(str(tmp_path / "a"), x, STATS)
    got = np.load(tmp_path / "a" / "present.npy")
    assert got.dtype == np.float64 and np.array_equal(got, x.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "newton_stats.npy"), [1.0, 7.0, 2.0, 1.5e-4, 0.0])
    # above the size cap: the same ascending sample of entries on every call, within the cap
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 64)
    bench.dump_outputs(str(tmp_path / "b"), x, STATS)
    bench.dump_outputs(str(tmp_path / "c"), x, STATS)
    b, c = np.load(tmp_path / "b" / "present.npy"), np.load(tmp_path / "c" / "present.npy")
    assert b.shape == (64,) and np.array_equal(b, c)
    assert np.all(np.diff(b) >= 0) and len(np.unique(b)) > 32 and np.all(np.isin(b, x.numpy()))
    # N ranks: a file per rank, the cap shared between them
    bench.dump_outputs(str(tmp_path / "d"), x, STATS, rank=1, world=2)
    assert np.load(tmp_path / "d" / "present_rank1.npy").shape == (32,)
    assert sorted(os.listdir(tmp_path / "d")) == ["newton_stats_rank1.npy", "present_rank1.npy"]


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--cells", "8"] + list(extra), capture_output=True, text=True, timeout=170)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_reproducible_outputs(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    b = _bench("--dump-outputs", str(tmp_path / "b"))
    for key in HEADLINE:
        assert key in a, key
    assert a["steps"] == 2 and a["warmup"] == 1 and a["full"] is False and a["dtype"] == "f64"
    assert a["ms_per_step"] > 0 and abs(a["value"] * a["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert not [key for key in FULL_ONLY + ("cpu_baseline",) if key in a]
    assert sorted(os.listdir(tmp_path / "a")) == ["newton_stats.npy", "present.npy"]
    xa, xb = np.load(tmp_path / "a" / "present.npy"), np.load(tmp_path / "b" / "present.npy")
    assert xa.dtype == np.float64 and xa.shape == (a["config"]["n_dofs"],) and np.isfinite(xa).all()
    assert np.abs(xa).max() > 0.1  # the lid's unit velocity is in the iterate
    # identical inputs: the runs can differ by the rounding of reordered FP64 sums at most (1e-16, amplified by the
    # solve far below 1e-9); at this size and at 128^3 they were measured bitwise equal
    diff = np.abs(xa - xb).max()
    print("run-to-run max |difference| of the dumped iterate: %.3e" % diff)
    assert diff <= 1e-9 * np.abs(xa).max()
    sa = np.load(tmp_path / "a" / "newton_stats.npy")
    assert sa[0] == 1 and sa[1] == a["linear_iterations_per_step"] and sa[4] == 0
    assert np.array_equal(sa, np.load(tmp_path / "b" / "newton_stats.npy"))


@pytest.mark.gpu
def test_full_run_adds_the_kernel_breakdown_and_roofline():
    d = _bench("--full", "--no-cpu")
    for key in HEADLINE + FULL_ONLY:
        assert key in d, key
    assert d["full"] is True and d["kernel_ms"]["instrumented_step_ms"] > 0 and d["roofline"]["launch_ms"] > 0
