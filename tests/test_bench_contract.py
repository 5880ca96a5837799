"""Driver contract: bench.py must emit ONE valid JSON line, including
under torch.distributed.run with N ranks (the driver's scale runs)."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

BENCH = Path(__file__).resolve().parent.parent / "bench.py"


@pytest.mark.timeout(300)
def test_bench_single_rank_cpu():
    r = subprocess.run(
        [sys.executable, "bench.py", "--device", "cpu", "--model", "tiny",
         "--steps", "2", "--warmup", "1", "--concurrency", "2",
         "--isl", "8", "--osl", "4", "--max-model-len", "64"],
        capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == 1 and j["value"] > 0
    for key in ("metric", "unit", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in j


@pytest.mark.timeout(300)
def test_bench_dump_outputs_repeatable_cpu(tmp_path):
    """--dump-outputs writes the timed steps' StepOutputs as float arrays,
    identical from run to run; --full is accepted and changes nothing the
    plain result line reports."""
    import numpy as np

    def run(out_dir, *extra):
        r = subprocess.run(
            [sys.executable, str(BENCH), "--device", "cpu", "--model", "tiny",
             "--steps", "5", "--warmup", "1", "--concurrency", "2",
             "--isl", "8", "--osl", "4", "--max-model-len", "64",
             "--dump-outputs", str(out_dir), *extra],
            capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads([ln for ln in r.stdout.splitlines()
                        if ln.startswith("{")][-1])
        return j, {p.name: np.load(p) for p in sorted(out_dir.glob("*.npy"))}

    ja, a = run(tmp_path / "a")
    jb, b = run(tmp_path / "b", "--full")
    assert set(a) == {"last_step_request_index.npy", "last_step_token_ids.npy",
                      "last_step_finished.npy", "timed_steps.npy"}
    assert set(a) == set(b)
    for name in a:
        assert a[name].dtype == np.float64
        np.testing.assert_array_equal(a[name], b[name])
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    steps = a["timed_steps.npy"]
    assert steps.shape[0] == ja["steps"] == 5 and steps.shape[2] == 3
    # every emitted token is recorded: matches the result line's count
    assert int((steps[:, :, 1] >= 0).sum()) == ja["config"]["timed_output_tokens"]
    n_last = len(a["last_step_token_ids.npy"])
    np.testing.assert_array_equal(steps[-1, :n_last, 1],
                                  a["last_step_token_ids.npy"])
    assert (steps[-1, n_last:] == -1).all()
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert ja[key] == jb[key]
    assert ja["ms_per_step"] > 0 and jb["ms_per_step"] > 0


@pytest.mark.timeout(600)
def test_bench_two_ranks_gloo():
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29517", "bench.py", "--gpus", "2",
         "--device", "cpu", "--model", "tiny", "--steps", "2",
         "--warmup", "1", "--concurrency", "2", "--isl", "8", "--osl", "4",
         "--max-model-len", "64"],
        capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, f"exactly rank0 prints: {lines}"
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2
    assert j["config"]["parallelism"] == "dp2"
