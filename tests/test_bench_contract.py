"""bench.py driver-contract tests: JSON schema, single-process run, and
the exact torchrun multi-rank launch path the driver uses (gloo on CPU)."""

import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


def _last_json_line(stdout: str) -> dict:
    for line in reversed(stdout.strip().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{stdout}")


def test_bench_single_process_contract():
    proc = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1",
         "--batch", "512"],
        capture_output=True, text=True, timeout=300, cwd=str(REPO),
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    out = _last_json_line(proc.stdout)
    assert REQUIRED_KEYS <= set(out.keys()), out.keys()
    assert out["value"] > 0
    assert out["higher_is_better"] is True
    assert out["scaling"] == "weak"
    assert out["data"] == "synthetic"
    assert out["steps"] == 3 and out["warmup"] == 1
    assert {"model", "global_batch", "seq_len", "parallelism"} <= set(
        out["config"].keys()
    )


def test_bench_dump_outputs_repeatable_and_full(tmp_path):
    """--dump-outputs writes the last timed step's deliveries as float
    .npy files, identical from run to run; a plain run skips the latency
    phase, --full reports it without changing what the steps compute."""
    import numpy as np

    def run(out_dir, *extra):
        proc = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "3",
             "--warmup", "1", "--batch", "512", "--agents", "64",
             "--dump-outputs", str(out_dir), *extra],
            capture_output=True, text=True, timeout=300, cwd=str(REPO),
        )
        assert proc.returncode == 0, proc.stdout + proc.stderr
        return _last_json_line(proc.stdout)

    plain = run(tmp_path / "a")
    full = run(tmp_path / "b", "--full")
    latency_keys = {"p50_latency_ms", "p99_latency_ms", "n_latency_samples"}
    assert not latency_keys & set(plain.keys())
    assert latency_keys <= set(full.keys())
    assert full["n_latency_samples"] > 0 and full["p50_latency_ms"] > 0
    assert plain["steps"] == full["steps"] == 3
    assert plain["ms_per_step"] > 0

    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["counts.npy", "headers.npy", "payloads.npy",
                     "sample_index.npy", "seq_offsets.npy"]
    total = 0
    for name in names:
        a = np.load(tmp_path / "a" / name)
        b = np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        assert a.shape == b.shape and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    counts = np.load(tmp_path / "a" / "counts.npy")
    offs = np.load(tmp_path / "a" / "seq_offsets.npy")
    pays = np.load(tmp_path / "a" / "payloads.npy")
    # one tick delivers exactly the 512 messages it enqueued
    assert counts.shape == (64,) and counts.sum() == 512 == len(offs)
    assert sorted(offs.tolist()) == list(range(512))
    assert pays.shape == (512, 1024)
    assert pays.min() >= 32 and pays.max() < 127  # printable synthetic bytes


def test_bench_torchrun_world2():
    """The driver's exact launch shape: torch.distributed.run, nnodes=1,
    nproc-per-node 2, master-addr 127.0.0.1 (gloo fallback on CPU)."""
    env = dict(os.environ)
    env.setdefault("GLOO_SOCKET_IFNAME", "lo")
    proc = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node", "2",
            "--master-addr", "127.0.0.1", "--master-port", "29517",
            "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
            "--batch", "256", "--agents", "64",
        ],
        capture_output=True, text=True, timeout=300, env=env, cwd=str(REPO),
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    out = _last_json_line(proc.stdout)
    assert out["config"]["agents"] == 128  # 64 per rank, weak scaling
    assert out["config"]["global_batch"] == 512
    assert "all-to-all" in out["config"]["parallelism"]
    assert out["value"] > 0


def test_bench_broadcast_mode():
    proc = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1",
         "--batch", "256", "--agents", "64", "--bcast-frac", "0.05"],
        capture_output=True, text=True, timeout=300, cwd=str(REPO),
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    out = _last_json_line(proc.stdout)
    assert out["value"] > 0
    # fan-out amplifies deliveries; no loss warning expected
    assert "loss" not in proc.stderr
