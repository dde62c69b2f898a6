"""The driver launches bench.py via torch.distributed.run for N>1 — exercise
that exact path on CPU (gloo, tiny preset) so the unattended multi-GPU run
has no untested plumbing."""

import json
import os
import socket
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_bench(nproc: int):
    cmd = [
        sys.executable, "-m", "torch.distributed.run",
        "--nnodes=1", f"--nproc-per-node={nproc}",
        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
        os.path.join(REPO, "bench.py"),
        "--gpus", str(nproc), "--steps", "2", "--warmup", "1",
        "--height", "128", "--width", "128", "--preset", "tiny",
        # gloo on the CPU also where GPUs are present: there may be fewer
        # GPUs than ranks, and this test is about the launch plumbing
        "--cpu",
    ]
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_bench_single_process():
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
           "--steps", "2", "--warmup", "1", "--height", "128", "--width", "128",
           "--preset", "tiny"]
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["metric"].startswith("end-to-end latency")
    assert rec["n_gpus"] == 1
    assert rec["value"] > 0
    assert rec["higher_is_better"] is False


def _run_single(*extra: str) -> dict:
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
           "--steps", "3", "--warmup", "1", "--height", "128", "--width", "128",
           "--preset", "tiny", *extra]
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's latents as float32 .npy,
    and the same arguments give the same arrays from run to run."""
    import numpy as np

    # on the CPU in fp32 the step itself is deterministic, so identical
    # inputs must give bit-identical outputs
    recs = [_run_single("--cpu", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    a = np.load(tmp_path / "a" / "latents.npy")
    b = np.load(tmp_path / "b" / "latents.npy")
    assert a.dtype == np.float32 and a.shape == (1, 4, 16, 16)
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)
    for rec in recs:
        assert rec["steps"] == 3
        assert rec["ms_per_step"] > 0
        assert abs(rec["value"] - rec["ms_per_step"] * 50 / 1000.0) < 1e-9


def test_bench_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """An output over the size limit is cut to a fixed sample that fits it."""
    import numpy as np
    import torch

    sys.path.insert(0, REPO)
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8192)
    x = torch.arange(5000, dtype=torch.bfloat16).reshape(50, 100)
    bench.dump_outputs(str(tmp_path / "a"), {"x": x, "small": x[:2]})
    bench.dump_outputs(str(tmp_path / "b"), {"x": x, "small": x[:2]})
    a = np.load(tmp_path / "a" / "x.npy")
    assert a.dtype == np.float32 and a.size < x.numel()
    assert np.array_equal(a, np.load(tmp_path / "b" / "x.npy"))
    assert np.isin(a, x.float().numpy()).all()
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), x[:2].float().numpy())
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 8192


def test_bench_full_flag_keeps_result_line():
    rec = _run_single("--full")
    assert rec["metric"].startswith("end-to-end latency")
    assert rec["unit"] == "s/image" and rec["higher_is_better"] is False
    assert rec["dtype"] in ("fp32", "bf16") and rec["ms_per_step"] > 0


def test_bench_torchrun_two_ranks():
    rec = _run_bench(2)
    assert rec["n_gpus"] == 2
    assert rec["config"]["parallelism"] == "cfg2x1patch"
    assert rec["value"] > 0
