"""bench.py's entry point on the CPU (no GPU call is reached): `--gpus` is authoritative.

- Under a launcher (WORLD_SIZE set) every rank exits non-zero unless WORLD_SIZE == --gpus, so a mislabelled line
  cannot be printed.
- A bare `bench.py --gpus N` (N > 1, no WORLD_SIZE) is the launcher: it starts torch.distributed.run as a child.
  Here (no GPU) the RCCL form stops before that with a clear error naming the visible-GPU count; the GPU test
  `tests/test_gpu_dp.py::test_bench_py_bare_gpus2_spawns_ranks` runs the spawned ranks.
- One GPU test: a plain run carries none of the `--full` legs and `--dump-outputs` writes the last step's arrays.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(kw)
    return env


@pytest.mark.parametrize("world,gpus", [("2", "1"), ("1", "2"), ("4", "8")])
def test_world_size_must_equal_gpus(world, gpus):
    p = subprocess.run([sys.executable, BENCH, "--gpus", gpus, "--steps", "1"], env=_env(WORLD_SIZE=world),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert f"WORLD_SIZE={world} but --gpus {gpus}" in p.stderr
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_bare_gpus_n_is_the_launcher_and_checks_devices():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--steps", "1"], env=_env(VQA_DIST_BACKEND="nccl"),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert "--gpus 8 needs 8 visible GPUs for RCCL" in p.stderr


def test_gpus_must_be_positive():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "0"], env=_env(), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 2 and "--gpus must be >= 1" in p.stderr


def _plain_run(out_dir, *extra):
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--seq", "8192",
           "--dump-outputs", str(out_dir), *extra]
    p = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(cuda, tmp_path):
    """A plain run prints the headline line with none of the --full legs, and --dump-outputs writes what the last
    timed train_step left its caller: the returned metrics, the weights, the gradient, the codebooks (fp32 / fp64,
    far below 64 MB). The batches and the initial weights are seeded: a second run gives the same arrays."""
    out, got = _plain_run(tmp_path / "a")
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["dtype"] == "bf16" and out["higher_is_better"] is True
    want = 2 * 8192 / (out["ms_per_step"] * 1e-3)
    assert abs(out["value"] - want) <= 1e-3 * want
    for k in ("roofline", "cpu_baseline", "config2_fp32", "config4_prior_train", "config5_upsampler_decode"):
        assert k not in out, k
    assert sorted(got) == ["codebook_0", "codebook_1", "codebook_2", "grads", "metrics", "weights"]
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) < 64 << 20
    assert got["metrics"].shape == (4 + 7 * 3,) and round(float(got["metrics"][0]), 5) == out["config"]["final_loss"]
    assert got["weights"].shape == got["grads"].shape and np.abs(got["grads"]).max() > 0
    assert all(got[f"codebook_{l}"].shape == (64, 2048) for l in range(3))
    _, again = _plain_run(tmp_path / "b")
    for k in got:
        assert np.array_equal(got[k], again[k]), f"{k} differs between two runs with the same arguments"


def test_launcher_command_shape(monkeypatch):
    """The child command: torch.distributed.run, one node, N processes per node, rendezvous on 127.0.0.1, this
    bench.py with the caller's own arguments; started with subprocess.call (a child, never an exec)."""
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", [BENCH, "--gpus", "4", "--steps", "5"])
    monkeypatch.setenv("VQA_DIST_BACKEND", "gloo")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.main() == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    i = cmd.index("--nproc-per-node")
    assert cmd[i + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--nnodes") + 1] == "1"
    assert os.path.abspath(cmd[cmd.index("--master-port") + 2]) == os.path.abspath(BENCH)
    assert cmd[-4:] == ["--gpus", "4", "--steps", "5"]
    assert seen["env"]["MASTER_ADDR"] == "127.0.0.1"
