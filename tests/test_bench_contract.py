"""The driver depends on bench.py's CLI + JSON contract; pin it."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


def _run_bench(extra, env_extra=None):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO
    env.update(env_extra or {})
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py")] + extra,
        capture_output=True, text=True, timeout=600, env=env, cwd=REPO,
    )
    assert r.returncode == 0, r.stderr
    line = r.stdout.strip().splitlines()[-1]
    return json.loads(line)


def test_bench_json_contract_cpu():
    out = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1",
                      "--batch-size", "2", "--model", "resnet18",
                      "--dtype", "fp32", "--memory-format", "contiguous"])
    assert REQUIRED_KEYS.issubset(out.keys()), REQUIRED_KEYS - out.keys()
    assert out["n_gpus"] == 1
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["higher_is_better"] is True
    assert out["scaling"] == "weak"
    assert out["data"] == "synthetic"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["global_batch"] == 2
    assert out["config"]["parallelism"] == "dp1"


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs writes the last timed step's results as float .npy
    files, the same from run to run.  A dumping run puts the seeded initial
    state back before its last timed step, so the files do not depend on
    how many steps came before it: 1 warmup + 2 steps dumps exactly what a
    single first step dumps.  --full is accepted and leaves the result
    line's meaning alone."""
    import numpy as np

    cfg = ["--gpus", "1", "--batch-size", "2", "--model", "resnet18",
           "--dtype", "fp32", "--memory-format", "contiguous"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    # Bit-equality needs a deterministic run: hide any GPU (its conv
    # backward-weights kernels sum in a varying order), one CPU thread.
    one = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1",
           "OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1"}
    out = _run_bench(cfg + ["--steps", "2", "--warmup", "1",
                            "--dump-outputs", a], one)
    full = _run_bench(cfg + ["--steps", "1", "--warmup", "0", "--full",
                             "--dump-outputs", b], one)
    assert REQUIRED_KEYS.issubset(full.keys())
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert full[k] == out[k]
    assert out["steps"] == 2 and full["steps"] == 1
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"loss.npy", "logits.npy", "bn1_weight.npy",
            "fc_weight.npy"}.issubset(names)
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64)
        assert np.isfinite(x).all()
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(a, "logits.npy")).shape == (2, 1000)
    assert np.load(os.path.join(a, "loss.npy")).shape == (1,)
    # the dumped step did update the model: affine BN weight starts at 1
    assert not np.all(np.load(os.path.join(a, "bn1_weight.npy")) == 1.0)


def test_bench_distributed_launch_cpu():
    """torchrun-launched bench on CPU/gloo world 2 (the driver's launch
    shape), value aggregated over ranks."""
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29531", "--no-python", sys.executable,
         os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--batch-size", "2", "--model", "resnet18",
         "--dtype", "fp32", "--memory-format", "contiguous"],
        capture_output=True, text=True, timeout=600, env=env, cwd=REPO,
    )
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2"
    assert out["config"]["global_batch"] == 4


def test_bench_multirank_cpu_gloo(tmp_path):
    """bench.py end-to-end under torch.distributed.run with 2 CPU/gloo ranks
    (VERDICT r01 next-round #1 done-criterion): the distributed branch —
    msbn DDP wrap, barriers, MAX-over-ranks timing, single JSON line."""
    import json
    import subprocess
    import sys

    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port), os.path.join(REPO, "bench.py"),
         "--gpus", "2", "--steps", "1", "--warmup", "0",
         "--batch-size", "2", "--model", "resnet18", "--dtype", "fp32",
         "--memory-format", "contiguous"],
        capture_output=True, text=True, timeout=600, cwd=REPO, env=env,
    )
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 4
    assert d["value"] > 0
