"""bench.py as the driver runs it: one JSON line on stdout that fits the driver's capture, and `--gpus N` starting its own
ranks when no launcher is around it (round-4 review items 1 and 3); a plain run is the headline alone and --dump-outputs
writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
SHORT = ["--steps", "3", "--warmup", "2", "--full", "--no-presets", "--no-epoch", "--no-cpu-baseline"]


def _env(**kw):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **kw)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "RR_F16X2"):
        env.pop(k, None)
    return env


def _run(args, env):
    p = subprocess.run([sys.executable, BENCH] + args, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                            # ONE line on stdout, nothing else
    assert len(lines[0].encode()) < 6144, len(lines[0])
    return json.loads(lines[0]), p.stderr


def test_one_gpu_line_is_short_complete_and_on_the_exact_arithmetic():
    line, err = _run(["--gpus", "1"] + SHORT, _env())
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype",
              "data", "config", "roofline", "roofline_gather"):
        assert line.get(k) is not None, k
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["dtype"] == "f32" and "three EXACT bf16" in line["gemm_arithmetic"]
    r = line["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["products_per_multiply"] == 6 and "linear_split_kernel" in r["kernel"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["avg_launch_us"] > 0
    assert line["f16x2_path"]["dtype"] != "f32" and line["f16x2_path"]["queries_per_s"] > 0     # the narrower form is labelled as such
    assert line["f32_mfma_path"]["queries_per_s"] > 0
    assert abs(line["value"] - 64 * 1e3 / line["ms_per_step"]) < 0.01 * line["value"]
    with open(os.path.join(REPO, line["detail"])) as f:
        detail = json.load(f)
    assert "kernels" in detail and "kernels_isolated" in detail and "detail kernels" in err


def test_plain_run_is_the_headline_alone_and_dumps_its_last_step(tmp_path):
    """Without --full: no comparison leg, no detail file, the contract's keys meaning what they do with --full.
    --dump-outputs: the last timed step's scores, loss, parameters and gradients; the same arguments give the same arrays."""
    args = ["--gpus", "1", "--steps", "3", "--warmup", "2"]
    line, _ = _run(args + ["--dump-outputs", str(tmp_path / "a")], _env())
    for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "dtype"):
        assert line.get(k) is not None, k
    assert line["steps"] == 3 and line["warmup"] == 2 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert abs(line["value"] - 64 * 1e3 / line["ms_per_step"]) < 0.01 * line["value"]
    for k in ("roofline", "roofline_gather", "cpu_baseline", "f32_mfma_path", "epoch_stream", "presets", "detail"):
        assert line.get(k) is None, k
    assert "f16x2_path" not in line
    names = sorted(os.listdir(tmp_path / "a"))
    assert {"scores.npy", "loss.npy", "param.encoder.W_h.weight.npy", "grad.encoder.W_h.weight.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    scores = np.load(tmp_path / "a" / "scores.npy")
    assert scores.dtype == np.float32 and scores.shape[0] == 64 * 64 and np.isfinite(scores).all()
    _run(args + ["--dump-outputs", str(tmp_path / "b")], _env())
    assert sorted(os.listdir(tmp_path / "b")) == names
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape, n
        np.testing.assert_array_equal(a, b, err_msg=n)


def test_gpus_2_without_a_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 2` as the driver may run it: the parent starts torch.distributed.run as a child before touching
    the GPU and relays rank 0's line.  On a one-GPU box the two ranks share GPU 0 and talk over gloo."""
    import torch
    extra = {} if torch.cuda.device_count() >= 2 else dict(RR_SINGLE_DEVICE="1", RR_DIST_BACKEND="gloo")
    line, _ = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--no-presets", "--no-epoch", "--no-cpu-baseline", "--no-f32-path",
                    "--no-fwd-only"], _env(**extra))
    assert line["n_gpus"] == 2 and line["config"]["parallelism"] == "dp2" and line["scaling"] == "weak"
    assert len(line["dp"]["rccl_ranks"]) == 2 and {r["rank"] for r in line["dp"]["rccl_ranks"]} == {0, 1}
    assert line["dp"]["allreduce_us"]["calls"] >= 2 and line["value"] > 0
