"""Data-parallel training of the task types outside the five single-normaliser ones (tests/test_gpu_dp_trainers.py holds
those): the four older composites and the six newer non-NIG task types.  A fresh 2-process job (tests/dp_task_types_job.py
under `python -m torch.distributed.run`, every rank holding a RAGGED shard of every global step) must reproduce the
1-process job's per-epoch training loss, validation metrics and checkpoint decisions over three epochs - the bounds
tests/test_gpu_dp_trainers.py sets, on the default three-term arithmetic.  The four NIG task types must raise a ValueError
that names the task type, on both ranks, before any step.  On a one-GPU box the two ranks share GPU 0 (RR_SINGLE_DEVICE=1)
and talk over gloo; with two GPUs the same file runs over RCCL."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB = os.path.join(REPO, "tests", "dp_task_types_job.py")
TASKS = ["mle_gaussian", "listnet_gauss", "mle_regression", "listnet_regression", "mledis_gaussian", "listnetdis_gauss",
         "listnetdis_lognorm", "listnet_uq", "dirichlet_uq", "regression_exploss"]
FUSED = set(TASKS) - {"listnetdis_lognorm", "regression_exploss"}
NIG = ["evidential", "mle_evidential", "mledis_evidential", "listnet_evidential"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dp_task_types")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("RR_F16X2", None)                       # the default arithmetic: a query's scores do not depend on its batch mates
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    one = str(d / "one.json")
    subprocess.run([sys.executable, JOB, "--out", one, "--tasks", ",".join(TASKS)], check=True, env=env, timeout=900)
    env2 = dict(env)
    if torch.cuda.device_count() < 2:
        env2.update(RR_SINGLE_DEVICE="1", RR_DIST_BACKEND="gloo")
    else:
        env2.setdefault("RR_DIST_BACKEND", "nccl")
    two = str(d / "two.json")
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                    "127.0.0.1", "--master-port", str(_free_port()), JOB, "--out", two, "--tasks", ",".join(TASKS),
                    "--refused", ",".join(NIG)], check=True, env=env2, timeout=900)
    with open(one) as f:
        a = json.load(f)
    with open(two) as f:
        b = json.load(f)
    assert a["world"] == 1 and b["world"] == 2
    return a, b


@pytest.mark.parametrize("task", TASKS)
def test_two_process_trainer_reproduces_the_one_process_trainer(jobs, task, parity_log):
    a, b = jobs
    h1, h2 = a["result"][task]["history"], b["result"][task]["history"]
    assert len(h1) == len(h2) == 3
    worst_loss = worst_metric = 0.0
    for e1, e2 in zip(h1, h2):
        rel = abs(e1["train_loss"] - e2["train_loss"]) / max(1e-6, abs(e1["train_loss"]))
        worst_loss = max(worst_loss, rel)
        for k in ("top1", "top1_in_pred_top25", "pred_top25_in_targ_top25"):
            worst_metric = max(worst_metric, abs(e1[k] - e2[k]))
        worst_metric = max(worst_metric, max(abs(x - y) for x, y in zip(e1["ndcg"], e2["ndcg"])))
        assert e1["checkpoint"] == e2["checkpoint"]
    line = (f"{task} backend={b['backend']}: losses 1proc {[e['train_loss'] for e in h1]} 2proc {[e['train_loss'] for e in h2]}; "
            f"max rel |loss_2proc - loss_1proc| {worst_loss:.2e}, max |metric diff| {worst_metric:.2e}")
    parity_log(line)
    print(line)
    assert worst_loss <= 1e-5 and worst_metric <= 1e-5, (task, worst_loss, worst_metric)
    # every optimizer step of a fused task type took the one-launch loss (4 steps x 3 epochs; rank 0 holds a shard of each)
    want = 12 if task in FUSED else 0
    assert a["result"][task]["fused_hits"] == want and b["result"][task]["fused_hits"] == want


@pytest.mark.parametrize("task", NIG)
def test_cross_step_task_types_are_refused_on_both_ranks_before_any_step(jobs, task):
    _, b = jobs
    per_rank = b["refused"][task]
    assert len(per_rank) == 2
    for r in per_rank:
        assert r["error"] is not None and task in r["error"], r
        assert r["steps"] == 0, r
