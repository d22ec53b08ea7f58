#!/usr/bin/env python3
"""Time `train_listwise.batch_loss` + `loss.backward` per composite task type at 64 queries x 64 candidates with device
events over a warmed-up loop, once with loss.FusedStep on (rr_task_loss_step_f32: one launch for the loss and its gradient)
and once with FusedStep.enabled = False (the per-term path), and count the kernel launches of one step for both.
Needs an MI355X.

    python tools/task_loss_bench.py [--iters 400] [--chunks 5] [--no-launches]

The launch counts come from a `rocprofv3 --kernel-trace` run of its own: the tool starts itself as a fresh child process
under rocprofv3 (`--trace-child`), which runs a fixed number of steps per task type and mode with one rr_digamma_f32 launch
(a kernel none of these losses uses) as the separator, and counts the kernels between separators in the trace.

The tool only uses batch_loss, loss.backward and loss.FusedStep, so the same file also runs in a tree that predates the
step entry (there both columns time the per-term path, which is what an A/B against such a tree wants)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reactranker_amd import loss as RL  # noqa: E402
from reactranker_amd import train_listwise as TL  # noqa: E402

TASKS = ["mle_gaussian", "listnet_gauss", "mle_regression", "listnet_regression", "mledis_gaussian", "listnetdis_gauss",
         "listnet_uq", "dirichlet_uq"]
Q, C = 64, 64
TRACE_STEPS = 10


def inputs():
    M = Q * C
    rng = np.random.default_rng(0)
    sp = lambda x: np.log1p(np.exp(x))                                          # noqa: E731
    two = np.stack([rng.standard_normal(M), sp(rng.standard_normal(M)) + 1e-2], 1).astype(np.float32)
    outs = {
        2: torch.tensor(two).cuda().requires_grad_(True),                        # [M, 2]: score, positive variance column
        1: torch.tensor(rng.standard_normal(M).astype(np.float32)).cuda().requires_grad_(True),
        "pos": torch.tensor((sp(rng.standard_normal(M)) + 1.0).astype(np.float32)).cuda().requires_grad_(True),
    }
    t = torch.tensor(rng.standard_normal(M).astype(np.float32)).cuda()
    return outs, t


def out_for(task, outs):
    if task in ("listnet_uq", "dirichlet_uq"):
        return outs["pos"]
    return outs[1] if task.endswith("_regression") else outs[2]


def step(task, outs, t, scope):
    o = out_for(task, outs)
    o.grad = None
    RL.backward(TL.batch_loss(task, o, scope, t, 0, 1, 3, 0.2))


def trace_child():
    """Under rocprofv3: TRACE_STEPS steps per (mode, task), separated by one digamma launch each."""
    outs, t = inputs()
    scope = [C] * Q
    x = torch.ones(1, device="cuda")
    for fused in (True, False):
        RL.FusedStep.enabled = fused
        for task in TASKS:
            step(task, outs, t, scope)                                           # warm-up (allocator, cached segments)
            torch.cuda.synchronize()
            RL.digamma(x)
            for _ in range(TRACE_STEPS):
                step(task, outs, t, scope)
            torch.cuda.synchronize()
            RL.digamma(x)
    torch.cuda.synchronize()


def count_launches():
    """{mode: {task: (launches per step, [kernel names of one step])}} from a rocprofv3 kernel trace of a child process."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--trace-child"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600, cwd=d)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel trace")
        rows = []
        for f in files:
            rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    cuts = [i for i, n in enumerate(names) if "digamma_kernel" in n]
    if len(cuts) != 4 * len(TASKS):
        raise RuntimeError(f"expected {4 * len(TASKS)} separators in the trace, found {len(cuts)}")
    res = {"fused": {}, "per_term": {}}
    k = 0
    for mode in ("fused", "per_term"):
        for task in TASKS:
            seg = names[cuts[k] + 1:cuts[k + 1]]
            k += 2
            per = len(seg) // TRACE_STEPS
            short = [n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:60] for n in seg[:per]]
            res[mode][task] = (len(seg) / TRACE_STEPS, short, round(sum(dur[cuts[k - 2] + 1:cuts[k - 1]]) / TRACE_STEPS, 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400, help="steps per timed chunk")
    ap.add_argument("--chunks", type=int, default=5, help="timed chunks per task type and mode; the median is reported")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-launches", action="store_true", help="skip the rocprofv3 child run that counts kernel launches")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_child:
        return trace_child()
    outs, t = inputs()
    scope = [C] * Q
    res, spread = {"fused": {}, "per_term": {}}, {"fused": {}, "per_term": {}}
    for mode, fused in (("fused", True), ("per_term", False)):
        RL.FusedStep.enabled = fused
        for task in TASKS:
            for _ in range(args.warmup):
                step(task, outs, t, scope)
            torch.cuda.synchronize()
            chunks = []
            for _ in range(args.chunks):                                        # the median chunk: other work shares the host
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    step(task, outs, t, scope)
                e1.record()
                torch.cuda.synchronize()
                chunks.append(e0.elapsed_time(e1) * 1000.0 / args.iters)
            res[mode][task] = round(float(np.median(chunks)), 2)
            spread[mode][task] = (round(min(chunks), 2), round(max(chunks), 2))
    RL.FusedStep.enabled = True
    launches = None
    if not args.no_launches:
        del outs, t
        launches = count_launches()
    print("us per step (batch_loss + loss.backward, device events, median of the chunks [min .. max]); launches per step and the sum of "
          "their kernel durations from the kernel trace")
    print(f"{'task type':20s} {'fused':>8s} {'[min .. max]':>18s} {'per-term':>9s} {'[min .. max]':>18s}"
          + ("   launches fused / per-term   kernel us fused / per-term" if launches else ""))
    for task in TASKS:
        (f0, f1), (p0, p1) = spread["fused"][task], spread["per_term"][task]
        line = f"{task:20s} {res['fused'][task]:8.2f} {f'[{f0} .. {f1}]':>18s} {res['per_term'][task]:9.2f} {f'[{p0} .. {p1}]':>18s}"
        if launches:
            line += (f"   {launches['fused'][task][0]:8.1f} / {launches['per_term'][task][0]:<8.1f}"
                     f"   {launches['fused'][task][2]:8.2f} / {launches['per_term'][task][2]:.2f}")
        print(line)
    if launches:
        for mode in ("fused", "per_term"):
            for task in TASKS:
                print(f"kernels of one {mode} step, {task}: " + "; ".join(launches[mode][task][1]))
    print(json.dumps(dict(queries=Q, candidates=C, iters=args.iters, chunks=args.chunks, us_per_step=res, us_min_max=spread,
                          launches_per_step=None if launches is None else
                          {m: {k: v[0] for k, v in launches[m].items()} for m in launches},
                          kernel_us_per_step=None if launches is None else
                          {m: {k: v[2] for k, v in launches[m].items()} for m in launches})))


if __name__ == "__main__":
    main()
