"""Isolated timing of the ApproxNDCG step launch (rr_approx_ndcg_step_f32: loss and gradient in one launch) next to the
LambdaRank step on the same windows (rr_lambdarank_step_f32), at the workload's window (256 queries of 64 candidates) and at
long lists (64 queries of 1000), and of its one-wave instantiation at the long lists (rr_approx_ndcg_set_waves pins the wave
count: both forms of one build in one process):
    python tools/approx_ndcg_bench.py [--out profiles/approx_ndcg_bench.txt]
Prints, and with --out also writes to that file, microseconds per call (median of 5 x 30 back-to-back calls) and pairs per second.  No threshold: ApproxNDCG walks every
pair twice (the soft ranks, then the gradient through them), each walk with one expf and one division per pair; the figures
show what that costs next to LambdaRank's one walk, and what the four-wave workgroup buys on long lists."""
import argparse, os, sys, statistics
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from reactranker_amd._lib import lib, ptr, stream, check
dev = "cuda"
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
ARGS = ap.parse_args()
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def t(fn, n=30, reps=5):
    for _ in range(5):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n * 1e3)
    return statistics.median(out)


def window(Q, C, seed=0):
    rng = np.random.default_rng(seed)
    score = (rng.standard_normal(Q * C) * 2).astype(np.float32)
    targets = np.concatenate([rng.permutation(C) for _ in range(Q)]).astype(np.float32)
    targets = (targets - targets.mean()) / (targets.std() + 1e-6)
    seg = (np.arange(Q + 1) * C).astype(np.int32)
    return torch.tensor(score).to(dev), torch.tensor(targets.astype(np.float32)).to(dev), torch.tensor(seg).to(dev)


L = lib()
TIMES = {}
for Q, C in ((256, 64), (64, 1000)):
    s, tg, seg = window(Q, C)
    n_pairs = Q * C * (C - 1)                                        # ordered pairs
    loss, count = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    part, d = torch.empty(2 * Q, device=dev), torch.empty(Q * C, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)

    def lambdarank(k):
        check(L.rr_lambdarank_step_f32(ptr(s), 1, ptr(tg), ptr(seg), Q, C, 1.0, k, 1.0 / n_pairs, ptr(loss), ptr(count), ptr(part),
                                       ptr(counter), ptr(d), 1, stream()))

    def approx_ndcg(k):
        check(L.rr_approx_ndcg_step_f32(ptr(s), 1, ptr(tg), ptr(seg), Q, C, 1.0, k, 1.0 / Q, ptr(loss), ptr(count), ptr(part),
                                        ptr(counter), ptr(d), 1, stream()))

    say(f"window {Q} x {C} ({n_pairs} ordered pairs)")
    forms = [(f"rr_lambdarank_step_f32, ndcg_k {k}", 0, (lambda k=k: lambdarank(k))) for k in (0, 10)]
    forms += [(f"rr_approx_ndcg_step_f32, ndcg_k {k}", 0, (lambda k=k: approx_ndcg(k))) for k in (0, 10)]
    if C > 64:
        forms += [("rr_approx_ndcg_step_f32, ndcg_k 0, pinned to 1 wave", 1, lambda: approx_ndcg(0)),
                  ("rr_approx_ndcg_step_f32, ndcg_k 0, pinned to 4 waves", 4, lambda: approx_ndcg(0))]
    for name, waves, fn in forms:
        check(L.rr_approx_ndcg_set_waves(waves))
        try:
            us = TIMES[name] = t(fn)
        finally:
            check(L.rr_approx_ndcg_set_waves(0))
        say(f"  {name:56s} {us:9.1f} us   {n_pairs / us * 1e-3:8.2f} G pairs/s")
    assert int(count) == Q and int(counter) == 0
    if C > 64:
        one, four = TIMES["rr_approx_ndcg_step_f32, ndcg_k 0, pinned to 1 wave"], TIMES["rr_approx_ndcg_step_f32, ndcg_k 0, pinned to 4 waves"]
        say(f"  four waves against one at {Q} x {C}: {one / four:.2f}x" + ("" if four < one else "  (four waves do NOT beat one here)"))
if ARGS.out:
    with open(ARGS.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
