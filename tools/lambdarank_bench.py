"""Isolated timing of the LambdaRank step launch (rr_lambdarank_step_f32: loss and gradient in one launch) next to RankNet's
two entry points for the same window (rr_ranknet_fwd_f32, which ends in the one-wave finish launch, + rr_ranknet_bwd_f32), at the
workload's window (256 queries of 64 candidates) and at long lists (64 queries of 1000):
    python tools/lambdarank_bench.py
Prints microseconds per call (median of 5 x 30 back-to-back calls) and pairs per second.  No threshold: LambdaRank does more
per pair (two rankings, a weight, the stable softplus); the figure shows what the weighting costs."""
import os, sys, statistics
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from reactranker_amd._lib import lib, ptr, stream, check
dev = "cuda"


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


for Q, C in ((256, 64), (64, 1000)):
    s, tg, seg = window(Q, C)
    n_pairs = Q * C * (C - 1)                                        # ordered pairs (all targets of a query are distinct)
    loss, pairs = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    part, d = torch.empty(2 * Q, device=dev), torch.empty(Q * C, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    scale = 1.0 / n_pairs
    gl = torch.full((1,), scale, device=dev)
    L = lib()

    def ranknet():
        check(L.rr_ranknet_fwd_f32(ptr(s), 1, ptr(tg), ptr(seg), Q, C, 1.0, ptr(loss), ptr(pairs), ptr(part), stream()))
        check(L.rr_ranknet_bwd_f32(ptr(s), 1, ptr(tg), ptr(seg), Q, C, 1.0, 0, ptr(gl), ptr(d), 1, stream()))

    def lambdarank(k):
        check(L.rr_lambdarank_step_f32(ptr(s), 1, ptr(tg), ptr(seg), Q, C, 1.0, k, scale, ptr(loss), ptr(pairs), ptr(part),
                                       ptr(counter), ptr(d), 1, stream()))

    print(f"window {Q} x {C} ({n_pairs} ordered pairs)")
    forms = [("rr_ranknet_fwd_f32 + rr_ranknet_bwd_f32", ranknet)]
    forms += [(f"rr_lambdarank_step_f32, ndcg_k {k}", (lambda k=k: lambdarank(k))) for k in (0, 10)]
    for name, fn in forms:
        us = t(fn)
        print(f"  {name:44s} {us:9.1f} us   {n_pairs / us * 1e-3:8.2f} G pairs/s")
    assert int(pairs) == n_pairs and int(counter) == 0
