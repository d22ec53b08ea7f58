#!/usr/bin/env python3
"""Time of single-forward uncertainty beside MC dropout, on one batch of 64 queries x 64 candidates and one of 64 x 1000
(Gaussian head, H = 300, dropout 0.1; molecules of 5 to 12 atoms, so that the 64,000-reaction batch keeps every activation
tensor under 2 GiB):
  analytic_stats        the rr_analytic_rank_stats_f32 call alone on the forward's output (32 nodes)
  distribution_predict  one eval-mode forward + analytic_stats
  mc_dropout_predict    T = 30 train-mode forwards + rr_mc_sample_stats_f32, on the same batch
Each figure is the median over 5 rounds of the mean of 30 back-to-back calls (mc_dropout_predict: 3 calls), every round
ending in a device synchronise; one untimed round warms the shapes up.  Writes the table to the given file.
Usage: python tools/analytic_uq_bench.py [out=profiles/analytic_uq_bench.txt] [n_nodes=32]"""
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from reactranker_amd import featurization, synth               # noqa: E402
from reactranker_amd import uncertainty as U                   # noqa: E402
from reactranker_amd.base_model import build_model             # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "analytic_uq_bench.txt")
NODES = int(sys.argv[2]) if len(sys.argv) > 2 else 32
T, ROUNDS, CALLS = 30, 5, 30
torch.cuda.set_device(0)
torch.manual_seed(0)
model = build_model(hidden_size=300, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.1, task_num=2,
                    ffn_last_layer="with_softplus", task_type="gauss_regression", add_features_dim=1).cuda()


def timed(fn, calls):
    """median over ROUNDS of (time of `calls` back-to-back calls) / calls, in seconds"""
    fn()
    per_call = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) / calls)
    return statistics.median(per_call)


lines = [f"analytic_uq_bench: one MI355X, Gaussian head, H = 300, dropout 0.1, n_nodes = {NODES}, MC dropout T = {T}; "
         f"median of {ROUNDS} rounds x {CALLS} calls (mc_dropout_predict: x 3 calls), ms per call",
         f"{'queries x cands':>16} {'analytic_stats':>15} {'distribution_predict':>21} {'mc_dropout_predict':>19} {'worst |mass-1|':>15}"]
for cands in (64, 1000):
    qb = synth.make_queries(900 + cands, 64, cands, atoms_lo=5, atoms_hi=12)
    batch = (featurization.BatchMolGraph(qb.r_specs, K=4), featurization.BatchMolGraph(qb.p_specs, K=4), qb.scope,
             torch.tensor(qb.targets).cuda(), qb.add_features)
    res = U.distribution_predict(model, [batch], n_nodes=NODES, gpu=0)[0]
    out = res["output"]
    t_stats = timed(lambda: U.analytic_stats(out, batch[2], batch[3], "gaussian", NODES, 0), CALLS)
    t_dist = timed(lambda: U.distribution_predict(model, [batch], n_nodes=NODES, gpu=0), CALLS)
    t_mc = timed(lambda: U.mc_dropout_predict(model, [batch], T, seed=0, gpu=0), 3)
    lines.append(f"{'64 x ' + str(cands):>16} {t_stats * 1e3:15.3f} {t_dist * 1e3:21.3f} {t_mc * 1e3:19.3f} "
                 f"{float((res['mass'] - 1).abs().max()):15.2e}")
    print(lines[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
