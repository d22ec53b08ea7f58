#!/usr/bin/env python3
"""Time of MC-dropout evaluation: uncertainty.mc_dropout_predict with T samples over B ListMLE-shaped batches (64 queries x
64 candidates, H = 300, dropout 0.1) beside what a user did before it - T train-mode passes of evaluate_top_scores plus
calculate_ndcg(is_order=True), whose per-candidate listing is built on the host one query at a time.  Both sides end in a
device synchronise; one untimed round of each warms the shapes up.  Prints one JSON line.
Usage: python tools/uq_bench.py [T=30] [batches=20]"""
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from reactranker_amd import eval as RE, featurization, synth   # noqa: E402
from reactranker_amd import uncertainty as U                   # noqa: E402
from reactranker_amd.base_model import build_model             # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 30
B = int(sys.argv[2]) if len(sys.argv) > 2 else 20
torch.cuda.set_device(0)
torch.manual_seed(0)
model = build_model(hidden_size=300, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.1, task_num=1,
                    ffn_last_layer="with_softplus", add_features_dim=1).cuda()
batches = []
for i in range(B):
    qb = synth.make_queries(700 + i, 64, 64)
    rb, pb = featurization.BatchMolGraph(qb.r_specs, K=4), featurization.BatchMolGraph(qb.p_specs, K=4)
    batches.append((rb, pb, qb.scope, torch.tensor(qb.targets), qb.add_features))      # host targets: calculate_ndcg lists them


def new_path():
    return U.mc_dropout_predict(model, batches, T, seed=0, gpu=0)


def old_path():
    model.train()
    for _ in range(T):
        with torch.no_grad():
            RE.evaluate_top_scores(model, 0, batches, ratio=0.25)
            RE.calculate_ndcg(model, 0, batches, NDCG_cut=0.25, is_order=True)
    model.eval()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


timed(new_path)
timed(old_path)
t_new = [timed(new_path) for _ in range(3)]
t_old = [timed(old_path) for _ in range(2)]
print(json.dumps(dict(T=T, batches=B, queries=64, cands=64, H=300, mc_dropout_predict_s=min(t_new),
                      mc_dropout_predict_all_s=t_new, T_x_evaluate_top_scores_plus_calculate_ndcg_s=min(t_old),
                      old_all_s=t_old)))
