"""Every output of the evaluation and selection entry points that tools/window_loss_bits.py does not reach, as one .npz - to
be run with two builds of the library (RR_LIB_PATH) on one MI355X and compared byte for byte:
    python tools/per_query_bits.py --out A.npz
    python tools/per_query_bits.py --compare A.npz B.npz    (prints the array count and the names that differ; status 1 on any)
Per seed, a ragged window with list lengths 0, 1, 2, 63, 64, 65, 257, 1000 and tied values: eval.ranking_stats,
eval.pairwise_stats_from_scores, eval.rank_correlation_stats and uncertainty.top1_sets at each wave pin, uncertainty.sample_stats
(T = 3), uncertainty.analytic_stats; then neighbors.knn and neighbors.kcenter_greedy (plain and weighted) on a pool with
duplicate rows at widths 37, 300 and 1100."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import eval as RE  # noqa: E402
from reactranker_amd import neighbors as NB  # noqa: E402
from reactranker_amd import uncertainty as UQ  # noqa: E402
from reactranker_amd._lib import lib  # noqa: E402
from tools.window_loss_bits import compare  # noqa: E402

SEEDS = (0, 1)
LENGTHS = (0, 1, 2, 63, 64, 65, 257, 1000)
OUT = {}


def put(name, x):
    assert name not in OUT, name
    OUT[name] = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def put_all(name, d):
    for k, v in (d.items() if isinstance(d, dict) else enumerate(d)):
        put(f"{name}/{k}", v)


def window_outputs(seed):
    rng = np.random.default_rng(seed)
    scope = [int(c) for c in rng.permutation(LENGTHS)]
    M = sum(scope)
    score = torch.tensor(np.round(rng.standard_normal(M) * 2).astype(np.float32) / 2).cuda()     # ties inside every longer list
    t = torch.tensor(np.round(rng.standard_normal(M) * 2).astype(np.float32) / 2)
    tag = f"s{seed}"
    put_all(tag + "/ranking_stats", RE.ranking_stats(score, scope, t, 0))
    put_all(tag + "/pairwise_stats", RE.pairwise_stats_from_scores(score, scope, t, 1.0, 0))
    p = torch.tensor(np.round(rng.random(M) * 8).astype(np.float32) / 8).cuda()
    for waves in (0, 1, 4):
        assert lib().rr_rank_correlation_set_waves(waves) == 0 and lib().rr_top1_sets_set_waves(waves) == 0
        put(f"{tag}/rank_correlation/w{waves}", RE.rank_correlation_stats(score, scope, t, 0))
        put_all(f"{tag}/top1_sets/w{waves}", UQ.top1_sets(p, scope, t, 0.4, 0))
    assert lib().rr_rank_correlation_set_waves(0) == 0 and lib().rr_top1_sets_set_waves(0) == 0
    samples = torch.stack([score, score.flip(0), score])
    put_all(tag + "/sample_stats", UQ.sample_stats(samples, scope, t, 0))
    head = torch.stack([score, 0.25 + p], 1)
    put_all(tag + "/analytic_stats", UQ.analytic_stats(head, scope, t, "gaussian", 32, 0))


def selection_outputs(seed, H):
    rng = np.random.default_rng(100 + seed)
    x = np.round(rng.standard_normal((3000, H)) * 2).astype(np.float32) / 2
    x[1500:] = x[:1500]                                              # every row twice: ties in every distance and score
    x = torch.tensor(x).cuda()
    tag = f"s{seed}/h{H}"
    put_all(tag + "/knn", NB.knn(x[:257], x, 16))
    put_all(tag + "/kcenter", NB.kcenter_greedy(x, 65))
    w = torch.tensor((1 + rng.integers(0, 3, 3000)).astype(np.float32)).cuda()
    put_all(tag + "/kcenter_weighted", NB.kcenter_greedy(x, 65, weight=w))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar="NPZ", default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    for seed in SEEDS:
        window_outputs(seed)
        for H in (37, 300, 1100):
            selection_outputs(seed, H)
    np.savez(args.out, **OUT)
    print(f"{len(OUT)} arrays -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
