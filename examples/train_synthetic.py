#!/usr/bin/env python3
"""main.py-shaped driver on synthetic reactions (the reference's main.py reads a CSV and needs RDKit; its flow is
build_model -> build_optimizer -> build_lr_scheduler -> train -> checkpoint, main.py:90-140).  Needs an MI355X.

    python examples/train_synthetic.py --task-type mle --epochs 5 --queries 256 --cands 32

The pairwise trainer's selectors (run_train_pairwise.run_train) are reached with --task-type ranknet (--train-strategy
sum_session | accelerate_grad | lambdarank | approx_ndcg, the last two with --ndcg-k, the last with --temperature), betanet,
betanet_evidential, or pair_baseline (the three-graph pair model):

    python examples/train_synthetic.py --task-type betanet --epochs 3 --queries 64 --cands 8
    python examples/train_synthetic.py --task-type ranknet --train-strategy lambdarank --ndcg-k 10 --epochs 3 --queries 64 --cands 32
    python examples/train_synthetic.py --task-type ranknet --train-strategy approx_ndcg --temperature 0.5 --epochs 3 --queries 64 --cands 32

Under `python -m torch.distributed.run --nproc-per-node N examples/train_synthetic.py ...` the listwise task types train data
parallel: every rank builds the same batches and keeps its block of whole queries of each (dp.shard_query_batch).  Backend:
$RR_DIST_BACKEND (default nccl = RCCL); RR_SINGLE_DEVICE=1 puts every rank on --gpu.  The four NIG task types need every target
of a step and are refused there (one process trains them).

A task type whose head predicts a distribution per candidate (evidential_ranking, mledis_gaussian, listnetdis_gauss, the NIG
ones) ends with the validation set's uncertainty from one forward per batch (uncertainty.evaluate_uncertainty,
method='distribution').

--evaluate-calibration (listwise task types, one process) holds out the first half of every validation batch's queries as the
calibration set and reports on the other half (uncertainty.evaluate_calibration): the fitted sigma scale with the pointwise
calibration before and after it, the top-1 calibration of p_top1, and the conformal top-1 sets at --alpha.  A distributional
head is read with method='distribution', any other with MC dropout.

--attribute grad_x_input | integrated_gradients [--ig-steps N] (listwise task types, one process) explains the first validation
query's predicted top candidate (attribution.attribute): the five product atoms and three bonds of largest |attribution|, the
attributions' total next to the score and, for integrated gradients, the gap that is left.

--neighbors K (listwise task types, one process) builds a bank of the training reactions' embeddings (neighbors.ReactionBank),
prints how the distance to the K nearest of them tracks the error on the validation set (neighbors.evaluate_applicability) and,
for every candidate of the first validation query, its K nearest training reactions with their targets.

--acquire N (listwise task types, one process) treats the validation reactions as an unlabelled pool and prints which N of
them to compute next (neighbors.acquire: greedy k-center from the bank of training embeddings, weighted by the head's own
predictive std where it has one), with the pool's coverage radius before and after.

--mahalanobis [--neighbors K] (listwise task types, one process) logs the applicability calibration with both distances side
by side: the mean distance to the K (default 8) nearest training reactions and the Mahalanobis distance to the Gaussian of the
training embeddings (latent_gaussian.EmbeddingGaussian, neighbors.evaluate_applicability(method='mahalanobis')).

--embedding-map N (listwise task types, one process) logs the explained variance of the first N principal components of the
training embeddings and writes the validation reactions' scores on them next to the checkpoint (<checkpoint>.embedding_map.pt:
scores [M, N], targets, scope, explained_variance_ratio).

--cluster-split RADIUS (listwise task types, one process) clusters the mean embedding of every query, training and validation
together, by sphere exclusion (clusters.sphere_exclusion; RADIUS 0: clusters.suggest_radius picks one), prints the cluster count
and sizes, sends whole clusters to train / validation / test folds (clusters.cluster_split) and prints, per held-out fold, the
quantiles of the distance to the nearest training query (clusters.split_report) next to a random split of the same fold sizes.

--fingerprint-neighbors K (listwise task types, one process) asks "has training seen this reaction?" of the structure instead of
the model: circular fingerprints of reactant and product, side by side, for every training and validation reaction
(fingerprints.reaction_fingerprint, mode='concat'), the K nearest training reactions of every validation reaction under the
Tanimoto distance (fingerprints.tanimoto_knn) and the validation reactions whose fingerprint a training reaction shares
(fingerprints.structure_overlap); it logs the mean structural nearest-neighbour similarity next to the mean latent distance
(neighbors.latent_distance) and the Spearman correlation of the two over the validation reactions.

--add-fingerprint [--fingerprint-bits N] (listwise task types, one process) trains with add_features_dim = N: the product's
binary circular fingerprint (fingerprints.feature_generate, made on the device, N bits, default 2048) takes the place of the
synthetic extra feature.

--bootstrap N (listwise task types, one process) prints the validation metrics of the restored best checkpoint with their 95 %
bootstrap intervals over the validation queries (significance.metric_intervals, N resamples), and the paired comparison of that
checkpoint against the last epoch's weights on the same queries: the difference per metric, its interval and the two-sided
sign-flip p-value (significance.paired_test, 5 N sign vectors).
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reactranker_amd import featurization, synth                      # noqa: E402
from reactranker_amd.base_model import build_model                    # noqa: E402
from reactranker_amd import attribution, clusters, fingerprints, latent_gaussian, neighbors, ranknet_baseline, significance, uncertainty   # noqa: E402
from reactranker_amd.run_train_pairwise import run_train              # noqa: E402
from reactranker_amd.train_listwise import train                      # noqa: E402
from reactranker_amd.train_utils import build_lr_scheduler, build_optimizer, param_count   # noqa: E402
from reactranker_amd.utils import load_checkpoint                     # noqa: E402


def make_batches(seed, n_queries, cands, per_batch, rank=0, world=1):
    out = []
    for b0 in range(0, n_queries, per_batch):
        qb = synth.make_queries(seed + b0, min(per_batch, n_queries - b0), cands)
        # a learnable target: a fixed function of the product graph and the extra feature, distinct inside a query
        tg = np.array([s.edges.shape[0] for s in qb.p_specs], np.float32) * 0.3 + qb.add_features[:, 0]
        tg = (tg - tg.mean()) / (tg.std() + 1e-6) + 1e-3 * np.arange(len(tg), dtype=np.float32)
        qb.targets = tg.astype(np.float32)
        extra = {}
        if world > 1:                                     # this rank's whole queries of the step + the step's counts
            from reactranker_amd import dp
            qb, glob = dp.shard_query_batch(qb, rank, world)
            extra["global"] = glob
        some = len(qb.scope) > 0
        out.append(dict(r=featurization.BatchMolGraph(qb.r_specs, K=4) if some else None,
                        p=featurization.BatchMolGraph(qb.p_specs, K=4) if some else None,
                        scope=qb.scope, targets=torch.tensor(qb.targets), add=qb.add_features,
                        mols_r=qb.r_specs, mols_p=qb.p_specs, **extra))
    return out


def halves(b):
    """the first and the second half of a batch's queries as two batches of the same form"""
    q = len(b["scope"]) // 2
    m = int(sum(b["scope"][:q]))
    out = []
    for qs, ms in ((slice(0, q), slice(0, m)), (slice(q, None), slice(m, None))):
        out.append(dict(r=featurization.BatchMolGraph(b["mols_r"][ms], K=4), p=featurization.BatchMolGraph(b["mols_p"][ms], K=4),
                        scope=list(b["scope"][qs]), targets=b["targets"][ms], add=b["add"][ms]))
    return out


def explain_top_candidate(model, b, method, steps, gpu, log):
    """The atoms and bonds of the product that moved the score of the first query's predicted top candidate."""
    res = attribution.attribute(model, b["r"], b["p"], b["add"], column=0, method=method, steps=steps, gpu=gpu)
    n0 = int(b["scope"][0])
    top = int(torch.argmax(res["score"][:n0]))
    start, size = b["p"].a_scope[top]
    b_start, b_size = b["p"].b_scope[top]
    atom = res["atom_p"][start:start + size].cpu().numpy()
    sym = res["bond_sym_p"][b_start:b_start + b_size].cpu().numpy()[0::2]        # one number per undirected bond
    edges = b["mols_p"][top].edges
    log.info("attribution (%s) of candidate %d of query 0: score %.5f, total %.5f%s", method, top, float(res["score"][top]),
             float(res["total"][top]), f", gap {float(res['gap'][top]):.2e}" if "gap" in res else "")
    for i in np.argsort(-np.abs(atom))[:5]:
        log.info("  atom %2d  %+.5f", int(i), float(atom[i]))
    for e in np.argsort(-np.abs(sym))[:3]:
        log.info("  bond %2d-%-2d  %+.5f", int(edges[e][0]), int(edges[e][1]), float(sym[e]))


def nearest_training_reactions(model, train_b, val_b, checkpoint, k, gpu, log):
    """Applicability domain and explanation by example from a bank of the training reactions' embeddings."""
    as_tuple = lambda b: (b["r"], b["p"], b["scope"], b["targets"], b["add"])          # noqa: E731
    bank = neighbors.ReactionBank.from_batches(model, [as_tuple(b) for b in train_b], gpu)
    res = neighbors.evaluate_applicability(model, bank, val_b, checkpoint, gpu, k=k, target_name=None)
    cal = res["calibration"]
    log.info("applicability (bank of %d training reactions, k %d): Spearman(error, latent distance) %.3f; mean latent distance %.4f",
             len(bank), k, cal["spearman"], float(res["distance"].mean()))
    log.info("  error left after removing the most distant rows: %s",
             ", ".join(f"{f:.1f}: mae {m:.4f}" for f, m in zip(cal["fractions"][::3], cal["mae"][::3])))
    b = val_b[0]
    n0 = int(b["scope"][0])
    vec = neighbors.reaction_vectors(model, [as_tuple(b)], gpu)[:n0]
    dist, idx, tgt = bank.query(vec, k)
    for c in range(n0):
        near = ", ".join(f"#{int(i)} (d {float(d):.4f}, target {float(t):+.3f})" for d, i, t in zip(dist[c], idx[c], tgt[c]))
        log.info("  query 0 candidate %2d (target %+.3f): %s", c, float(b["targets"][c]), near)


def structural_neighbours(model, train_b, val_b, k, gpu, log):
    """How close the validation reactions lie to the training ones by structure (Tanimoto on circular fingerprints) and by the
    model's embedding, side by side."""
    as_tuple = lambda b: (b["r"], b["p"], b["scope"], b["targets"], b["add"])          # noqa: E731
    fp = lambda bs: torch.cat([fingerprints.reaction_fingerprint(b["r"], b["p"], mode="concat", gpu=gpu) for b in bs])   # noqa: E731
    bank_bits, val_bits = fp(train_b), fp(val_b)
    dist, idx = fingerprints.tanimoto_knn(val_bits, bank_bits, k, bank_popcount=fingerprints.row_popcount(bank_bits))
    found = idx >= 0
    sim = torch.where(found, 1.0 - dist, torch.zeros_like(dist)).sum(dim=1) / found.sum(dim=1).clamp_min(1)
    same = fingerprints.structure_overlap(bank_bits, val_bits)
    bank = neighbors.ReactionBank.from_batches(model, [as_tuple(b) for b in train_b], gpu)
    latent = neighbors.latent_distance(bank, neighbors.reaction_vectors(model, [as_tuple(b) for b in val_b], gpu), k)
    # (the calibration's Spearman is that of |pred - target| and the third argument: with targets of zero, of `sim` and `latent`)
    rho = uncertainty.uncertainty_calibration(sim, torch.zeros_like(sim), latent)["spearman"]
    log.info("structural neighbours (%d bits per reaction, bank of %d training reactions, k %d): mean Tanimoto similarity to the k "
             "nearest %.4f, to the nearest %.4f; %d of %d validation reactions share a fingerprint with a training reaction",
             32 * bank_bits.shape[1], bank_bits.shape[0], k, float(sim.mean()), float(same["similarity"].mean()), same["count"],
             val_bits.shape[0])
    log.info("  next to the model's embedding: mean latent distance to the k nearest %.4f; Spearman(similarity, latent distance) %.3f",
             float(latent.mean()), rho)


def both_distances(model, train_b, val_b, checkpoint, k, gpu, log):
    """The applicability calibration with the k-nearest-neighbour distance and the Mahalanobis distance side by side."""
    as_tuple = lambda b: (b["r"], b["p"], b["scope"], b["targets"], b["add"])          # noqa: E731
    bank = neighbors.ReactionBank.from_batches(model, [as_tuple(b) for b in train_b], gpu)
    gauss = latent_gaussian.EmbeddingGaussian.from_bank(bank)
    log.info("embedding Gaussian of %d training reactions: %d of %d directions kept", gauss.n_, gauss.rank_, bank.vectors.shape[1])
    for method, kw in (("knn", dict(k=k)), ("mahalanobis", dict(gaussian=gauss))):
        res = neighbors.evaluate_applicability(model, bank, val_b, checkpoint, gpu, target_name=None, method=method, **kw)
        cal = res["calibration"]
        log.info("applicability, %-11s: Spearman(error, distance) %.3f; mean distance %.4f; mae after removing the most distant "
                 "rows: %s", method, cal["spearman"], float(res["distance"].mean()),
                 ", ".join(f"{f:.1f}: {m:.4f}" for f, m in zip(cal["fractions"][::3], cal["mae"][::3])))


def embedding_map(model, train_b, val_b, checkpoint, n, gpu, log):
    """PCA of the training embeddings: the explained variance of the first n components, the validation set's scores on them."""
    as_tuple = lambda b: (b["r"], b["p"], b["scope"], b["targets"], b["add"])          # noqa: E731
    gauss = latent_gaussian.EmbeddingGaussian.fit(neighbors.reaction_vectors(model, [as_tuple(b) for b in train_b], gpu))
    n = min(n, gauss.rank_)
    evr = gauss.explained_variance_ratio_[:n]
    log.info("embedding map: %d components explain %.1f %% of the variance (%s)", n, 100 * float(evr.sum()),
             ", ".join(f"{100 * float(v):.1f}" for v in evr))
    scores = gauss.project(neighbors.reaction_vectors(model, [as_tuple(b) for b in val_b], gpu), n)
    path = checkpoint + ".embedding_map.pt"
    torch.save(dict(scores=scores.cpu(), targets=torch.cat([torch.as_tensor(b["targets"]).reshape(-1) for b in val_b]),
                    scope=[int(c) for b in val_b for c in b["scope"]], explained_variance_ratio=evr), path)
    log.info("  scores of %d validation reactions written to %s", scores.shape[0], path)


def reactions_to_compute_next(model, train_b, val_b, n, gpu, log):
    """Batch acquisition: the validation reactions as the pool, the training reactions as what is labelled already."""
    as_tuple = lambda b: (b["r"], b["p"], b["scope"], None, b["add"])                  # noqa: E731  (a pool has no targets)
    bank = neighbors.ReactionBank.from_batches(model, [(b["r"], b["p"], b["scope"], b["targets"], b["add"]) for b in train_b], gpu)
    weight = "std" if model.ffn.head() in uncertainty.MOMENT_KIND_OF_HEAD else None   # no predicted variance: pure coverage
    res = neighbors.acquire(model, bank, [as_tuple(b) for b in val_b], n, gpu, weight=weight)
    log.info("acquisition (pool of %d validation reactions, bank of %d, weight %s): coverage radius %.4f -> %.4f after %d picks",
             res["min_dist"].numel(), len(bank), weight, float(res["radius_before"]), float(res["radius_after"]),
             int((res["rows"] >= 0).sum()))
    for t, (row, bt, q, c, gain) in enumerate(zip(*[res[k].cpu().tolist() for k in ("rows", "batch", "query", "candidate", "gain")])):
        if row >= 0:
            log.info("  pick %2d: pool row %4d = batch %d, query %2d, candidate %2d  (score %.5f; %d pool rows are nearest to it)",
                     t, row, bt, q, c, gain, int((res["assign"] == t).sum()))


def cluster_held_out_split(model, train_b, val_b, radius, gpu, log):
    """A cluster-held-out split of all queries next to a random split of the same fold sizes (clusters.sphere_exclusion on the
    mean reaction vector per query, clusters.cluster_split, clusters.split_report)."""
    as_tuple = lambda b: (b["r"], b["p"], b["scope"], b["targets"], b["add"])          # noqa: E731
    bank = neighbors.ReactionBank.from_batches(model, [as_tuple(b) for b in list(train_b) + list(val_b)], gpu)
    qv = clusters.query_vectors(bank.vectors, bank.group)
    if radius <= 0:
        radius = clusters.suggest_radius(qv, k=min(8, max(1, qv.shape[0] - 1)), quantile=0.5)
    res = clusters.sphere_exclusion(qv, radius)
    sizes = res["sizes"].cpu().tolist()
    log.info("cluster split: %d queries, radius %.4f -> %d clusters; sizes %s%s; %d singletons", qv.shape[0], radius, len(sizes),
             sizes[:12], " ..." if len(sizes) > 12 else "", sum(1 for s in sizes if s == 1))
    folds = clusters.cluster_split(res["labels"], (0.8, 0.1, 0.1), seed=0)
    counts = torch.bincount(folds, minlength=3).cpu().tolist()
    log.info("  folds by cluster (train / validation / test): %s queries", counts)
    g = torch.Generator().manual_seed(0)
    random_folds = torch.repeat_interleave(torch.arange(3), torch.tensor(counts))[torch.randperm(sum(counts), generator=g)].to(folds.device)
    for name, f in (("cluster", folds), ("random ", random_folds)):
        rep = clusters.split_report(qv, f, k=1)
        for fold, n, q in zip(rep["folds"], rep["n"], rep["quantiles"].tolist()):
            log.info("  %s split, fold %d (%3d queries): distance to the nearest training query, quantiles %s = %s", name, fold, n,
                     "/".join(f"{lv:g}" for lv in rep["levels"]), " ".join(f"{v:.4f}" for v in q))


def intervals_and_comparison(model, val_b, last_table, n, gpu, log):
    """What the validation means are worth: their bootstrap intervals, and whether the best checkpoint really beats the last epoch."""
    val = [(b["r"], b["p"], b["scope"], b["targets"], b["add"]) for b in val_b]
    iv = significance.metric_intervals(model, gpu, val, n_resamples=n)
    log.info("validation metrics of the best checkpoint, 95 %% bootstrap intervals over %d queries (%d resamples):",
             iv["top1"]["n"], n)
    for name, v in iv.items():
        log.info("  %-22s %8.4f  [%8.4f, %8.4f]  se %.4f  (n %d)", name, v["estimate"], v["lo"], v["hi"], v["se"], v["n"])
    best_table, names = significance.query_table(model, gpu, val)
    cmp = significance.paired_test(best_table, last_table, n_resamples=5 * n, names=names)
    log.info("best checkpoint against the last epoch's weights, paired over the same queries (sign-flip test, %d sign vectors):", 5 * n)
    for name, v in cmp.items():
        log.info("  %-22s diff %+8.4f  [%+8.4f, %+8.4f]  p %.4f  (wins %d, ties %d, losses %d)", name, v["diff"], v["lo"], v["hi"],
                 v["p_value"], v["wins"], v["ties"], v["losses"])


PAIRWISE = {   # --task-type -> (train_strategy or None = --train-strategy, run_train's task_type)
    "ranknet": (None, "baseline"), "betanet": ("sum_session", "BetaNet"),
    "betanet_evidential": ("sum_session", "BetaNet_envidential"), "pair_baseline": ("baseline", "baseline"),
}


def head_for(task_type):
    """task_num and head of the model each task type trains: the NIG (normal-inverse-gamma) losses read the four softplus'd
    columns of 'evidential_with_softplus', the '*dis_*' ones a mean / positive-variance pair, listnet_uq and dirichlet_uq
    the positive scores of 'listnet_with_uncertainty'."""
    if task_type in ("evidential", "mle_evidential", "mledis_evidential", "listnet_evidential"):
        return dict(task_num=4, ffn_last_layer="with_softplus", task_type=None)
    if task_type == "listnetdis_lognorm":
        return dict(task_num=2, ffn_last_layer="with_softplus", task_type="listnetdis_lognorm")
    if task_type in ("mledis_gaussian", "listnetdis_gauss"):
        return dict(task_num=2, ffn_last_layer="with_softplus", task_type=None)
    if task_type in ("listnet_uq", "dirichlet_uq"):
        return dict(task_num=1, ffn_last_layer="with_uncertainty", task_type="listnet")
    if task_type == "evidential_ranking":
        return dict(task_num=2, ffn_last_layer="no_softplus", task_type="evidential_ranking")
    if task_type in ("gauss_regression", "mle_gaussian", "listnet_gauss"):
        return dict(task_num=2, ffn_last_layer="no_softplus", task_type=None)
    return dict(task_num=1, ffn_last_layer="with_softplus", task_type=None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task-type", default="mle")
    ap.add_argument("--train-strategy", default="sum_session", help="with --task-type ranknet: sum_session | accelerate_grad | lambdarank | approx_ndcg")
    ap.add_argument("--ndcg-k", type=int, default=0, help="with --train-strategy lambdarank | approx_ndcg: NDCG truncation (0: the whole list)")
    ap.add_argument("--temperature", type=float, default=1.0, help="with --train-strategy approx_ndcg: soft-rank temperature, in score units")
    ap.add_argument("--pair-batch", type=int, default=256, help="with --task-type pair_baseline: pairs per optimizer step")
    ap.add_argument("--save-metric", default="NDCG@all", help="listwise task types: the checkpoint criterion, e.g. NDCG@all | average_score | "
                    "kendall_tau | spearman | mrr (the last three: mean per-query rank correlation, eval.rank_correlation)")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--cands", type=int, default=32)
    ap.add_argument("--batch-queries", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=300)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--evaluate-calibration", action="store_true", help="listwise task types: calibrate sigma and the top-1 sets on half "
                    "of the validation queries and report on the other half")
    ap.add_argument("--alpha", type=float, default=0.1, help="with --evaluate-calibration: the top-1 sets miss the best candidate with "
                    "probability at most alpha")
    ap.add_argument("--attribute", choices=attribution.METHODS, default=None, help="listwise task types: after training, which atoms "
                    "and bonds moved the score of the first validation query's predicted top candidate")
    ap.add_argument("--neighbors", type=int, default=0, metavar="K", help="listwise task types: after training, the applicability "
                    "calibration of the distance to the K nearest training reactions, and the first validation query's neighbours")
    ap.add_argument("--mahalanobis", action="store_true", help="listwise task types: after training, the applicability calibration "
                    "with the k-nearest-neighbour distance (k = --neighbors or 8) and the Mahalanobis distance side by side")
    ap.add_argument("--embedding-map", type=int, default=0, metavar="N", help="listwise task types: after training, the explained "
                    "variance of the first N principal components of the training embeddings; the validation scores are written out")
    ap.add_argument("--acquire", type=int, default=0, metavar="N", help="listwise task types: after training, which N validation "
                    "reactions to compute next (greedy k-center from the training embeddings) and the coverage radius before and after")
    ap.add_argument("--cluster-split", type=float, default=None, metavar="RADIUS", help="listwise task types: after training, sphere-"
                    "exclusion clusters of all queries' mean embeddings (0: a radius from clusters.suggest_radius), the folds of a "
                    "cluster-held-out split and their distance to the training fold next to a random split of the same sizes")
    ap.add_argument("--bootstrap", type=int, default=0, metavar="N", help="listwise task types: after training, the validation metrics "
                    "with 95 %% bootstrap intervals (N resamples of the queries) and the paired test of the best checkpoint against the last epoch")
    ap.add_argument("--fingerprint-neighbors", type=int, default=0, metavar="K", help="listwise task types: after training, the mean "
                    "Tanimoto similarity of the validation reactions to their K structurally nearest training reactions next to the latent distance")
    ap.add_argument("--add-fingerprint", action="store_true", help="listwise task types: train with the product's binary circular "
                    "fingerprint as the additional features (add_features_dim = --fingerprint-bits)")
    ap.add_argument("--fingerprint-bits", type=int, default=2048, help="with --add-fingerprint: bits of the fingerprint")
    ap.add_argument("--ig-steps", type=int, default=16, help="with --attribute integrated_gradients: midpoint nodes")
    ap.add_argument("--checkpoint", default="/tmp/reactranker_amd_synthetic/model.pt")
    args = ap.parse_args()
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    log = logging.getLogger("train_synthetic")
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:                                          # started by torch.distributed.run: data-parallel listwise training
        if args.task_type in PAIRWISE:
            raise SystemExit("examples/train_synthetic.py shards the listwise task types only; run the pairwise ones in one process")
        import torch.distributed as dist
        if not os.environ.get("RR_SINGLE_DEVICE"):
            args.gpu = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(args.gpu)
        dist.init_process_group(os.environ.get("RR_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
    if args.task_type == "pair_baseline":                 # positive outputs for pred_p = y / sum(y)
        model = ranknet_baseline.build_model(hidden_size=args.hidden, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True,
                                             dropout=0.1, task_num=2, ffn_last_layer="evidential")
    elif args.task_type == "betanet_evidential":          # positive scores: the evidence
        model = build_model(hidden_size=args.hidden, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.1,
                            add_features_dim=1, task_num=1, ffn_last_layer="evidential")
    elif args.task_type in PAIRWISE:
        model = build_model(hidden_size=args.hidden, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.1,
                            add_features_dim=1, task_num=1, ffn_last_layer="no_softplus")
    else:
        if args.add_fingerprint and world > 1:
            raise SystemExit("--add-fingerprint runs in one process")
        model = build_model(hidden_size=args.hidden, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.1,
                            add_features_dim=args.fingerprint_bits if args.add_fingerprint else 1, **head_for(args.task_type))
    log.info("parameters: %d", param_count(model))
    train_b = make_batches(0, args.queries, args.cands, args.batch_queries, rank, world)
    val_b = make_batches(10 ** 6, max(args.batch_queries, args.queries // 8), args.cands, args.batch_queries, rank, world)
    if args.add_fingerprint and args.task_type not in PAIRWISE:
        for b in list(train_b) + list(val_b):             # the product's fingerprint, made on the device, as the additional features
            b["add"] = fingerprints.feature_generate("binary_morgan_fingerprint", b["p"], num_bits=args.fingerprint_bits, gpu=args.gpu)
    opt = build_optimizer(model.cuda(args.gpu))
    sch = build_lr_scheduler(opt, warmup_epochs=2, total_epochs=args.epochs, train_data_size=args.queries,
                             batch_size=args.batch_queries, init_lr=1e-4, max_lr=1e-3, final_lr=1e-4)
    if args.task_type in PAIRWISE:
        strategy, task = PAIRWISE[args.task_type]
        hist = run_train(model, sch, train_b, val_b, args.checkpoint, opt, args.epochs, seed=0, gpu=args.gpu,
                         train_strategy=strategy or args.train_strategy, task_type=task, logger=log, target_name=None,
                         batch_size=args.pair_batch, val_batch_size=args.pair_batch, ndcg_k=args.ndcg_k, temperature=args.temperature)
        key = "acc" if args.task_type == "pair_baseline" else "top1"
        best = max(hist, key=lambda h: h[key])
        log.info("best epoch %d: %s %.4f", best["epoch"], key, best[key])
        load_checkpoint(args.checkpoint, model)
        log.info("checkpoint %s restored", args.checkpoint)
        return
    rng = np.random.default_rng(0)
    hist = train(model, sch, lambda ep: [train_b[i] for i in rng.permutation(len(train_b))], val_b, args.checkpoint, opt,
                 args.epochs, seed=0, gpu=args.gpu, task_type=args.task_type, logger=log, save_metric=args.save_metric)
    best = max(hist, key=lambda h: h["ndcg"][3])
    if "rank_correlation" in hist[-1]:
        log.info("last epoch's rank correlation: %s", hist[-1]["rank_correlation"])
    if world > 1:
        import torch.distributed as dist
        dist.barrier()                                    # rank 0 wrote the checkpoint
    if rank == 0:
        log.info("best epoch %d: NDCG@all %.4f top1 %.4f", best["epoch"], best["ndcg"][3], best["top1"])
    last_table = None
    if world == 1 and args.bootstrap:                     # the last epoch's per-query rows, before the best checkpoint replaces the weights
        last_table = significance.query_table(model, args.gpu, [(b["r"], b["p"], b["scope"], b["targets"], b["add"]) for b in val_b])[0]
    load_checkpoint(args.checkpoint, model)
    if rank == 0:
        log.info("checkpoint %s restored", args.checkpoint)
    if world == 1 and model.ffn.head() in uncertainty.MOMENT_KIND_OF_HEAD:
        # the head predicts a distribution per candidate: its uncertainty on the validation set from ONE forward per batch
        uq = uncertainty.evaluate_uncertainty(model, val_b, args.checkpoint, args.gpu, method="distribution", target_name=None)
        log.info("uncertainty (method='distribution', kind %s): %s, worst |mass - 1| %.1e, Spearman(error, std) %.3f",
                 uncertainty.MOMENT_KIND_OF_HEAD[model.ffn.head()],
                 ", ".join(f"{k} {v:.3f}" for k, v in zip(uncertainty.QSTAT_NAMES, uq["qstats"])), uq["mass_worst"],
                 uq["calibration"]["spearman"])
    if world == 1 and args.evaluate_calibration:
        method = "distribution" if model.ffn.head() in uncertainty.MOMENT_KIND_OF_HEAD else "MC_dropout"
        cal_b, test_b = zip(*[halves(b) for b in val_b if len(b["scope"]) >= 2])
        res = uncertainty.evaluate_calibration(model, cal_b, test_b, args.checkpoint, args.gpu, method=method, alpha=args.alpha,
                                               target_name=None)
        for when in ("before", "after"):
            pc = res["probabilistic"][when]
            log.info("calibration (%s), sigma scale %.3f: nll %.4f crps %.4f mean z^2 %.3f sharpness %.4f rmse %.4f "
                     "miscalibration area %.4f", method, pc["sigma_scale"], pc["nll"], pc["crps"], pc["z2_mean"], pc["sharpness"],
                     pc["rmse"], pc["miscalibration_area"])
        t1 = res["top1"]
        log.info("top-1 of p_top1 on %d test queries: accuracy %.3f, confidence %.3f, ECE %.3f, Brier %.3f", t1["n"], t1["accuracy"],
                 t1["confidence"], t1["ece"], t1["brier"])
        log.info("conformal top-1 sets at alpha %.2f: tau %.4f, coverage %.3f, mean set size %.2f of %.2f candidates", args.alpha,
                 res["tau"], res["coverage"], res["mean_set_size"], float(np.mean(res["scope"])))
    if world == 1 and args.attribute:
        explain_top_candidate(model, val_b[0], args.attribute, args.ig_steps, args.gpu, log)
    if world == 1 and args.neighbors:
        nearest_training_reactions(model, train_b, val_b, args.checkpoint, args.neighbors, args.gpu, log)
    if world == 1 and args.fingerprint_neighbors:
        structural_neighbours(model, train_b, val_b, args.fingerprint_neighbors, args.gpu, log)
    if world == 1 and args.mahalanobis:
        both_distances(model, train_b, val_b, args.checkpoint, args.neighbors or 8, args.gpu, log)
    if world == 1 and args.embedding_map:
        embedding_map(model, train_b, val_b, args.checkpoint, args.embedding_map, args.gpu, log)
    if world == 1 and args.acquire:
        reactions_to_compute_next(model, train_b, val_b, args.acquire, args.gpu, log)
    if world == 1 and args.cluster_split is not None:
        cluster_held_out_split(model, train_b, val_b, args.cluster_split, args.gpu, log)
    if world == 1 and args.bootstrap:
        intervals_and_comparison(model, val_b, last_table, args.bootstrap, args.gpu, log)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
