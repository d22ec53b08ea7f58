"""On-device ranking evaluation — mirror of the metric part of reference `reactranker/train/eval.py`
(`ranking_metrics` :475-555, `evaluate_top_scores` :76-177, `calculate_ndcg` :329-457, `compute_NDCG` :460-472) and
`reactranker/metrics.py` (NDCG@k).

The reference scores ONE query per forward and does the ranking in Python lists; here all queries of a batch are
scored in one forward and ranked by one kernel (one wavefront per query).  The data-loading half of the
reference's function (DataProcessor / SMILES parsing) is outside the hot path: callers hand in batches.
"""
from __future__ import annotations

from typing import Iterable, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .loss import _prep, _vec


NSTATS = 12          # RR_RANKING_NSTATS (include/reactranker_hip.h)
RANK_CORR_NSTATS = 8  # RR_RANK_CORR_NSTATS


def ranking_stats(scores: torch.Tensor, scope, targets, gpu: int = None, ratio: float = 0.25,
                  ndcg_cut: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-query statistics and predicted orders for lists described by `scope`.

    Returns (stats [Q, 12] float64 = top1 hit, predicted top-1 in target top-25%, recall@25%, NDCG1, NDCG2, NDCG25%,
             NDCG_all, NDCG@10(exp2), target top-1 in predicted top-`ratio`, calculate_ndcg's NDCG@`ndcg_cut`, KL,
             recall@`ratio`;
             order [M] int32 = within-list index of the candidate at each predicted rank)."""
    if scores.dim() > 1:
        scores = scores[:, 0]                              # eval.py:125-126, :390-394, :508-509
    scope, seg, total, max_len, t = _prep(scores, scope, targets, gpu)
    s = _vec(scores.detach())
    order = torch.empty(total, dtype=torch.int32, device=s.device)
    stats = torch.empty(len(scope), NSTATS, dtype=torch.float64, device=s.device)
    check(lib().rr_ranking_metrics_f32(ptr(s), s.stride(0), ptr(t), ptr(seg), len(scope), max_len, float(ratio),
                                       float(ndcg_cut), ptr(order), ptr(stats), stream()), "rr_ranking_metrics_f32")
    return stats, order


def _mean_stats(stats: torch.Tensor, exchange=None) -> np.ndarray:
    """Mean of the per-query statistics over every query - of every rank when `exchange` (reactranker_amd.dp.Exchange)
    spans a process group: each rank evaluated its own queries, the float64 column sums and the count are all-reduced."""
    if exchange is None or not exchange.on:
        return stats.mean(dim=0).cpu().numpy()
    v = torch.cat([stats.sum(dim=0), torch.tensor([float(stats.shape[0])], dtype=torch.float64, device=stats.device)])
    v = exchange.sum(v).cpu().numpy()
    return v[:-1] / max(v[-1], 1.0)


def ranking_metrics_from_scores(scores, scope, targets, gpu: int = None):
    """(top1, recall25, top25, NDCG_[NDCG1, NDCG2, NDCG25, NDCG_all]) as the reference's ranking_metrics returns
    them (eval.py:548-555)."""
    stats, _ = ranking_stats(scores, scope, targets, gpu)
    m = stats.mean(dim=0).cpu().numpy()
    return float(m[0]), float(m[2]), float(m[1]), m[3:7].copy()


def ranking_metrics(model, gpu, batches: Iterable, show_info: bool = False, exchange=None):
    """Evaluate `model` over an iterable of (r_batch, p_batch, scope, targets, add_features) batches of whole
    queries; same return value as the reference's ranking_metrics (which switches the model to eval mode, :487).
    exchange: a reactranker_amd.dp.Exchange when every rank evaluates its own shard of the validation queries."""
    was_training = model.training
    model.eval()
    stats, _ = _eval_stats(model, gpu, batches)
    model.train(was_training)
    m = _mean_stats(stats, exchange)
    return float(m[0]), float(m[2]), float(m[1]), m[3:7].copy()


def _eval_stats(model, gpu, batches, ratio=0.25, ndcg_cut=0.5, transform=None, keep_mode=False):
    """Score every batch of whole queries with `model` and rank it on the device: (stats [Q_total, 12], list of
    (scores, order, scope, targets) per batch).  The mode of `model` is left as the caller set it (the reference's
    evaluate_top_scores / calculate_ndcg do not call model.eval(): eval.py:83-84, :337-338)."""
    rows, per_batch = [], []
    with torch.no_grad():
        for r_batch, p_batch, scope, targets, add_features in batches:
            if len(scope) == 0:                              # an empty shard of a data-parallel evaluation
                continue
            out = model(r_batch, p_batch, gpu=gpu, add_features=add_features)
            if transform is not None:
                out = transform(out)
            stats, order = ranking_stats(out, scope, targets, gpu, ratio, ndcg_cut)
            rows.append(stats)
            per_batch.append((out, order, list(scope), targets))
    if not rows:
        dev = torch.device("cuda", torch.cuda.current_device() if gpu is None else gpu)
        return torch.zeros(0, NSTATS, dtype=torch.float64, device=dev), per_batch
    return torch.cat(rows, 0), per_batch


def top_scores_from_scores(scores, scope, targets, gpu: int = None, ratio: float = 0.25):
    """(average_score, average_pred_in_targ, average_top1_in_pred) of evaluate_top_scores (eval.py:172-177) for one
    batch of scored lists."""
    stats, _ = ranking_stats(scores, scope, targets, gpu, ratio)
    m = stats.mean(dim=0).cpu().numpy()
    return float(m[0]), float(m[11]), float(m[8])


def evaluate_top_scores(model, gpu, batches: Iterable, ratio: float = 0.25, show_info=False, exchange=None):
    """Reference evaluate_top_scores (train/eval.py:76-177) over an iterable of (r_batch, p_batch, scope, targets,
    add_features) batches of whole queries: returns (average_score = top-1 by first maximum, average_pred_in_targ =
    share of the predicted top-`ratio` inside the target top-`ratio`, average_top1_in_pred = the TARGET's top-1 inside
    the predicted top-`ratio`).  This - not ranking_metrics - is what the RankNet epoch driver validates with
    (run_train_pairwise.py:91-96) and what both test() functions report (test_listwise.py:51-54, test_ranknet.py:59)."""
    stats, _ = _eval_stats(model, gpu, batches, ratio=ratio)
    m = _mean_stats(stats, exchange)
    return float(m[0]), float(m[11]), float(m[8])


def calculate_ndcg(model, gpu, batches: Iterable, NDCG_cut: float = 0.5, is_order: bool = True, means=None, stds=None,
                   show_info=False, exchange=None):
    """Reference calculate_ndcg (train/eval.py:329-457): (NDCG_mean, KL_mean, total_order, None).

    `means` / `stds` de-standardise the model output first (:379-388: mean column * std + mean, variance column *
    std^2).  With is_order, `total_order` holds one row per candidate, queries in input order and candidates in TARGET
    order: [target, prediction, (uncertainty,) true rank, predicted rank] (:406-420); without it the raw
    [target, prediction...] rows (:444-449) and NDCG / KL are None.  The reference's fourth value (the SMILES of every
    row, :427-437) belongs to the DataFrame side and is returned as None."""
    def destd(out):
        if means is None:
            return out
        if out.dim() > 1:                                   # :380-386
            scale = torch.ones(out.size(1), dtype=out.dtype, device=out.device)
            shift = torch.zeros_like(scale)
            scale[0], shift[0] = float(stds), float(means)
            if out.size(1) > 1:
                scale[1] = float(stds) ** 2
            return out * scale + shift
        return out * float(stds) + float(means)

    stats, per_batch = _eval_stats(model, gpu, batches, ndcg_cut=NDCG_cut, transform=destd)
    total_order = []
    for out, order, scope, targets in per_batch:
        o = out.detach().cpu()
        t = torch.as_tensor(np.asarray(targets), dtype=torch.float32).reshape(-1)
        if not is_order:
            cols = o.reshape(o.size(0), -1)
            total_order.extend([[float(a)] + [float(x) for x in b] if o.dim() > 1 else [float(a), float(b[0])]
                                for a, b in zip(t.tolist(), cols.tolist())])
            continue
        pred = o[:, 0] if o.dim() > 1 else o
        off = 0
        for c in scope:                                      # the listing only (host bookkeeping, :406-420)
            bt, bp = t[off:off + c], pred[off:off + c]
            idx = torch.sort(bt, descending=True, stable=True)[1]
            sp = bp[idx]
            pred_order = torch.argsort(torch.argsort(sp, descending=True, stable=True), stable=True) + 1
            cols = [bt[idx], sp]
            if o.dim() > 1:
                cols.append(o[off:off + c, 1][idx])
            cols += [torch.arange(1, c + 1, dtype=torch.float32), pred_order.float()]
            total_order.extend(torch.stack(cols, dim=1).tolist())
            off += c
    if not is_order:
        return None, None, total_order, None
    m = _mean_stats(stats, exchange)         # (the listing stays this rank's own queries)
    return float(m[9]), float(m[10]), total_order, None


def calculate_mse(model, gpu, batches: Iterable, exchange=None) -> float:
    """Reference calculate_mse (train/eval.py:558-609; the `save_metric='mse'` criterion of train_listwise.py:345-351):
    switches the model to eval mode and returns the mean squared error between the first output column and the targets
    of the LAST batch - the reference overwrites its `MSE` in every iteration of the loop and returns the final one (:607-609),
    which is kept.  Data parallel: the last global batch's squared errors and count are summed over the ranks."""
    from .loss import MSELoss
    model.eval()
    last = None
    with torch.no_grad():
        for r_batch, p_batch, scope, targets, add_features in batches:
            last = (r_batch, p_batch, scope, targets, add_features)
        dev = torch.device("cuda", torch.cuda.current_device() if gpu is None else gpu)
        v = torch.zeros(2, dtype=torch.float64, device=dev)                 # [sum of squared errors, count]
        if last is not None and len(last[2]) > 0:
            out = model(last[0], last[1], gpu=gpu, add_features=last[4])
            pred = out[:, 0] if out.dim() > 1 else out
            t = torch.as_tensor(last[3], dtype=torch.float32).reshape(-1)
            n = int(pred.shape[0])
            v[0] = MSELoss()(pred.contiguous(), t).double().sum() * n      # rr_mse_fwd_f32: the mean over this shard
            v[1] = n
        if exchange is not None and exchange.on:
            v = exchange.sum(v)
    return float(v[0] / v[1].clamp(min=1.0))


# ------------------------------------------------------------------------------------------------ rank correlation
def rank_correlation_stats(scores: torch.Tensor, scope, targets, gpu: int = None) -> torch.Tensor:
    """rr_rank_correlation_f32 on one batch of scored lists: [Q, 8] float64 on the device = Kendall tau-b, Spearman rho (on
    tie-averaged ranks), reciprocal rank of the target's first maximum, top-1 regret, then the pair counts P (concordant),
    D (discordant), X (tied in score only), Y (tied in target only).  tau-b and rho are NaN where a key is constant; an empty
    list has NaN in the first four columns.  Column 0 of a 2-D output is read in place, by its stride."""
    if scores.dim() > 1:
        scores = scores[:, 0]
    scope, seg, total, max_len, t = _prep(scores, scope, targets, gpu)
    s = _vec(scores.detach())
    stats = torch.empty(len(scope), RANK_CORR_NSTATS, dtype=torch.float64, device=s.device)
    check(lib().rr_rank_correlation_f32(ptr(s), s.stride(0), ptr(t), ptr(seg), len(scope), max_len, ptr(stats), stream()),
          "rr_rank_correlation_f32")
    return stats


def _nanmean_stats(stats: torch.Tensor, exchange=None):
    """Per column of the [Q, 8] rank-correlation statistics: (sums [8] of the entries that are not NaN, counts [8] of those
    entries), float64 numpy arrays - summed over every rank when `exchange` (reactranker_amd.dp.Exchange) spans a process
    group.  Columns 0..3 are means once divided (sums / counts, NaN where the count is 0); columns 4..7, the pair counts, are
    used as plain sums."""
    n = stats.shape[1]
    ok = ~torch.isnan(stats)
    v = torch.cat([torch.where(ok, stats, torch.zeros_like(stats)).sum(dim=0), ok.to(torch.float64).sum(dim=0)])
    if exchange is not None and exchange.on:
        v = exchange.sum(v)
    v = v.cpu().numpy()
    return v[:n].copy(), v[n:].copy()


def _rank_correlation_dict(sums: np.ndarray, counts: np.ndarray) -> dict:
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(counts[:4] > 0, sums[:4] / np.maximum(counts[:4], 1.0), np.nan)
        P, D, X, Y = (float(x) for x in sums[4:8])
        den = (P + D + X) * (P + D + Y)
        pooled = (P - D) / np.sqrt(den) if den > 0 else float("nan")
    return dict(kendall_tau=float(mean[0]), spearman=float(mean[1]), mrr=float(mean[2]), regret=float(mean[3]),
                n_defined=int(counts[0]), kendall_tau_pooled=float(pooled), pairs=[P, D, X, Y])


def rank_correlation_from_scores(scores, scope, targets, gpu: int = None) -> dict:
    """The rank agreement of one batch of scored lists with their targets: {kendall_tau, spearman, mrr, regret: means over
    the queries where each is defined (NaN when there is none); n_defined: the number of queries behind kendall_tau;
    kendall_tau_pooled: tau-b of the pair counts summed over all queries, (P - D) / sqrt((P + D + X) (P + D + Y));
    pairs: those four sums [P, D, X, Y]}."""
    return _rank_correlation_dict(*_nanmean_stats(rank_correlation_stats(scores, scope, targets, gpu)))


def rank_correlation(model, gpu, batches: Iterable, exchange=None) -> dict:
    """rank_correlation_from_scores over an iterable of (r_batch, p_batch, scope, targets, add_features) batches of whole
    queries scored by `model`; switches the model to eval mode and restores the caller's mode, as ranking_metrics does.
    exchange: a reactranker_amd.dp.Exchange when every rank evaluates its own shard of the queries (an empty shard is
    skipped; the sums and counts are all-reduced).  The means are NaN when no query is defined anywhere."""
    was_training = model.training
    model.eval()
    rows = []
    with torch.no_grad():
        for r_batch, p_batch, scope, targets, add_features in batches:
            if len(scope) == 0:
                continue
            out = model(r_batch, p_batch, gpu=gpu, add_features=add_features)
            rows.append(rank_correlation_stats(out, scope, targets, gpu))
    model.train(was_training)
    if rows:
        stats = torch.cat(rows, 0)
    else:
        dev = torch.device("cuda", torch.cuda.current_device() if gpu is None else gpu)
        stats = torch.zeros(0, RANK_CORR_NSTATS, dtype=torch.float64, device=dev)
    return _rank_correlation_dict(*_nanmean_stats(stats, exchange))


def ndcg_at_k(scores, scope, relevance, gpu: int = None) -> np.ndarray:
    """metrics.NDCG(k=10, 'exp2') of every query: `relevance` are the grades, ranked by `scores`."""
    stats, _ = ranking_stats(scores, scope, relevance, gpu)
    return stats[:, 7].cpu().numpy()


# ------------------------------------------------------------------------------------------------ pairwise evaluation
def pairwise_stats_from_scores(scores, scope, targets, sigma: float = 1.0, gpu: int = None):
    """rr_pairwise_eval_f32 on one batch of scored lists: (sums [4] float64 = {sum over the queries with at least one
    positive pair of 1 - mismatches / (2 npos), number of those queries, sum of the cross-entropy terms, their pair count},
    per_query [Q, 4] float64 = {npos, mismatches, cross-entropy sum, 0}), both on the device.  pairwise_acc = sums[0] /
    sums[1], eval_cross_entropy_loss = sums[2] / sums[3]."""
    if scores.dim() > 1:
        scores = scores[:, 0]                              # eval.py:208-209
    scope, seg, total, max_len, t = _prep(scores, scope, targets, gpu)
    s = _vec(scores.detach())
    per_query = torch.empty(max(len(scope), 1), 4, dtype=torch.float64, device=s.device)
    sums = torch.empty(4, dtype=torch.float64, device=s.device)
    check(lib().rr_pairwise_eval_f32(ptr(s), s.stride(0), ptr(t), ptr(seg), len(scope), max_len, float(sigma), ptr(per_query),
                                     ptr(sums), stream()), "rr_pairwise_eval_f32")
    return sums, per_query[:len(scope)]


def _pairwise_sums(model, gpu, batches, sigma, exchange):
    dev = torch.device("cuda", torch.cuda.current_device() if gpu is None else gpu)
    tot = torch.zeros(4, dtype=torch.float64, device=dev)
    with torch.no_grad():
        for r_batch, p_batch, scope, targets, add_features in batches:
            if len(scope) == 0:
                continue
            out = model(r_batch, p_batch, gpu=gpu, add_features=add_features)
            tot += pairwise_stats_from_scores(out, scope, targets, sigma, gpu)[0]
    if exchange is not None and exchange.on:
        tot = exchange.sum(tot)
    return tot.cpu().numpy()


def pairwise_acc(model, gpu, batches: Iterable, show_info: bool = False, exchange=None) -> float:
    """Reference pairwise_acc (train/eval.py:180-224) over (r_batch, p_batch, scope, targets, add_features) batches of whole
    queries: per query 1 - sum_ij |[s_i > s_j] - [t_i > t_j]| / (2 #{t_i > t_j}), queries without a positive pair skipped, mean
    over the rest (NaN when none is left, as np.mean of an empty list).  Switches the model to eval mode like the reference."""
    model.eval()
    v = _pairwise_sums(model, gpu, batches, 1.0, exchange)
    return float(v[0] / v[1]) if v[1] > 0 else float("nan")


def eval_cross_entropy_loss(model, gpu, batches: Iterable, sigma: float = 1.0, exchange=None) -> float:
    """Reference eval_cross_entropy_loss (train/eval.py:15-73): over all queries the sum over the pairs with t_i != t_j of
    0.5 (1 - S_ij) sigma (s_i - s_j) - logsigmoid(-sigma (s_i - s_j)), divided by their count - the code as written (its
    docstring states the opposite sign).  The score differences are those of a [C, 1] prediction; with the squeezed [C]
    output of a task_num = 1 model the reference's `y_pred - y_pred.t()` is zero and it returns ln 2."""
    model.eval()
    v = _pairwise_sums(model, gpu, batches, sigma, exchange)
    return float(v[2] / v[3]) if v[3] > 0 else float("nan")


def pair_acc_from_outputs(y_pred, targets) -> torch.Tensor:
    """rr_pair_acc_f32: 1 - mean_b |[y_b0 > y_b1] - [tp_b0 > tp_b1]| with tp = softmax of the pair's targets (eval.py:246-264);
    a [1] float32 device tensor."""
    from .loss import _pair_rows
    _lib.require_cuda(y_pred, "y_pred")
    y = _pair_rows(y_pred.detach(), "y_pred")
    t = _pair_rows(targets, "targets", y.device)
    if t.shape[0] != y.shape[0] or y.shape[0] < 1:
        raise RuntimeError("pair_acc_from_outputs: y_pred and targets must hold the same, non-zero number of pairs")
    acc = torch.empty(1, dtype=torch.float32, device=y.device)
    check(lib().rr_pair_acc_f32(ptr(y), y.stride(0), ptr(t), t.stride(0), y.shape[0], ptr(acc), stream()), "rr_pair_acc_f32")
    return acc


def pairwise_baseline_acc(model, gpu, pair_batches: Iterable, show_info: bool = False) -> float:
    """Reference pairwise_baseline_acc (train/eval.py:226-273) over pair batches (reactranker_amd.pairs.pair_windows): the
    accuracy of every batch, the last short one included, then the mean over the batches.  In eval mode the pair model
    encodes every distinct molecule of a batch once (reactranker_amd.ranknet_baseline)."""
    model.eval()
    accs = []
    with torch.no_grad():
        for b in pair_batches:
            if len(b["targets"]) == 0:
                continue
            y = model(b["r"], b["p1"], b["p2"], gpu=gpu, pair_index=b.get("index"))
            accs.append(pair_acc_from_outputs(y, b["targets"]))
    return float(torch.cat(accs).double().mean()) if accs else float("nan")
