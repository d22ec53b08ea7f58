"""Pairwise epoch driver on pre-packed windows of whole queries: `run_train` of the reference
(reactranker/train/run_train_pairwise.py:18-140) with its five selectors (:66-90): train_strategy 'sum_session' /
'accelerate_grad' (RankNet, what main_ranknet.py uses) and 'baseline' (the pair model of reactranker_amd.ranknet_baseline)
under task_type 'baseline', and task_type 'BetaNet' / 'BetaNet_envidential'.  Standardises the targets like the reference (:36-45: z-score with the training
set's statistics, sign flipped unless the target is 'lgk'), runs `factorized_training_loop` per epoch, evaluates on the
validation windows with `evaluate_top_scores` (:91-96) and checkpoints on the selected metric (:97-117).  The DataFrame / SMILES side stays the reference's."""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from .eval import evaluate_top_scores, pairwise_baseline_acc, rank_correlation
from .pairs import pair_windows
from .train_listwise import RANK_CORR_METRICS, standardize_batches
from .train_pairwise import (baseline_pairwise_training_loop, beta_dis_train_loop, beta_evi_train_loop,
                             factorized_training_loop)
from .utils import save_checkpoint


def standardize_pairwise(train_targets, val_targets, target_name: str = "ea"):
    """run_train_pairwise.py:36-45: z-score with the training mean / population std; every target except 'lgk' flips sign."""
    tr, va = np.asarray(train_targets, np.float64), np.asarray(val_targets, np.float64)
    mean, std = float(tr.mean()), float(tr.std())
    sign = 1.0 if target_name == "lgk" else -1.0
    return sign * (tr - mean) / std, sign * (va - mean) / std, mean, std


def run_train(model: torch.nn.Module, scheduler, train_batches: Sequence, val_batches: Sequence,
              path_checkpoints: Union[str, List[str], None], optimizer, epochs: int, seed: int, gpu: int,
              train_strategy: str = "sum_session", task_type: str = "baseline", logger=None,
              target_name: Optional[str] = "ea", save_metric: Optional[str] = None, sigma: float = 1.0, epoch_hook=None,
              group=None, batch_size: int = 1000, val_batch_size: int = 500, ndcg_k: int = 0, temperature: float = 1.0):
    """Selectors as in the reference (:66-90): task_type 'BetaNet' -> beta_dis_train_loop (alpha0 = 100), 'BetaNet_envidential' ->
    beta_evi_train_loop (max_coeff = 0.01; needs epochs >= 2 and a positive head), otherwise task_type 'baseline' with
    train_strategy 'sum_session' / 'accelerate_grad' -> factorized_training_loop or 'baseline' -> the pair model's
    baseline_pairwise_training_loop.  train_strategy 'lambdarank' (task_type 'baseline'; not in the reference) runs
    factorized_training_loop on the NDCG-weighted pair loss, truncated at `ndcg_k` positions (0: the whole list);
    train_strategy 'approx_ndcg' (likewise) runs it on ApproxNDCG, one minus the NDCG at `ndcg_k` on soft ranks of
    `temperature` (score units).  Anything else is a ValueError.

    train_strategy 'baseline': `model` is a reactranker_amd.ranknet_baseline model and every window also carries `mols_r` /
    `mols_p`, the reactant / product graph of each candidate; after the targets are standardised the pairs of all training
    windows are cut into batches of `batch_size` (the short last one is skipped, train_pairwise.py:24) and those of the
    validation windows into batches of `val_batch_size` (:103: 500).  Validation is pairwise_baseline_acc and the checkpoint is
    written when it does not fall (:125-127); the history then holds {epoch, train_loss, acc, checkpoint}.

    Otherwise returns the per-epoch history [{epoch, train_loss, top1, pred_top25_in_targ_top25, top1_in_pred_top25 (the TARGET's
    top-1 inside the predicted top-25 %), checkpoint, checkpoint_all (which of the three 'all' metrics improved)}].
    epoch_hook(epoch, model, record): optional observer called after every epoch's validation (not in the reference).
    save_metric 'kendall_tau' / 'spearman' / 'mrr' (not in the reference) select on that mean of eval.rank_correlation, as in
    reactranker_amd.train_listwise.train: the record then also holds its dict under `rank_correlation`.
    group: data-parallel training under torch.distributed exactly as in reactranker_amd.train_listwise.train - every rank
    passes its shard of every window (whole queries, each batch carrying the window's `global` counts) and of the
    validation queries; the loss is normalised by the WINDOW's ordered pairs, gradients are summed over the ranks,
    validation statistics likewise, rank 0 writes the checkpoints (main_ranknet.py:143-160 is the single-process driver)."""
    from .dp import Exchange
    selector = select_loop(train_strategy, task_type)
    if selector == "BetaNet_envidential" and epochs < 2:
        raise ValueError("task_type 'BetaNet_envidential' needs epochs >= 2: its annealing coefficient divides by epochs - 1 "
                         "(reference train_pairwise.py:308 raises ZeroDivisionError)")
    if gpu is not None:
        torch.cuda.set_device(gpu)
    model = model.cuda(gpu)
    ex = Exchange(model, group)
    try:
        if selector == "pair_baseline":
            return _run_train_pairs(model, scheduler, train_batches, val_batches, path_checkpoints, optimizer, epochs, gpu,
                                    logger, target_name, epoch_hook, ex, batch_size, val_batch_size)
        return _run_train(model, scheduler, train_batches, val_batches, path_checkpoints, optimizer, epochs, gpu, selector,
                          logger, target_name, save_metric, sigma, epoch_hook, ex, ndcg_k, temperature)
    finally:
        ex.close()


def select_loop(train_strategy: str, task_type: str) -> str:
    """The reference's if / elif chain (:66-90) as one name: 'pair_baseline', 'sum_session', 'accelerate_grad', 'BetaNet' or
    'BetaNet_envidential' - and 'lambdarank' and 'approx_ndcg', this library's additions; ValueError for anything the
    reference's chain would fall through."""
    if task_type == "baseline" and train_strategy == "baseline":
        return "pair_baseline"
    if task_type == "baseline" and train_strategy in ("sum_session", "accelerate_grad", "lambdarank", "approx_ndcg"):
        return train_strategy
    if task_type in ("BetaNet", "BetaNet_envidential"):
        return task_type
    raise ValueError("reactranker_amd covers the reference's pairwise selectors: train_strategy 'baseline' / 'sum_session' / "
                     "'accelerate_grad' (and its own 'lambdarank' / 'approx_ndcg') with task_type 'baseline', or task_type 'BetaNet' / "
                     "'BetaNet_envidential' "
                     f"(got train_strategy {train_strategy!r}, task_type {task_type!r})")


def _all_pairs(windows, batch_size):
    mols_r, mols_p, scope, targets = [], [], [], []
    for b in windows:
        if "mols_r" not in b or "mols_p" not in b:
            raise ValueError("train_strategy 'baseline' needs `mols_r` and `mols_p` (one graph per candidate) in every window")
        mols_r += list(b["mols_r"])
        mols_p += list(b["mols_p"])
        scope += [int(c) for c in b["scope"]]
        targets.append(np.asarray(torch.as_tensor(b["targets"]).cpu(), np.float32).reshape(-1))
    t = np.concatenate(targets) if targets else np.zeros(0, np.float32)
    return list(pair_windows(mols_r, mols_p, scope, t, batch_size))


def _run_train_pairs(model, scheduler, train_batches, val_batches, path_checkpoints, optimizer, epochs, gpu, logger, target_name,
                     epoch_hook, ex, batch_size, val_batch_size):
    mean, std = 0.0, 1.0
    if target_name is not None:
        tn = "lgk" if target_name == "lgk" else "ea"
        train_batches, val_batches, mean, std = standardize_batches(list(train_batches), list(val_batches), tn, True, None, ex)
    train_pairs = _all_pairs(train_batches, batch_size)
    val_pairs = _all_pairs(val_batches, val_batch_size)
    ex.broadcast_model(model)
    ex.check_same_steps(sum(1 for b in train_pairs if b["full"]), next(model.parameters()).device)
    say = logger.info if (logger is not None and ex.is_writer) else (lambda *_: None)
    score_old, history = 0.0, []
    for epoch in range(epochs):
        say("learning rate is: {}".format(optimizer.param_groups[0]["lr"]))
        model.zero_grad()
        model.train()
        epoch_loss = baseline_pairwise_training_loop(epoch, epochs, model, optimizer, scheduler, train_pairs,
                                                     batch_size=batch_size, max_coeff=0.001, gpu=gpu, exchange=ex)
        acc = pairwise_baseline_acc(model, gpu, val_pairs)
        saved = False
        if acc >= score_old:                                  # :125-127
            score_old = acc
            if path_checkpoints is not None:
                saved = True
                if ex.is_writer:
                    save_checkpoint(path_checkpoints, model, mean, std)
        history.append(dict(epoch=epoch + 1, train_loss=float(epoch_loss), acc=float(acc), checkpoint=saved))
        if epoch_hook is not None:
            epoch_hook(epoch, model, history[-1])
        say("Epoch [{}/{}],train_loss,{:.4f}, acc,{:.4f}".format(epoch + 1, epochs, epoch_loss, acc))
    return history


def _run_train(model, scheduler, train_batches, val_batches, path_checkpoints, optimizer, epochs, gpu, train_strategy, logger,
               target_name, save_metric, sigma, epoch_hook, ex, ndcg_k=0, temperature=1.0):
    mean, std = 0.0, 1.0
    if target_name is not None:
        # same statistics as the listwise trainer's default branch: z-score, sign flipped unless 'lgk' (:39-44)
        tn = "lgk" if target_name == "lgk" else "ea"
        train_batches, val_batches, mean, std = standardize_batches(list(train_batches), list(val_batches), tn, True, None, ex)
    ex.broadcast_model(model)
    ex.check_same_steps(len(train_batches), next(model.parameters()).device)
    score_old = [0.0, 0.0, 0.0] if save_metric == "all" else (float("-inf") if save_metric in RANK_CORR_METRICS else 0.0)
    say = logger.info if (logger is not None and ex.is_writer) else (lambda *_: None)
    history = []
    for epoch in range(epochs):
        say("learning rate is: {}".format(optimizer.param_groups[0]["lr"]))
        model.zero_grad()
        model.train()
        if train_strategy == "BetaNet":                       # :78-82
            epoch_loss = beta_dis_train_loop(epoch, model, optimizer, scheduler, train_batches, alpha0=100, gpu=gpu, exchange=ex)
        elif train_strategy == "BetaNet_envidential":         # :83-88
            epoch_loss = beta_evi_train_loop(epoch, model, optimizer, scheduler, train_batches, max_coeff=0.01, epochs=epochs,
                                             gpu=gpu, exchange=ex)
        else:
            epoch_loss = factorized_training_loop(epoch, model, optimizer, scheduler, train_batches, sigma=sigma,
                                                  training_algo=train_strategy, gpu=gpu, exchange=ex, ndcg_k=ndcg_k,
                                                  temperature=temperature)
        model.eval()
        with torch.no_grad():
            # evaluate_top_scores, not ranking_metrics (:91-96): its third value is the TARGET's top-1 inside the
            # predicted top-25 % (eval.py:156-159)
            top1, recall25, top25 = evaluate_top_scores(
                model, gpu, [(b["r"], b["p"], b["scope"], b["targets"], b.get("add")) for b in val_batches], ratio=0.25,
                exchange=ex)
        saved = False
        saved_which = [False, False, False]                  # save_metric='all': T1 / T25_in_T25 / T25 (main_ranknet.py:68-74)

        def keep(path, which=0):
            nonlocal saved
            saved_which[which] = True
            if path is not None:
                saved = True
                if ex.is_writer:
                    save_checkpoint(path, model, mean, std)
        if save_metric is None or save_metric == "average_score":
            if top1 >= score_old:
                score_old = top1
                keep(path_checkpoints)
        elif save_metric == "all":
            for i, v in enumerate((top1, recall25, top25)):
                if v >= score_old[i]:
                    score_old[i] = v
                    keep(path_checkpoints[i] if path_checkpoints is not None else None, i)
        elif save_metric in RANK_CORR_METRICS:
            corr = rank_correlation(model, gpu, [(b["r"], b["p"], b["scope"], b["targets"], b.get("add")) for b in val_batches],
                                    exchange=ex)
            if corr[save_metric] >= score_old:                # False for a NaN: it never replaces the best and never saves
                score_old = corr[save_metric]
                keep(path_checkpoints)
        else:
            raise Exception("Unknown save metric")
        history.append(dict(epoch=epoch + 1, train_loss=float(epoch_loss), top1=float(top1),
                            pred_top25_in_targ_top25=float(recall25), top1_in_pred_top25=float(top25), checkpoint=saved,
                            checkpoint_all=list(saved_which)))
        if save_metric in RANK_CORR_METRICS:
            history[-1]["rank_correlation"] = corr
        if epoch_hook is not None:
            epoch_hook(epoch, model, history[-1])
        say("Epoch [{}/{}],train_loss,{:.4f}, average_score_top1,{:.4f}, average_pred_in_targ_top25%,{:.4f}"
            .format(epoch + 1, epochs, epoch_loss, top1, top25))
    return history
