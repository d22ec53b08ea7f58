"""The pairwise trainer's loops on pre-packed windows (reference reactranker/train/train_pairwise.py): RankNet's
`factorized_training_loop` (:81-173), the two Beta loops `beta_dis_train_loop` (:176-262) and `beta_evi_train_loop` (:263-338),
and the pair model's `baseline_pairwise_training_loop` (:6-78).

RankNet training loop on pre-packed windows of whole queries: `factorized_training_loop` of the reference
(reactranker/train/train_pairwise.py:81-173).  The reference runs one forward per query and accumulates loss /
lambdas until `batch_size` candidates have been seen (:141-160); here a batch already IS such a window (its queries
are scored in one forward, reactranker_amd.loss.ranknet_loss / ranknet_lambda handle every query of the window), so
one batch = one optimizer step with the same normalisation (loss / ordered pairs of the window).

A batch is a mapping with keys  r, p (BatchMolGraph), scope (list[int]), targets (float32 [M]), add (ndarray or None).
"""
from __future__ import annotations

from typing import Iterable

import torch

from .loss import (annealing_coef, approx_ndcg_loss, backward as loss_backward, beta_evidential_loss, betanet_loss,
                   lambdarank_loss, pair_softmax_mse, ranknet_lambda, ranknet_loss, sq_pairs)


def _run_epoch(model, optimizer, scheduler, batches, exchange, plan, step, rank_mean: bool = False) -> float:
    """The epoch skeleton of the four loops; returns the mean of the per-step losses (NaN when no batch made a step, as
    np.mean of an empty list).  A loop supplies its decision per batch in two parts, around the zero_grad:
      plan(b, ex, dev)  None - the window is skipped - or whatever `step` needs (the window's normaliser);
      step(b, planned)  forward and backward; returns the [1] loss, or None when this rank's shard holds nothing: zero
                        gradient, and a zero loss is recorded.
    rank_mean: the gradient and the reported loss are the MEAN over the ranks (each rank normalised by its own count),
    otherwise the plain sum (every rank normalised by the WINDOW's count already).
    The per-step losses stay on the device until the epoch ends: no host synchronisation per step."""
    from .dp import Exchange
    own_exchange = exchange is None
    ex = exchange if exchange is not None else Exchange(model)   # (under torch.distributed it owns the gradient bucket)
    dev = next(model.parameters()).device
    minibatch_loss = []
    for b in batches:
        planned = plan(b, ex, dev)
        if planned is None:
            continue
        model.zero_grad()
        loss = step(b, planned)
        minibatch_loss.append(torch.zeros(1, device=dev) if loss is None else loss)
        ex.reduce_grads(1.0 / ex.world if rank_mean else 1.0)
        optimizer.step()
        scheduler.step()
    model.zero_grad()
    if own_exchange:
        ex.close()
    if not minibatch_loss:
        return float("nan")
    per_step = ex.sum(torch.cat(minibatch_loss).double())
    if rank_mean:
        per_step = per_step / ex.world
    return float(per_step.mean())


def factorized_training_loop(epoch: int, model, optimizer, scheduler, batches: Iterable, sigma: float = 1.0,
                             training_algo: str = "sum_session", gpu: int = 0, exchange=None, ndcg_k: int = 0,
                             temperature: float = 1.0) -> float:
    """One epoch; returns the mean of the per-step losses like the reference (:173).
    training_algo: 'sum_session' (autograd through the pair losses, :117-122,147-148), 'accelerate_grad'
    (closed-form lambdas pushed through y_pred.backward, :123-137,149-151) or 'lambdarank' (not in the reference: the pair
    costs of 'sum_session' weighted by |delta NDCG| truncated at `ndcg_k` positions, 0 = the whole list -
    reactranker_amd.loss.lambdarank_loss; loss and gradient come from one launch) or 'approx_ndcg' (not in the reference
    either: one minus the NDCG at `ndcg_k` written on soft ranks of `temperature`, in score units -
    reactranker_amd.loss.approx_ndcg_loss; one launch as well, normalised by the window's QUERY count).

    The window's ordered-pair count - the loss's normaliser (:106,147) and the reason a window is skipped (:101-103) - is
    counted on the host from the targets the batch carries (dp.count_pairs, cached on the batch), and the per-step losses
    stay on the device until the epoch ends: no host synchronisation per step (the reference reads `.item()` per query).
    exchange: a reactranker_amd.dp.Exchange; a batch is then this rank's shard of the window and the normaliser is the
    whole window's pair count."""
    from .dp import step_counts
    if training_algo not in ("sum_session", "accelerate_grad", "lambdarank", "approx_ndcg"):
        raise ValueError("training algo {} not implemented".format(training_algo))

    def plan(b, ex, dev):
        if "_counts" not in b:
            b["_counts"] = step_counts(b["scope"], b["targets"]) if len(b["scope"]) else dict(queries=0, cands=0, pairs=0)
        local = b["_counts"]
        glob = ex.counts(b, dev)[1] if ex.on else local
        # windows without any ordered pair carry no information (:101-103)
        return (local, glob) if glob["pairs"] > 0 else None

    def step(b, planned):
        local, glob = planned
        pairs = glob["pairs"]
        if local["pairs"] == 0:                          # this rank's shard has no ordered pair
            return None
        y_pred = model(b["r"], b["p"], gpu=gpu, add_features=b.get("add"))
        if y_pred.dim() > 1:
            y_pred = y_pred[:, 0]
        if training_algo == "lambdarank":
            loss, _ = lambdarank_loss(y_pred, b["scope"], b["targets"], sigma, ndcg_k, gpu, pairs=pairs)
            loss_backward(loss)
        elif training_algo == "approx_ndcg":
            loss, _ = approx_ndcg_loss(y_pred, b["scope"], b["targets"], temperature, ndcg_k, gpu, queries=glob["queries"])
            loss_backward(loss)
        else:
            loss_sum, _ = ranknet_loss(y_pred if training_algo == "sum_session" else y_pred.detach(), b["scope"],
                                       b["targets"], sigma, gpu)
            loss = loss_sum / pairs
            if training_algo == "sum_session":
                loss_backward(loss)
            else:
                back = ranknet_lambda(y_pred, b["scope"], b["targets"], sigma, gpu)
                y_pred.backward(back / pairs)
        return loss.detach().sum().reshape(1)

    return _run_epoch(model, optimizer, scheduler, batches, exchange, plan, step)


def window_sq_pairs(batch, exchange, device) -> tuple:
    """(this shard's, the whole window's) sum of C * C - C: the normaliser of the two Beta loops (:198, :230).  Counted from
    `scope` on the host.  Under an active Exchange the window total is the `sq_pairs` entry of the batch's `global` counts
    when it is there, otherwise one all-reduce - cached on the batch either way."""
    if "_sq_pairs" not in batch:
        local = sq_pairs(batch["scope"])
        glob = local
        if exchange is not None and exchange.on:
            g = (batch.get("global") or {}).get("sq_pairs")
            if g is None:
                g = int(exchange.sum(torch.tensor([float(local)], dtype=torch.float64, device=device)).item())
            glob = int(g)
        batch["_sq_pairs"] = (local, glob)
    return batch["_sq_pairs"]


def _sq_pair_loop(loss_of, model, optimizer, scheduler, batches, gpu, exchange) -> float:
    def plan(b, ex, dev):
        pairs = window_sq_pairs(b, ex, dev)[1]
        return pairs if pairs > 0 else None              # nothing to normalise by (the reference would divide by zero)

    def step(b, pairs):
        if len(b["scope"]) == 0:                         # an empty shard
            return None
        y_pred = model(b["r"], b["p"], gpu=gpu, add_features=b.get("add"))
        loss_sum, _ = loss_of(y_pred, b["scope"], b["targets"])
        loss = loss_sum / pairs
        loss_backward(loss)
        return loss.detach().sum().reshape(1)

    return _run_epoch(model, optimizer, scheduler, batches, exchange, plan, step)


def beta_dis_train_loop(epoch: int, model, optimizer, scheduler, batches: Iterable, alpha0: float = 100, gpu: int = 0,
                        exchange=None) -> float:
    """One epoch of `task_type='BetaNet'` (:176-262); returns the mean of the per-step losses (:262).

    The reference hard-codes "two queries per optimizer step" and its end-of-epoch flush raises AttributeError whenever a
    partial group remains (:254 calls .item() on a Python int).  Here, as in factorized_training_loop, a pre-packed window IS
    one optimizer step, normalised by the window's sum of C * C - C (:198, :230); a window whose count is 0 (only
    one-candidate queries) is skipped.  exchange: a reactranker_amd.dp.Exchange; a batch is then this rank's shard of the
    window and the normaliser is the whole window's count (window_sq_pairs)."""
    return _sq_pair_loop(lambda y, scope, t: betanet_loss(y, scope, t, alpha0, gpu), model, optimizer, scheduler, batches, gpu,
                         exchange)


def beta_evi_train_loop(epoch: int, model, optimizer, scheduler, batches: Iterable, max_coeff: float = 0.001,
                        epochs: int = 100, gpu: int = 0, exchange=None) -> float:
    """One epoch of `task_type='BetaNet_envidential'` (:263-338): the model's raw scores are the evidence, so it needs a
    positive head (ffn_last_layer 'evidential' / 'with_softplus'); the penalty is annealed with max_coeff * (epoch /
    (epochs - 1)) ** 3 (:308).  epochs == 1 is a ZeroDivisionError in the reference: a ValueError that says so here.
    Windows, normaliser and `exchange` as in beta_dis_train_loop."""
    if epochs == 1:
        raise ValueError("beta_evi_train_loop: epochs == 1 makes the annealing coefficient max_coeff * (epoch / (epochs - 1)) "
                         "** 3 a division by zero (reference train_pairwise.py:308); train for at least 2 epochs")
    coef = annealing_coef(max_coeff, epoch, epochs)
    return _sq_pair_loop(lambda y, scope, t: beta_evidential_loss(y, scope, t, coef, gpu), model, optimizer, scheduler, batches,
                         gpu, exchange)


def baseline_pairwise_training_loop(epoch: int, epochs: int, model, optimizer, scheduler, pair_batches: Iterable,
                                    batch_size: int = 1000, max_coeff: float = 0.01, gpu: int = 0, exchange=None) -> float:
    """One epoch of `train_strategy='baseline'` (:6-78) over pair batches (reactranker_amd.pairs.pair_windows): one optimizer
    step per batch of exactly `batch_size` pairs - shorter ones are skipped (:24) - on loss = mean_b sum_k (softmax(t_b)_k -
    y_bk / sum_k y_bk)^2 (:33-59; the loop's variance, KL and annealing terms never reach the loss, so `epochs` and
    `max_coeff` are accepted and unused).  Returns the mean of the per-step losses (NaN when no batch was whole, as np.mean of
    an empty list).  exchange: every rank holds its own pair batches of one global step and the same number of them; the
    gradient is the mean over the ranks."""
    def step(b, _):
        y_pred = model(b["r"], b["p1"], b["p2"], gpu=gpu)
        loss = pair_softmax_mse(y_pred, b["targets"])
        loss_backward(loss)
        return loss.detach().reshape(1)

    return _run_epoch(model, optimizer, scheduler, pair_batches, exchange,
                      lambda b, ex, dev: True if len(b["targets"]) >= batch_size else None, step, rank_mean=True)
