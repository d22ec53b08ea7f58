"""Listwise training loop on pre-packed batches: the loop body, loss dispatch, validation and checkpoint selection
of the reference trainer (reactranker/train/train_listwise.py:21-372) for every task type whose branch works there
(SUPPORTED_TASKS; not 'mle_dirichlet', which raises NameError in the reference).  The reference's DataFrame / SMILES plumbing (DataProcessor, Parsing_features: out of scope,
SURVEY.md section 2 row 17) is replaced by an iterable of batches; everything downstream of
`model(r_inputs, p_inputs, gpu=gpu, add_features=...)` keeps the reference's call shapes.

A batch is a mapping with keys  r, p (BatchMolGraph), scope (list[int]), targets (float32 [M]), add (ndarray [M,F] or
None) - what train_listwise.py:176-189 gets from generate_batch_reactions + parsing_reactions.
"""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional, Sequence, Union

import numpy as np
import torch

from . import loss as RL
from .eval import calculate_mse, rank_correlation, ranking_metrics
from .utils import save_checkpoint

NDCG_METRICS = ["NDCG@1", "NDCG@2", "NDCG@25%", "NDCG@all"]
RANK_CORR_METRICS = ("kendall_tau", "spearman", "mrr")     # not in the reference: eval.rank_correlation's scale-free means
SUPPORTED_TASKS = ("mle", "listnet", "evidential_ranking", "gauss_regression", "mle_gaussian", "listnet_gauss",
                   "mle_regression", "listnet_regression", "regression",
                   "mledis_gaussian", "listnetdis_gauss", "listnetdis_lognorm", "listnet_uq", "evidential", "mle_evidential",
                   "mledis_evidential", "listnet_evidential", "dirichlet_uq", "regression_exploss")


def standardize_targets(train_targets, val_targets, target_name: str = "ea", normalize_target=True, save_metric=None):
    """Target standardisation and sign flip of the reference trainer (train/train_listwise.py:66-122), on arrays.

    Activation energies ('ea' and every name other than 'lgk' / 'lgk_bi') rank the LOWEST value first, so their sign
    is flipped; 'lgk' keeps its sign, 'lgk_bi' is passed through.  `normalize_target`: True -> z-score with the
    training set's mean / population std (ddof=0); False -> sign only; a float f -> x * f / (max - min) of the
    training set; a string 'lo,hi' -> min-max onto [lo, hi].  With an NDCG save metric the validation targets stay
    raw (:117-120).  Returns (train_std, val_std, mean, std) - mean / std are what the checkpoint stores."""
    tr = np.asarray(train_targets, np.float64)
    va = np.asarray(val_targets, np.float64)
    mean, std = float(tr.mean()), float(tr.std())                 # pandas .std(ddof=0)
    if target_name == "lgk_bi":
        f = lambda x: x                                           # noqa: E731
    else:
        sign = 1.0 if target_name == "lgk" else -1.0
        if isinstance(normalize_target, float):
            mx, mn = tr.max(), tr.min()
            f = lambda x: sign * (x * normalize_target) / (mx - mn)                       # noqa: E731
        elif isinstance(normalize_target, str):
            mx, mn = tr.max(), tr.min()
            lo, hi = (int(v) for v in normalize_target.split(","))
            f = lambda x: sign * (x - mn) * (hi - lo) / (mx - mn) + lo                   # noqa: E731
        elif normalize_target:
            f = lambda x: sign * (x - mean) / std                                        # noqa: E731
        else:
            f = lambda x: sign * x                                                       # noqa: E731
    val_std = va if save_metric in NDCG_METRICS else f(va)
    return f(tr), val_std, mean, std


def standardize_batches(train_batches, val_batches, target_name="ea", normalize_target=True, save_metric=None, exchange=None):
    """standardize_targets over lists of packed batches: statistics from ALL training targets (the reference computes
    them on the training DataFrame), new batch dicts with standardised float32 `targets`.  With a data-parallel
    `exchange` the statistics are those of every rank's training targets (gathered in rank order), so each rank applies
    the transformation the single-process run applies."""
    def cat(bs):
        return np.concatenate([np.asarray(torch.as_tensor(b["targets"]).cpu(), np.float64).reshape(-1) for b in bs]) \
            if len(bs) else np.zeros(0)
    tr_local, va_local = cat(train_batches), cat(val_batches)
    if exchange is not None and exchange.on:
        import torch.distributed as dist
        parts = [None] * exchange.world
        dist.all_gather_object(parts, tr_local, group=exchange.group)
        tr_all, _, mean, std = standardize_targets(np.concatenate(parts), np.zeros(0), target_name, normalize_target, save_metric)
        lo = sum(len(q) for q in parts[:exchange.rank])
        tr = tr_all[lo:lo + len(tr_local)]
        # the validation transform uses the training statistics only: apply it to this rank's validation targets
        _, va, _, _ = standardize_targets(np.concatenate(parts), va_local, target_name, normalize_target, save_metric)
    else:
        tr, va, mean, std = standardize_targets(tr_local, va_local, target_name, normalize_target, save_metric)

    def split(bs, flat):
        out, off = [], 0
        for b in bs:
            n = int(torch.as_tensor(b["targets"]).numel())
            nb = dict(b)
            nb["targets"] = torch.tensor(flat[off:off + n], dtype=torch.float32)
            off += n
            out.append(nb)
        return out
    return split(train_batches, tr), split(val_batches, va), mean, std


def _loss_terms(task_type: str, output, scope, targets, gpu, epoch, epochs, max_coeff):
    """The terms of the loss the reference trainer forms for one batch (train_listwise.py:196-285), in the order of
    dp.TASK_TERMS[task_type]."""
    mle, listnet, evid, gauss, mse = RL.MLEloss(), RL.ListnetLoss(), RL.evidential_ranking(), RL.GaussDisLoss(), RL.MSELoss()
    if task_type == "mle":
        return [mle(output, scope, targets, gpu)]
    if task_type == "listnet":
        return [listnet(output, scope, targets, gpu)]
    if task_type == "evidential_ranking":
        return [evid(output, scope, targets, max_coeff, epoch, epochs, gpu)]
    if task_type == "gauss_regression":
        return [gauss(output[:, 0], output[:, 1], targets, gpu)]
    if task_type == "mle_gaussian":
        return [mle(output[:, 0], scope, targets, gpu), gauss(output[:, 0], output[:, 1], targets, gpu)]
    if task_type == "listnet_gauss":
        return [listnet(output[:, 0], scope, targets, gpu), gauss(output[:, 0], output[:, 1], targets, gpu)]
    if task_type == "mle_regression":
        return [mse(output, targets), mle(output, scope, targets, gpu)]
    if task_type == "listnet_regression":
        return [listnet(output, scope, targets, gpu), mse(output, targets)]
    if task_type == "regression":                       # the reference's default branch: nn.MSELoss
        return [mse(output, targets)]
    if task_type == "mledis_gaussian":                  # the odd columns are log(variance) (:196-202)
        return [RL.MLEDisLoss()(output[:, 0::2], torch.exp(output[:, 1::2]), scope, targets, gpu),
                gauss(output[:, 0], output[:, 1], targets, gpu)]
    if task_type == "listnetdis_gauss":
        return [RL.Listnet_For_Gauss()(output[:, 0::2], output[:, 1::2], scope, targets, gpu),
                gauss(output[:, 0], output[:, 1], targets, gpu)]
    if task_type == "listnetdis_lognorm":               # its ListNet term is commented out in the reference (:215-219)
        return [RL.Lognorm()(output[:, 0], output[:, 1], targets, gpu)]
    if task_type == "listnet_uq":
        return [RL.Listnet_with_uq()(output, scope, targets, max_coeff, epoch, epochs, gpu)]
    if task_type == "dirichlet_uq":
        return [RL.Dirichlet_uq()(output, scope, targets, max_coeff, epoch, epochs, gpu)]
    if task_type == "regression_exploss":               # an inline expression there (:274-279)
        return [RL.ExpMSELoss()(output, targets)]
    if task_type in ("evidential", "mle_evidential", "mledis_evidential", "listnet_evidential"):
        # NIG columns mu, v, alpha, beta of the [M, 4k] output (:229-260); [M, 1] slices against [M] targets: the M x M form
        mu, lam, alpha, beta = output[:, 0::4], output[:, 1::4], output[:, 2::4], output[:, 3::4]
        evid = RL.evidential_loss_new(mu, lam, alpha, beta, targets, gpu, lam=0.2 if task_type == "mle_evidential" else 0.1)
        if task_type == "evidential":
            return [evid]
        if task_type == "mle_evidential":
            return [mle(output[:, 0], scope, targets, gpu), evid]
        variance = beta / (lam * (alpha - 1))
        if task_type == "mledis_evidential":
            return [RL.MLEDisLoss()(mu, variance, scope, targets, gpu), evid]
        return [RL.Listnet_For_Gauss()(mu, variance, scope, targets, gpu), evid]      # listnet_evidential
    if task_type == "mle_dirichlet":
        raise ValueError("task_type 'mle_dirichlet' raises NameError in the reference (its losses are never instantiated, "
                         "train_listwise.py:267-269); it is not supported")
    raise ValueError(f"task_type {task_type!r} is not covered by reactranker_amd (supported: {SUPPORTED_TASKS})")


def batch_loss(task_type: str, output, scope, targets, gpu, epoch: int = 0, epochs: int = 1, max_coeff: float = 1e-4, norm=None):
    """The loss the reference trainer forms for one batch (train_listwise.py:196-285).

    norm: None, or a mapping with the GLOBAL `queries` and `cands` counts of the step this batch is a shard of (what
    dp.Exchange.counts returns as its second value).  Every term is then divided by the global count of its own normaliser
    (dp.TASK_TERMS) instead of the batch's: the result is this shard's share of the whole step's loss - the shards' losses
    add up to the unsharded loss and their gradients to the unsharded gradient.  The four NIG task types compare every
    candidate with every target of the step and cannot be formed from a shard (ValueError).

    The eight composite task types of loss.TASK_STEPS take one launch for the loss and its gradient (loss.FusedStep,
    rr_task_loss_step_f32) when the output needs a gradient; FusedStep.enabled = False forms them term by term."""
    from . import dp
    if norm is not None:
        dp.require_shardable(task_type)
    if task_type in RL.TASK_STEPS:
        coef = RL.annealing_coef(max_coeff, epoch, epochs) if task_type in ("listnet_uq", "dirichlet_uq") else 0.0
        fused = RL.task_step_loss(task_type, output, scope, targets, gpu, coef, norm)
        if fused is not None:
            return fused
    terms = _loss_terms(task_type, output, scope, targets, gpu, epoch, epochs, max_coeff)
    if norm is not None:
        terms = [t if f == 1.0 else t * f for t, f in zip(terms, dp.term_scales(task_type, scope, norm))]
    loss = terms[0]
    for t in terms[1:]:
        loss = loss + t
    return loss


def train(model: torch.nn.Module, scheduler, train_batches: Union[Sequence, Callable[[int], Iterable]],
          val_batches: Sequence, path_checkpoints: Union[str, List[str], None], optimizer, epochs: int, seed: int, gpu: int,
          task_type: str = "mle", logger=None, save_metric: Optional[str] = None, max_coeff: float = 1e-4,
          mean: float = 0.0, std: float = 1.0, target_name: Optional[str] = None, normalize_target=True,
          epoch_hook: Optional[Callable] = None, group=None):
    """Same control flow as the reference train(): fixed seed, per batch forward / loss / zero_grad / backward /
    optimizer.step / scheduler.step (train_listwise.py:287-290), validation with ranking_metrics after every epoch,
    checkpoint whenever the selected metric does not get worse (:310-350).  `train_batches` is a sequence, or a
    callable epoch -> iterable (the reference reshuffles with seed=epoch, :178).  Returns the per-epoch history.
    save_metric 'kendall_tau' / 'spearman' / 'mrr' (RANK_CORR_METRICS; not in the reference) select on the mean per-query
    Kendall tau-b, Spearman rho or reciprocal rank of eval.rank_correlation: one more validation pass per epoch, whose dict
    the history record then holds under `rank_correlation`; the best starts at -inf (tau and rho lie in [-1, 1]) and a NaN
    epoch (no query with a defined value) never replaces it and never saves.
    epoch_hook(epoch, model, record): optional observer called after every epoch's validation (not in the reference; the
    trajectory tests read the validation scores through it).

    Data parallel (the reference has no distributed code): under an initialised torch.distributed
    (`group` = a process group, None = the default one) every rank passes ITS shard of every global step - whole queries,
    see reactranker_amd.dp.shard_query_batch - and of the validation queries.  Per step the rank's gradient is weighted
    by its share of the loss's normaliser and summed over the ranks in one all-reduce of the flat bucket the explicit
    backward writes into; validation statistics are summed over the ranks; rank 0 writes the checkpoints; every rank
    returns the same history.  Task types that sum terms with different normalisers (dp.TASK_TERMS) instead divide every
    term by the whole step's count (batch_loss(norm=...)) and sum the ranks' gradients unweighted; the four NIG task types need
    every target of the step and are refused (ValueError) before the first step.  One process (no torch.distributed) runs the same code with the exchange switched off."""
    from .dp import Exchange
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    model = model.cuda(gpu)
    ex = Exchange(model, group)
    try:
        if ex.on:                                       # refused before the first step, on every rank
            from .dp import require_shardable
            require_shardable(task_type)
        return _train(model, scheduler, train_batches, val_batches, path_checkpoints, optimizer, epochs, gpu, task_type, logger,
                      save_metric, max_coeff, mean, std, target_name, normalize_target, epoch_hook, ex)
    finally:
        ex.close()


def _train(model, scheduler, train_batches, val_batches, path_checkpoints, optimizer, epochs, gpu, task_type, logger, save_metric,
           max_coeff, mean, std, target_name, normalize_target, epoch_hook, ex):
    if target_name is not None:                       # raw targets: standardise / flip like the reference (:66-122)
        if callable(train_batches):
            raise ValueError("target standardisation needs the training batches as a sequence (statistics over all of them)")
        train_batches, val_batches, mean, std = standardize_batches(list(train_batches), list(val_batches), target_name,
                                                                     normalize_target, save_metric, ex)
    ex.broadcast_model(model)                         # identical replicas (a no-op for one process)
    if not callable(train_batches):
        ex.check_same_steps(len(train_batches), next(model.parameters()).device)
    # dropout streams: every forward draws a fresh stream seed from torch's generator (mpn._fresh_seed), which the
    # manual_seed above makes reproducible - like the reference, whose nn.Dropout advances that generator per call.
    # model.dropout_seed (a test knob that pins ONE stream for every step) must stay unset here.
    if getattr(model, "dropout_seed", None) is not None:
        model.dropout_seed = None
    score_old = [0.0, 0.0, 0.0] if save_metric == "all" else (float("inf") if save_metric == "mse" else 0.0)   # :54-59
    if save_metric in RANK_CORR_METRICS:
        score_old = float("-inf")
    history = []
    say = logger.info if (logger is not None and ex.is_writer) else (lambda *_: None)
    dev = next(model.parameters()).device
    from .dp import _KIND
    one_weight = task_type in _KIND                      # ONE normaliser: the rank's gradient is weighted as a whole
    for epoch in range(epochs):
        say("learning rate is: {}".format(optimizer.param_groups[0]["lr"]))
        model.train()
        loss = torch.zeros(1, device=dev)
        for b in (train_batches(epoch) if callable(train_batches) else train_batches):
            optimizer.zero_grad()
            norm = None
            if ex.on and not one_weight:                # terms with different normalisers: divide each by the step's count
                local, glob = ex.counts(b, dev)
                norm = glob
            if len(b["scope"]) > 0:
                output = model(b["r"], b["p"], gpu=gpu, add_features=b.get("add"))
                loss = batch_loss(task_type, output, b["scope"], b["targets"], gpu, epoch, epochs, max_coeff, norm=norm)
                RL.backward(loss)                       # loss.backward() (:288) seeded with the library's constant one (loss.FusedStep)
            else:                                       # an empty shard: this rank adds nothing to the step
                loss = torch.zeros(1, device=dev)
            if ex.on:
                if one_weight:
                    local, glob = ex.counts(b, dev)
                    w = ex.weight(task_type, local, glob)
                else:                                   # the rank's loss is already its share of the step's: plain sums
                    w = 1.0
                ex.reduce_grads(w)
                loss = loss.detach().reshape(-1)[:1] * w    # summed over the ranks below: the whole step's loss
            optimizer.step()
            scheduler.step()
        model.eval()
        top1, recall25, top25, ndcg = ranking_metrics(
            model, gpu, [(b["r"], b["p"], b["scope"], b["targets"], b.get("add")) for b in val_batches], exchange=ex)
        saved = False

        def keep(path):
            nonlocal saved
            saved = True
            if path is not None and ex.is_writer:
                save_checkpoint(path, model, mean, std)
        if save_metric is None or save_metric == "average_score":
            if top1 >= score_old:
                score_old = top1
                keep(path_checkpoints)
        elif save_metric == "all":
            for i, v in enumerate((top1, recall25, top25)):
                if v >= score_old[i]:
                    score_old[i] = v
                    keep(path_checkpoints[i] if path_checkpoints is not None else None)
        elif save_metric == "average_pred_in_targ":
            if recall25 >= score_old:
                score_old = recall25
                keep(path_checkpoints)
        elif save_metric == "average_top1_in_pred":
            if top25 >= score_old:
                score_old = top25
                keep(path_checkpoints)
        elif save_metric in NDCG_METRICS:
            v = ndcg[NDCG_METRICS.index(save_metric)]
            if v >= score_old:
                score_old = v
                keep(path_checkpoints)
        elif save_metric == "mse":                          # :345-351 (calculate_mse: the LAST validation batch's error)
            mse_val = calculate_mse(model, gpu, [(b["r"], b["p"], b["scope"], b["targets"], b.get("add")) for b in val_batches],
                                    exchange=ex)
            if mse_val <= score_old:
                score_old = mse_val
                keep(path_checkpoints)
        elif save_metric in RANK_CORR_METRICS:
            corr = rank_correlation(model, gpu, [(b["r"], b["p"], b["scope"], b["targets"], b.get("add")) for b in val_batches],
                                    exchange=ex)
            if corr[save_metric] >= score_old:                  # False for a NaN
                score_old = corr[save_metric]
                keep(path_checkpoints)
        else:
            raise Exception("Unknown save metric")
        saved = saved and path_checkpoints is not None
        last_loss = float(ex.sum(loss.detach().sum().reshape(1).clone()))     # the reference logs the last step's loss (:353)
        rec = dict(epoch=epoch + 1, train_loss=last_loss, top1=float(top1), top1_in_pred_top25=float(top25),
                   pred_top25_in_targ_top25=float(recall25), ndcg=[float(x) for x in ndcg], checkpoint=saved)
        if save_metric == "mse":
            rec["mse"] = float(mse_val)
        if save_metric in RANK_CORR_METRICS:
            rec["rank_correlation"] = corr
        history.append(rec)
        if epoch_hook is not None:
            epoch_hook(epoch, model, rec)
        say("Epoch [{}/{}], train_loss,{:.4f}, top1,{:.4f}, top1_in_pred_top25%,{:.4f}, pred_top25%_in_targ_top25%,{:.4f}"
            .format(epoch + 1, epochs, rec["train_loss"], top1, top25, recall25))
    return history
