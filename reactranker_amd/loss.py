"""Ranking / pointwise losses — mirror of reference `reactranker/train/loss.py`: the losses on the hot
path (MLEloss :64-99, ListnetLoss :317-352, evidential_ranking :477-556, GaussDisLoss :144-162,
LogCumsumExp :9-61), RankNet's inline loss (train/train_pairwise.py:99-137), and the rest of the
trainer's import line (MLEDisLoss, Lognorm, Listnet_For_evidential, Listnet_For_Gauss, Listnetlognorm,
Listnet_with_uq, evidential_loss_new, Dirichlet_uq) plus the regression_exploss expression, and the pairwise trainer's
inline losses: the Beta-density KL of beta_dis_train_loop (train_pairwise.py:189-226), the evidential pair loss of
beta_evi_train_loop (:276-307) and the pair loss of baseline_pairwise_training_loop (:33-59).

Same call signatures (`loss(score, scope, targets, gpu)` and kin) and return shapes ([1] for the
per-query means, 0-d for ListNet and the pointwise means).  Each loss is one fused HIP kernel per
direction (one wavefront per query) instead of a Python loop of ~10 ATen ops per query.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, lib, ptr, stream


@lru_cache(maxsize=256)
def _segments(scope: tuple, device_str: str):
    off = np.zeros(len(scope) + 1, np.int32)
    np.cumsum(np.asarray(scope, np.int64), out=off[1:])
    t = torch.from_numpy(off).to(device_str)
    return t, int(off[-1]), (max(scope) if scope else 0)


def _targets(targets, device) -> torch.Tensor:
    """targets as a contiguous float32 vector on `device` (reference loss.py:85)"""
    t = torch.as_tensor(targets, dtype=torch.float32)
    if t.device != device:                              # (a same-device .to() still costs a dispatch on the step's host path)
        t = t.to(device)
    return t.reshape(-1).contiguous()


def _call(name, *args):
    """the library's entry point `name` on the current stream; a non-zero status raises"""
    check(getattr(lib(), name)(*args, stream()), name)


def _prep(score: torch.Tensor, scope, targets, gpu, what: str = "score"):
    """scope as a tuple, its device offsets, the candidate and longest-list counts, the targets (None stays None)"""
    if gpu is not None:
        torch.cuda.set_device(gpu)                      # reference loss.py:83
    _lib.require_cuda(score, what)
    scope = tuple(int(c) for c in (scope.tolist() if hasattr(scope, "tolist") else scope))
    seg, total, max_len = _segments(scope, str(score.device))
    if total != score.shape[0]:
        raise RuntimeError(f"sum(scope) = {total} but {what} has {score.shape[0]} rows")
    t = None if targets is None else _targets(targets, score.device)
    if t is not None and t.numel() != total:
        raise RuntimeError("targets and score lengths differ")
    return scope, seg, total, max_len, t


def _vec(x: torch.Tensor) -> torch.Tensor:
    """1-D float32 view with arbitrary element stride (a column of the [M,2] model output is fine)."""
    if x.dtype != torch.float32:
        x = x.float()
    if x.dim() != 1:
        x = x.reshape(-1)
    return x


def _f1(dev):
    return torch.empty(1, dtype=torch.float32, device=dev)


def _first_column(y: torch.Tensor) -> torch.Tensor:
    """[M] as it is, the first column of [M, k] (read in place; reference train_pairwise.py:115-116)"""
    return y[:, 0] if y.dim() > 1 else y


def _ndcg_k(ndcg_k, what) -> int:
    if int(ndcg_k) != ndcg_k or ndcg_k < 0:
        raise ValueError(f"{what}: ndcg_k must be a non-negative integer (0: the whole list)")
    return int(ndcg_k)


def _inv_count(n) -> float:
    """1 / n of a positive host count as the float32 the step kernels multiply by"""
    return float(np.float32(1.0 / int(n)))


class FusedStep:
    """Loss and d loss / d score in ONE launch (rr_listmle_step_f32 and its ListNet / evidential twins, csrc/loss.hip).

    The reference's trainer step is `loss = loss_func(score, ...); loss.backward()` (train/train_listwise.py:287-288): the loss
    is the root of the graph and its upstream gradient is the constant one.  When the score requires a gradient the forward
    therefore also writes d loss / d score for that case - same operations in the same order as the backward kernel with an
    upstream gradient of 1.0f, the bits are the same - and `reactranker_amd.loss.backward(loss)` starts the backward with the
    library's cached constant-one tensor: the loss's backward then recognises it (by address) and hands out the gradient
    that already exists.  What a step no longer launches: the separate reduction of the per-query partials, autograd's
    ones_like(loss) fill, a `.sum()` over one element, the loss's backward kernel.  Any other upstream gradient (a plain
    `loss.backward()`, a scaled loss) takes the backward kernel as before - nothing depends on the fast path being hit.
    The composite task types of TASK_STEPS do the same over the head's whole output (rr_task_loss_step_f32, csrc/task_loss.hip:
    _TaskStepFn below); there another upstream gradient multiplies the stored gradient.
    hits counts the backward calls it served (tests)."""
    enabled = True
    hits = 0
    _unit = {}
    _counter = {}


def _unit_like(t: torch.Tensor) -> torch.Tensor:
    key = (str(t.device), tuple(t.shape))
    u = FusedStep._unit.get(key)
    if u is None:
        u = FusedStep._unit[key] = torch.ones(tuple(t.shape), dtype=torch.float32, device=t.device)
    return u


def _is_unit(g: torch.Tensor) -> bool:
    u = FusedStep._unit.get((str(g.device), tuple(g.shape)))
    return u is not None and g.dtype == torch.float32 and g.data_ptr() == u.data_ptr()


def _counter(dev) -> torch.Tensor:
    """the zero-initialised ticket word of the step kernels: one per (device, stream) - launches of one stream are ordered,
    and every launch leaves it at zero"""
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
    c = FusedStep._counter.get(key)
    if c is None:
        c = FusedStep._counter[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return c


def backward(loss: torch.Tensor) -> None:
    """`loss.backward()` for a loss that is the root of the graph (reference train/train_listwise.py:288), started with the
    library's constant-one gradient instead of a freshly filled one: a loss of this module then returns the gradient its
    forward launch already wrote (FusedStep).  Works for any other one-element float32 loss as well (plain autograd)."""
    if loss.numel() == 1 and loss.dtype == torch.float32 and loss.is_cuda:
        loss.backward(gradient=_unit_like(loss))
    else:
        loss.backward()


class _FusedListFn(torch.autograd.Function):
    """rr_{kind}_{fwd,step,bwd}_f32 of the three losses with a one-launch step (FusedStep).  'listmle' and 'listnet' read one
    strided column; 'evidential_ranking' reads the two columns of an [M, 2] tensor.  'listnet' also passes `total` (its ONE
    mean over all candidates) and returns 0-d (torch.mean, reference loss.py:347); the other two return [1]."""

    @staticmethod
    def _in(kind, x):
        return [ptr(x[:, 0]), ptr(x[:, 1]), x.stride(0)] if kind == "evidential_ranking" else [ptr(x), x.stride(0)]

    @staticmethod
    def _out(kind, x):
        """an empty gradient like x and its arguments"""
        d = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
        return d, ([ptr(d[:, 0]), ptr(d[:, 1]), 2] if kind == "evidential_ranking" else [ptr(d), 1])

    @staticmethod
    def forward(ctx, kind, x, targets, seg, Q, max_len, total):
        x = x.detach()
        if kind != "evidential_ranking":
            x = _vec(x)
        elif x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 2 or x.stride(1) != 1:
            x = x.float().reshape(-1, 2).contiguous()
        loss, part = _f1(x.device), torch.empty(max(Q, 1), dtype=torch.float32, device=x.device)
        args = _FusedListFn._in(kind, x) + [ptr(targets), ptr(seg), Q, max_len] + ([total] if kind == "listnet" else [])
        ctx.ds_unit = None
        if FusedStep.enabled and ctx.needs_input_grad[1]:
            d, outs = _FusedListFn._out(kind, x)
            _call(f"rr_{kind}_step_f32", *args, ptr(loss), ptr(part), ptr(_counter(x.device)), *outs)
            ctx.ds_unit = d
        else:
            _call(f"rr_{kind}_fwd_f32", *args, ptr(loss), ptr(part))
        ctx.save_for_backward(x, targets, seg)
        ctx.meta = (kind, args)
        return loss.reshape(()) if kind == "listnet" else loss

    @staticmethod
    def backward(ctx, g):
        if ctx.ds_unit is not None and _is_unit(g):      # the gradient the forward launch already wrote (handed out once)
            d, ctx.ds_unit = ctx.ds_unit, None
            FusedStep.hits += 1
        else:
            x = ctx.saved_tensors[0]                     # (the saved tensors keep the pointers in `args` alive)
            kind, args = ctx.meta
            g = g.reshape(-1).contiguous().float()
            d, outs = _FusedListFn._out(kind, x)
            _call(f"rr_{kind}_bwd_f32", *args, ptr(g), *outs)
        return (None, d) + (None,) * 5


# The window losses: a sum over the queries of a window plus a count (ordered pairs, ranked queries), normalised by a HOST count.
# kind (the entry points' stem: rr_{kind}_{fwd,bwd,step}_f32) -> (partial dtype, partial words per query, has a step entry,
# what bwd passes after the hyper-parameters).  The hyper-parameters themselves come with the call, as the entry points
# take them after max_len.
_WINDOW = {
    "ranknet": (torch.float32, 2, False, (0,)),           # (sigma); bwd mode 0: the true gradient of loss_sum
    "lambdarank": (torch.float32, 2, True, ()),           # (sigma, ndcg_k)
    "approx_ndcg": (torch.float32, 2, True, ()),          # (temperature, ndcg_k)
    "betanet": (torch.float64, 1, False, ()),             # (alpha0)
    "beta_evidential": (torch.float64, 1, False, ()),     # (the annealing coefficient)
}


class _WindowFn(torch.autograd.Function):
    """scale * loss_sum of one of _WINDOW and the window's count (int64 device scalar, not differentiable).  A kind with a step
    entry, when the score wants a gradient and FusedStep is on: rr_{kind}_step_f32 writes the loss and scale * d loss_sum /
    d score in one launch and `backward(loss)` hands that gradient out.  Otherwise rr_{kind}_fwd_f32, and rr_{kind}_bwd_f32
    with the upstream gradient times `scale` - the same bits for an upstream gradient of one."""

    @staticmethod
    def forward(ctx, kind, score, targets, seg, Q, max_len, hyper, scale):
        part_dtype, part_words, has_step, bwd_extra = _WINDOW[kind]
        s = _vec(score.detach())
        loss = _f1(s.device)
        count = torch.empty(1, dtype=torch.int64, device=s.device)
        part = torch.empty(part_words * max(Q, 1), dtype=part_dtype, device=s.device)
        args = [ptr(s), s.stride(0), ptr(targets), ptr(seg), Q, max_len, *hyper]
        ctx.ds_unit = None
        if has_step and FusedStep.enabled and ctx.needs_input_grad[1]:
            d = torch.empty(s.shape[0], dtype=torch.float32, device=s.device)
            _call(f"rr_{kind}_step_f32", *args, scale, ptr(loss), ptr(count), ptr(part), ptr(_counter(s.device)), ptr(d), 1)
            ctx.ds_unit = d
        else:
            _call(f"rr_{kind}_fwd_f32", *args, ptr(loss), ptr(count), ptr(part))
            if scale != 1.0:
                loss = loss * scale                      # (a float32 product, as in the step kernel)
        ctx.save_for_backward(s, targets, seg)
        ctx.meta = (kind, args + list(bwd_extra), scale)
        ctx.mark_non_differentiable(count)
        return loss.reshape(()), count

    @staticmethod
    def backward(ctx, g, _gc):
        if ctx.ds_unit is not None and _is_unit(g):      # the gradient the forward launch already wrote (handed out once)
            d, ctx.ds_unit = ctx.ds_unit, None
            FusedStep.hits += 1
        else:
            s = ctx.saved_tensors[0]                     # (the saved tensors keep the pointers in `args` alive)
            kind, args, scale = ctx.meta
            g = g.reshape(-1).float()
            if scale != 1.0:
                g = g * scale
            g = g.contiguous()
            d = torch.empty(s.shape[0], dtype=torch.float32, device=s.device)
            _call(f"rr_{kind}_bwd_f32", *args, ptr(g), ptr(d), 1)
        return (None, d) + (None,) * 6


class _PointwiseFn(torch.autograd.Function):
    """rr_{kind}_fwd_f32 / rr_{kind}_bwd_f32 of the pointwise means: kind 'mse' and 'exp_mse' (var None), 'gauss_nll' and
    'lognorm' (x and var read with one stride); 0-d mean."""

    @staticmethod
    def forward(ctx, kind, x, var, targets):
        m = _vec(x.detach())
        v = None if var is None else _vec(var.detach())
        if v is not None and v.stride(0) != m.stride(0):
            v = v.contiguous()
            m = m.contiguous()
        n = m.shape[0]
        if targets.shape[0] != n or (v is not None and v.shape[0] != n):
            raise RuntimeError(f"{kind}: inputs and targets lengths differ")
        loss = _f1(m.device)
        part = torch.empty(int(lib().rr_pointwise_partial_count(n)), dtype=torch.float32, device=m.device)
        args = ([ptr(m)] if v is None else [ptr(m), ptr(v)]) + [m.stride(0), ptr(targets), n]
        _call(f"rr_{kind}_fwd_f32", *args, ptr(loss), ptr(part))
        ctx.save_for_backward(m, targets, *([] if v is None else [v]))
        ctx.meta = (kind, args, [tuple(x.shape)] + ([] if var is None else [tuple(var.shape)]))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        kind, args, shapes = ctx.meta                    # (the saved tensors keep the pointers in `args` alive)
        m = ctx.saved_tensors[0]
        g = g.reshape(-1).contiguous().float()
        ds = [torch.empty(sh, dtype=torch.float32, device=m.device) for sh in shapes]      # contiguous, in the inputs' shapes
        _call(f"rr_{kind}_bwd_f32", *args, ptr(g), *[ptr(d) for d in ds], 1)
        return (None, *ds, *([None] * (3 - len(ds))))


class LogCumsumExp(torch.autograd.Function):
    """Reference train/loss.py:9-61 for a 1-D input (dim 0), forward and backward in HIP."""

    @staticmethod
    def forward(ctx, input_data):
        x = input_data.detach().float().contiguous()
        _lib.require_cuda(x, "input_data")
        if x.dim() != 1:
            raise RuntimeError("LogCumsumExp: 1-D input expected (the reference applies it per sorted list)")
        y = torch.empty_like(x)
        check(lib().rr_logcumsumexp_fwd_f32(ptr(x), x.shape[0], ptr(y), stream()), "rr_logcumsumexp_fwd_f32")
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        x, y = ctx.saved_tensors
        g = grad_output.float().contiguous()
        gx = torch.empty_like(x)
        check(lib().rr_logcumsumexp_bwd_f32(ptr(x), ptr(y), ptr(g), x.shape[0], ptr(gx), stream()),
              "rr_logcumsumexp_bwd_f32")
        return gx


class MLEloss(nn.Module):
    """ListMLE (reference train/loss.py:64-99)."""

    def forward(self, score, scope, targets_train, gpu: int = None):
        scope, seg, total, max_len, t = _prep(score, scope, targets_train, gpu)
        return _FusedListFn.apply("listmle", score, t, seg, len(scope), max_len, total)


class ListnetLoss(nn.Module):
    """ListNet top-1 (reference train/loss.py:317-352)."""

    def forward(self, score, scope, targets, gpu: int = None):
        scope, seg, total, max_len, t = _prep(score, scope, targets, gpu)
        return _FusedListFn.apply("listnet", score, t, seg, len(scope), max_len, total)


class evidential_ranking(nn.Module):
    """UC-Listwise (reference train/loss.py:477-556); max_coeff/epoch/epochs are accepted and unused, as there."""

    def forward(self, possibilities, scope, targets, max_coeff=None, epoch=None, epochs=None, gpu: int = None):
        scope, seg, total, max_len, t = _prep(possibilities, scope, targets, gpu)
        return _FusedListFn.apply("evidential_ranking", possibilities, t, seg, len(scope), max_len, total)


class GaussDisLoss(nn.Module):
    """Reference train/loss.py:144-162."""

    def forward(self, mean_scores, std_scores, targets, gpu: int = None):
        if gpu is not None:
            torch.cuda.set_device(gpu)
        _lib.require_cuda(mean_scores, "mean_scores")
        return _PointwiseFn.apply("gauss_nll", mean_scores, std_scores, _targets(targets, mean_scores.device))


class MSELoss(nn.Module):
    """nn.MSELoss() of the default 'regression' branch (reference train/train_listwise.py:166-167,282-285)."""

    def forward(self, output, targets):
        _lib.require_cuda(output, "output")
        return _PointwiseFn.apply("mse", output, None, _targets(targets, output.device))


def ranknet_loss(y_pred, scope, targets, sigma: float = 1.0, gpu: int = None):
    """RankNet 'sum_session' over a window of queries (reference train/train_pairwise.py:99-122,141).

    Returns (loss_sum, pairs): loss_sum is differentiable (divide by pairs and call backward,
    as the trainer does at :147-150); pairs is an int64 device scalar.  `y_pred` may be [M] or
    [M, k] (first column used, :115-116).
    """
    y_pred = _first_column(y_pred)
    scope, seg, total, max_len, t = _prep(y_pred, scope, targets, gpu)
    return _WindowFn.apply("ranknet", y_pred, t, seg, len(scope), max_len, (float(sigma),), 1.0)


def ranknet_lambda(y_pred, scope, targets, sigma: float = 1.0, gpu: int = None):
    """'accelerate_grad' closed-form lambdas `back` (reference train/train_pairwise.py:125-133)."""
    y_pred = _first_column(y_pred)
    scope, seg, total, max_len, t = _prep(y_pred, scope, targets, gpu)
    s = _vec(y_pred.detach())
    one = torch.ones(1, dtype=torch.float32, device=s.device)
    out = torch.empty(s.shape[0], dtype=torch.float32, device=s.device)
    _call("rr_ranknet_bwd_f32", ptr(s), s.stride(0), ptr(t), ptr(seg), len(scope), max_len, float(sigma), 1, ptr(one), ptr(out), 1)
    return out


def lambdarank_loss(y_pred, scope, targets, sigma: float = 1.0, ndcg_k: int = 0, gpu: int = None, pairs: int = None):
    """LambdaRank over a window of queries: RankNet's pair cost, every pair weighted by the |delta NDCG| of swapping the two
    candidates in the current predicted order - gains exp(target) as in `ranking_metrics`, NDCG truncated at `ndcg_k`
    positions (0: the whole list).  The weights are constants; the definition is in DESIGN section 4b.  This library's own
    loss: the reference trainer has none.

    Returns (loss, pairs_tensor).  pairs=None: loss is loss_sum, as for ranknet_loss.  pairs: a host int, the ordered-pair
    count to normalise by (the WINDOW's count for a shard of a data-parallel step) - loss is loss_sum * float32(1 / pairs) and
    `backward(loss)` then takes the gradient the same launch wrote (FusedStep).  pairs_tensor is this call's own count, an
    int64 device scalar.  `y_pred` may be [M] or [M, k] (first column, read in place)."""
    y_pred = _first_column(y_pred)
    if not sigma > 0:
        raise ValueError("lambdarank_loss: sigma must be positive")
    ndcg_k = _ndcg_k(ndcg_k, "lambdarank_loss")
    scale = 1.0
    if pairs is not None:
        if int(pairs) <= 0:
            raise ValueError("lambdarank_loss: pairs must be a positive count (a window without pairs is skipped by the trainer)")
        scale = _inv_count(pairs)
    scope, seg, total, max_len, t = _prep(y_pred, scope, targets, gpu)
    return _WindowFn.apply("lambdarank", y_pred, t, seg, len(scope), max_len, (float(sigma), ndcg_k), scale)


def _temperature(temperature, what) -> float:
    # judged as the float32 the kernels get, by rr_soft_rank_fwd_f32's rule: they multiply by 1 / T, which has to be finite
    with np.errstate(all="ignore"):
        t = np.float32(temperature)
        ok = t > 0 and np.isfinite(t) and np.isfinite(np.float32(1.0) / t)
    if not ok:
        raise ValueError(f"{what}: temperature must be a positive finite float32 with a finite reciprocal (score units)")
    return float(temperature)


class _SoftRankFn(torch.autograd.Function):
    """rr_soft_rank_fwd_f32 / rr_soft_rank_bwd_f32 (csrc/approx_ndcg.hip)"""

    @staticmethod
    def forward(ctx, score, seg, Q, max_len, temperature):
        s = _vec(score.detach())
        rank = torch.empty(s.shape[0], dtype=torch.float32, device=s.device)
        args = [ptr(s), s.stride(0), ptr(seg), Q, max_len, temperature]
        _call("rr_soft_rank_fwd_f32", *args, ptr(rank), 1)
        ctx.save_for_backward(s, seg)
        ctx.args = args
        return rank

    @staticmethod
    def backward(ctx, g):
        s = ctx.saved_tensors[0]                         # (the saved tensors keep the pointers in `args` alive)
        g = g.float().contiguous()
        d = torch.empty(s.shape[0], dtype=torch.float32, device=s.device)
        _call("rr_soft_rank_bwd_f32", *ctx.args, ptr(g), 1, ptr(d), 1)
        return (d,) + (None,) * 4


def soft_rank(y_pred, scope, temperature: float = 1.0, gpu: int = None):
    """Differentiable ranks of every candidate inside its query: r_i = 1 + sum_{j != i} sigmoid((s_j - s_i) / T), 1 for the
    best score; float32 [M], differentiable in `y_pred`.  Tied scores get equal ranks and the ranks of a query of C candidates
    sum to C (C + 1) / 2.  `temperature` is in SCORE units: against a spread of the scores much smaller than T every rank
    blurs towards (C + 1) / 2, and as T -> 0 the ranks become the hard ones (and the gradient vanishes).  Soft Spearman, soft
    top-k recall and the like are a few lines of torch on top.  `y_pred` may be [M] or [M, k] (first column, read in place).
    DESIGN section 4b."""
    y_pred = _first_column(y_pred)
    temperature = _temperature(temperature, "soft_rank")
    scope, seg, total, max_len, _ = _prep(y_pred, scope, None, gpu, "y_pred")
    return _SoftRankFn.apply(y_pred, seg, len(scope), max_len, temperature)


def approx_ndcg_loss(y_pred, scope, targets, temperature: float = 1.0, ndcg_k: int = 0, gpu: int = None, queries: int = None):
    """ApproxNDCG over a window of queries: per ranked query 1 - sum_i G_i psi(r_i), the NDCG that `ranking_metrics` reports
    (gains exp(target), truncated at `ndcg_k` positions, 0: the whole list) written on the soft ranks r_i of `soft_rank`, so
    the gradient flows through the ranks; inside the list the truncation is a smooth gate sigmoid(k + 1/2 - r), one rank wide.
    `temperature` is in SCORE units (see soft_rank): small against the score differences the loss approaches 1 - NDCG and its
    gradient vanishes, large it blurs the ranks.  The definition is in DESIGN section 4b.  This library's own loss.

    Returns (loss, ranked_tensor).  queries=None: loss is the plain sum over the queries.  queries: a host int, the query count
    to normalise by (the WINDOW's count for a shard of a data-parallel step) - loss is the sum * float32(1 / queries) and
    `backward(loss)` then takes the gradient the same launch wrote (FusedStep).  ranked_tensor is this call's number of ranked
    queries (those with two different targets; the others add nothing and get a zero gradient), an int64 device scalar.
    `y_pred` may be [M] or [M, k] (first column, read in place)."""
    y_pred = _first_column(y_pred)
    temperature = _temperature(temperature, "approx_ndcg_loss")
    ndcg_k = _ndcg_k(ndcg_k, "approx_ndcg_loss")
    scale = 1.0
    if queries is not None:
        if int(queries) != queries or int(queries) <= 0:
            raise ValueError("approx_ndcg_loss: queries must be a positive count")
        scale = _inv_count(queries)
    scope, seg, total, max_len, t = _prep(y_pred, scope, targets, gpu)
    return _WindowFn.apply("approx_ndcg", y_pred, t, seg, len(scope), max_len, (temperature, ndcg_k), scale)


# ---------------------------------------------------------------------------------------------- the remaining task types' losses
def annealing_coef(max_coeff, epoch, epochs):
    """The annealing coefficient of Listnet_with_uq / Dirichlet_uq (reference train/loss.py:393, 468), computed on the host as
    there: epochs == 1 raises ZeroDivisionError in both."""
    return max_coeff * (epoch / (epochs - 1)) ** 3


def _columns(tensors, n, what):
    """Columns 0 .. n-1 of torch.cat(tensors, 1) as 1-D views, without the copy (the reference concatenates, loss.py:120,
    211, 253, 295); a 1-D tensor counts as one column."""
    cols = []
    for x in tensors:
        if x.dim() == 1:
            cols.append(x)
        elif x.dim() == 2:
            cols.extend(x[:, k] for k in range(x.shape[1]))
        else:
            raise RuntimeError(f"{what}: inputs must be [M] or [M, k], got {tuple(x.shape)}")
    if len(cols) < n:
        raise RuntimeError(f"{what}: needs {n} input columns, got {len(cols)}")
    return cols[:n]


_LISTWISE_COEF = ("listnet_uq", "dirichlet_uq")       # entries that take the annealing coefficient


class _ListwiseVariantFn(torch.autograd.Function):
    """rr_{kind}_fwd_f32 / rr_{kind}_bwd_f32 over 1-D (possibly strided) per-candidate inputs; loss shape [1]."""

    @staticmethod
    def forward(ctx, kind, coef, targets, seg, Q, max_len, *xs):
        vs = [_vec(x.detach()) for x in xs]
        dev = vs[0].device
        for v in vs[1:]:
            if v.shape[0] != vs[0].shape[0]:
                raise RuntimeError(f"{kind}: inputs have {vs[0].shape[0]} and {v.shape[0]} rows")
        loss, part = _f1(dev), torch.empty(max(Q, 1), dtype=torch.float32, device=dev)
        args = [a for v in vs for a in (ptr(v), v.stride(0))] + [ptr(targets), ptr(seg), Q, max_len]
        if kind in _LISTWISE_COEF:
            args.append(float(coef))
        name = f"rr_{kind}_fwd_f32"
        check(getattr(lib(), name)(*args, ptr(loss), ptr(part), stream()), name)
        ctx.save_for_backward(targets, seg, *vs)
        ctx.meta = (kind, coef, Q, max_len, [tuple(x.shape) for x in xs])
        return loss

    @staticmethod
    def backward(ctx, g):
        targets, seg, *vs = ctx.saved_tensors
        kind, coef, Q, max_len, shapes = ctx.meta
        g = g.reshape(-1).contiguous().float()
        ds = [torch.empty(v.shape[0], dtype=torch.float32, device=v.device) for v in vs]
        args = [a for v in vs for a in (ptr(v), v.stride(0))] + [ptr(targets), ptr(seg), Q, max_len]
        if kind in _LISTWISE_COEF:
            args.append(float(coef))
        name = f"rr_{kind}_bwd_f32"
        check(getattr(lib(), name)(*args, ptr(g), *[ptr(d) for d in ds], 1, stream()), name)
        return (None,) * 6 + tuple(d.reshape(sh) for d, sh in zip(ds, shapes))


def _listwise(kind, xs, scope, targets, gpu, coef=0.0):
    scope, seg, total, max_len, t = _prep(xs[0], scope, targets, gpu)
    for x in xs[1:]:
        _lib.require_cuda(x, kind)
        if x.shape[0] != total:
            raise RuntimeError(f"sum(scope) = {total} but an input has {x.shape[0]} rows")
    return _ListwiseVariantFn.apply(kind, coef, t, seg, len(scope), max_len, *xs)


class MLEDisLoss(nn.Module):
    """ListMLE with a per-candidate variance (reference train/loss.py:102-141): mean and variance are [M, k] (or [M]);
    columns 0 and 1 of their concatenation are the score and the variance, as there.  Returns shape [1]."""

    def forward(self, mean, variance, scope, targets, gpu: int = None):
        return _listwise("mledis", _columns((mean, variance), 2, "MLEDisLoss"), scope, targets, gpu)


class Listnet_For_Gauss(nn.Module):
    """Reference train/loss.py:233-272 (columns as in MLEDisLoss).  Returns shape [1]."""

    def forward(self, mean, variance, scope, targets, gpu: int = None):
        return _listwise("listnet_gauss", _columns((mean, variance), 2, "Listnet_For_Gauss"), scope, targets, gpu)


class Listnetlognorm(nn.Module):
    """Reference train/loss.py:275-314 (columns as in MLEDisLoss; scores must be non-zero).  Returns shape [1]."""

    def forward(self, mean, variance, scope, targets, gpu: int = None):
        return _listwise("listnet_lognorm", _columns((mean, variance), 2, "Listnetlognorm"), scope, targets, gpu)


class Listnet_For_evidential(nn.Module):
    """Reference train/loss.py:187-230: columns 0, 1, 2 of cat(mean, v, alpha).  Returns shape [1]."""

    def forward(self, mean, v, alpha, scope, targets, gpu: int = None):
        return _listwise("listnet_evidential", _columns((mean, v, alpha), 3, "Listnet_For_evidential"), scope, targets, gpu)


def _one_column(x, what):
    if x.dim() != 1:
        raise RuntimeError(f"{what}: scores must be [M] (the task_num = 1 head's output), got {tuple(x.shape)}")
    return x


class Listnet_with_uq(nn.Module):
    """Reference train/loss.py:355-399 on positive scores [M].  Returns shape [1]."""

    def forward(self, score, scope, targets, max_coeff, epoch, epochs, gpu: int = None):
        coef = annealing_coef(max_coeff, epoch, epochs)
        return _listwise("listnet_uq", [_one_column(score, "Listnet_with_uq")], scope, targets, gpu, coef)


class Dirichlet_uq(nn.Module):
    """Reference train/loss.py:440-474 on positive concentrations [M].  Returns shape [1]."""

    def forward(self, concentration, scope, targets, max_coeff, epoch, epochs, gpu: int = None):
        coef = annealing_coef(max_coeff, epoch, epochs)
        return _listwise("dirichlet_uq", [_one_column(concentration, "Dirichlet_uq")], scope, targets, gpu, coef)


class _NigFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cross, lam, eps, targets, *params):
        xs = [_vec(x.detach()) for x in params]
        n = targets.shape[0]
        dev = xs[0].device
        loss, part = _f1(dev), torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        args = [a for x in xs for a in (ptr(x), x.stride(0))] + [ptr(targets), n, int(cross), float(lam)]
        check(lib().rr_nig_fwd_f32(*args, float(eps), ptr(loss), ptr(part), stream()), "rr_nig_fwd_f32")
        ctx.save_for_backward(targets, *xs)
        ctx.meta = (cross, lam, [tuple(x.shape) for x in params])
        return loss.reshape(())                         # torch.mean -> 0-d (reference loss.py:437)

    @staticmethod
    def backward(ctx, g):
        targets, *xs = ctx.saved_tensors
        cross, lam, shapes = ctx.meta
        n = targets.shape[0]
        g = g.reshape(-1).contiguous().float()
        ds = [torch.empty(n, dtype=torch.float32, device=g.device) for _ in range(4)]
        args = [a for x in xs for a in (ptr(x), x.stride(0))] + [ptr(targets), n, int(cross), float(lam)]
        check(lib().rr_nig_bwd_f32(*args, ptr(g), *[ptr(d) for d in ds], 1, stream()), "rr_nig_bwd_f32")
        return (None,) * 4 + tuple(d.reshape(sh) for d, sh in zip(ds, shapes))


def evidential_loss_new(mu, v, alpha, beta, targets, gpu, lam=1, epsilon=1e-4):
    """Deep-evidential-regression NLL + regulariser (reference train/loss.py:402-437), mean over the BROADCAST shape, 0-d.

    Two forms, as torch broadcasting makes them: parameters [M] with targets [M] (elementwise), or parameters [M, 1] with
    targets [M] - what the trainer passes (column slices of the [M, 4] output) - which evaluates every parameter row
    against every target, M x M terms.  Any other shape is refused."""
    if gpu is not None:
        torch.cuda.set_device(gpu)
    _lib.require_cuda(mu, "mu")
    params = (mu, v, alpha, beta)
    shape = tuple(mu.shape)
    t = torch.as_tensor(targets, dtype=torch.float32)
    if t.dim() > 1 or any(tuple(x.shape) != shape for x in params):
        raise ValueError(f"evidential_loss_new: parameters {[tuple(x.shape) for x in params]} with targets {tuple(t.shape)}: "
                         "supported are parameters [M] or [M, 1], all alike, with targets [M]")
    t = _targets(t, mu.device)
    M = t.shape[0]
    if len(shape) == 1 and shape[0] == M:
        cross = 0
    elif len(shape) == 2 and shape[1] == 1 and shape[0] == M:
        cross = 1
    else:
        raise ValueError(f"evidential_loss_new: parameters {shape} with targets [{M}]: "
                         "supported are parameters [M] (elementwise) or [M, 1] (all M x M pairs) with targets [M]")
    for x in params:
        _lib.require_cuda(x, "evidential_loss_new parameter")
    return _NigFn.apply(cross, float(lam), float(epsilon), t, *params)


def digamma(x: torch.Tensor) -> torch.Tensor:
    """The device digamma behind evidential_loss_new's d/dalpha (elementwise, float32, no autograd)."""
    _lib.require_cuda(x, "x")
    x = x.detach().float().contiguous()
    y = torch.empty_like(x)
    check(lib().rr_digamma_f32(ptr(x), x.numel(), ptr(y), stream()), "rr_digamma_f32")
    return y


class Lognorm(nn.Module):
    """Reference train/loss.py:165-184 (0-d mean).  The reference prints the value on every call; this one does not."""

    def forward(self, scores, std_scores, targets, gpu: int = None):
        if gpu is not None:
            torch.cuda.set_device(gpu)
        _lib.require_cuda(scores, "scores")
        return _PointwiseFn.apply("lognorm", scores, std_scores, _targets(targets, scores.device))


class ExpMSELoss(nn.Module):
    """mean((exp(targets) - exp(output))^2): the 'regression_exploss' branch (reference train/train_listwise.py:274-279),
    an inline expression there.  0-d."""

    def forward(self, output, targets):
        _lib.require_cuda(output, "output")
        return _PointwiseFn.apply("exp_mse", output, None, _targets(targets, output.device))


# ---------------------------------------------------------------------------------------------- composite task types in one launch
# task type -> (list term, point term, columns it reads, loss is 0-d) for rr_task_loss_step_f32 (csrc/task_loss.hip)
TASK_STEPS = {
    "mle_gaussian": (_lib.RR_LIST_MLE, _lib.RR_POINT_GAUSS, 2, False),
    "listnet_gauss": (_lib.RR_LIST_LISTNET, _lib.RR_POINT_GAUSS, 2, True),
    "mle_regression": (_lib.RR_LIST_MLE, _lib.RR_POINT_MSE, 1, False),
    "listnet_regression": (_lib.RR_LIST_LISTNET, _lib.RR_POINT_MSE, 1, True),
    "mledis_gaussian": (_lib.RR_LIST_MLEDIS, _lib.RR_POINT_GAUSS, 2, False),
    "listnetdis_gauss": (_lib.RR_LIST_LISTNET_GAUSS, _lib.RR_POINT_GAUSS, 2, False),
    "listnet_uq": (_lib.RR_LIST_LISTNET_UQ, _lib.RR_POINT_NONE, 1, False),
    "dirichlet_uq": (_lib.RR_LIST_DIRICHLET_UQ, _lib.RR_POINT_NONE, 1, False),
}


def task_loss_step(list_term, point_term, out2d, targets, seg, Q, max_len, coef, n_queries, n_cands, dout2d, terms=None,
                   counter=None):
    """One rr_task_loss_step_f32 launch on out2d [M, n_cols] (unit column stride): returns the [1] loss, fills dout2d."""
    dev = out2d.device
    loss, part = _f1(dev), torch.empty(2 * max(Q, 1), dtype=torch.float32, device=dev)
    a = _lib.TaskLossArgs(list_term=list_term, point_term=point_term, out=out2d.data_ptr(), ld_out=out2d.stride(0),
                          n_cols=out2d.shape[1], targets=targets.data_ptr(), seg_off=seg.data_ptr(), Q=Q, max_len=max_len,
                          coef=float(coef), n_queries=int(n_queries), n_cands=int(n_cands), loss=loss.data_ptr(),
                          terms=None if terms is None else terms.data_ptr(), dout=dout2d.data_ptr(), ld_dout=dout2d.stride(0),
                          partial=part.data_ptr(), counter=(_counter(dev) if counter is None else counter).data_ptr())
    check(lib().rr_task_loss_step_f32(C.byref(a), stream()), "rr_task_loss_step_f32")
    return loss


class _TaskStepFn(torch.autograd.Function):
    """A composite task type's loss over the head's output, loss and d loss / d out in one launch (FusedStep): the forward
    keeps d loss / d out for an upstream gradient of one; `backward(loss)` with the library's constant one hands it out, any
    other upstream gradient multiplies it."""

    @staticmethod
    def forward(ctx, out, targets, seg, Q, max_len, list_term, point_term, coef, n_queries, n_cands, scalar):
        o = out.detach()
        o2 = o if o.dim() == 2 else o.unsqueeze(1)
        dout = torch.empty(tuple(out.shape), dtype=torch.float32, device=o.device)
        loss = task_loss_step(list_term, point_term, o2, targets, seg, Q, max_len, coef, n_queries, n_cands,
                              dout if dout.dim() == 2 else dout.unsqueeze(1))
        ctx.dout = dout
        return loss.reshape(()) if scalar else loss

    @staticmethod
    def backward(ctx, g):
        d = ctx.dout
        if d is None:
            raise RuntimeError("reactranker_amd.loss: the gradient of this fused loss was already handed out (a second backward "
                               "through a retained graph); set loss.FusedStep.enabled = False for that")
        if _is_unit(g):                                  # handed out once, without a reference left behind: autograd keeps it
            ctx.dout = None                              # as the leaf's .grad instead of cloning it
            FusedStep.hits += 1
        else:
            d = d * g.reshape(()).float()
        return (d,) + (None,) * 10


def task_step_loss(task_type, output, scope, targets, gpu, coef=0.0, norm=None):
    """batch_loss of one of TASK_STEPS through rr_task_loss_step_f32, or None where the entry does not apply (FusedStep off,
    no gradient wanted, an output layout it does not know): the caller then forms the loss term by term.  norm: the counts
    to divide by (mapping with `queries` and `cands`), None = this batch's own."""
    spec = TASK_STEPS.get(task_type)
    if spec is None or not FusedStep.enabled or not (torch.is_tensor(output) and output.requires_grad and torch.is_grad_enabled()):
        return None
    list_term, point_term, cols, scalar = spec
    if output.dtype != torch.float32 or not output.is_cuda:
        return None
    if cols == 1:
        if task_type in ("listnet_uq", "dirichlet_uq"):
            ok = output.dim() == 1
        else:
            ok = output.dim() == 1 or (output.dim() == 2 and output.shape[1] == 1)
    elif task_type in ("mledis_gaussian", "listnetdis_gauss"):   # their list term reads columns 0, 1 of cat(out[:, 0::2], out[:, 1::2])
        ok = output.dim() == 2 and output.shape[1] == 2
    else:
        ok = output.dim() == 2 and output.shape[1] >= 2
    if ok and output.dim() == 2:
        ok = (output.stride(1) == 1 or output.shape[1] == 1) and output.stride(0) >= output.shape[1]
    elif ok:
        ok = output.stride(0) >= 1
    if not ok:
        return None
    scope, seg, total, max_len, t = _prep(output, scope, targets, gpu)
    nq, nc = (len(scope), total) if norm is None else (int(norm["queries"]), int(norm["cands"]))
    return _TaskStepFn.apply(output, t, seg, len(scope), max_len, list_term, point_term, coef, nq, nc, scalar)


# ---------------------------------------------------------------------------------------------- the pairwise trainer's remaining losses
# (loss_sum over all C x C entries of every query, csrc/pairwise.hip, through _WindowFn)
def betanet_loss(y_pred, scope, targets, alpha0: float = 100.0, gpu: int = None):
    """The Beta-density KL loss of `beta_dis_train_loop` over a window of queries (reference train/train_pairwise.py:189-226):
    tau = sigmoid(targets), pi = sigmoid(score); per query the sum over ALL C x C entries of exp(lt) * (lt - lp), where lt / lp
    are the log densities of Beta(alpha0 * tau_j / (tau_i + tau_j), alpha0 * tau_i / (tau_i + tau_j)) and of the same with pi,
    both at tau_j / (tau_i + tau_j).

    Returns (loss_sum, pairs) like ranknet_loss: loss_sum is differentiable (the trainer divides by the window's pairs and calls
    backward); pairs = sum of C * C - C (:198), an int64 device scalar.  `y_pred` may be [M] or [M, k] (first column)."""
    y_pred = _first_column(y_pred)
    if not alpha0 > 0:
        raise ValueError("betanet_loss: alpha0 must be positive")
    scope, seg, total, max_len, t = _prep(y_pred, scope, targets, gpu)
    return _WindowFn.apply("betanet", y_pred, t, seg, len(scope), max_len, (float(alpha0),), 1.0)


def beta_evidential_loss(y_pred, scope, targets, coef: float, gpu: int = None):
    """The evidential pair loss of `beta_evi_train_loop` (reference train/train_pairwise.py:276-307): the raw scores are the
    evidence (they must be positive - a softplus head; the reference gives NaN otherwise, and so does this), T = tau_j /
    (tau_i + tau_j), P = p_j / (p_i + p_j); per query the sum over all C x C entries of (T1-P1)^2 + (T2-P2)^2 + (P1 (1-P1) +
    P2 (1-P2)) / (p_i + p_j + 1) + coef * 2 |ln(T1 / P1) (p_j - 1)|.  coef: the annealing coefficient (`annealing_coef`).
    Returns (loss_sum, pairs) like betanet_loss."""
    y_pred = _first_column(y_pred)
    scope, seg, total, max_len, t = _prep(y_pred, scope, targets, gpu)
    return _WindowFn.apply("beta_evidential", y_pred, t, seg, len(scope), max_len, (float(coef),), 1.0)


def sq_pairs(scope) -> int:
    """sum of C * C - C over the queries of a window: the normaliser of the two losses above (train_pairwise.py:198, 274)."""
    return int(sum(int(c) * int(c) - int(c) for c in scope))


class _PairMseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, targets):
        B = y.shape[0]
        loss = _f1(y.device)
        part = torch.empty(int(lib().rr_pair_partial_count(B)), dtype=torch.float64, device=y.device)
        check(lib().rr_pair_softmax_mse_fwd_f32(ptr(y), y.stride(0), ptr(targets), targets.stride(0), B, ptr(loss), ptr(part),
                                                stream()), "rr_pair_softmax_mse_fwd_f32")
        ctx.save_for_backward(y, targets)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        y, targets = ctx.saved_tensors
        B = y.shape[0]
        g = g.reshape(-1).contiguous().float()
        dy = torch.empty(B, 2, dtype=torch.float32, device=y.device)
        check(lib().rr_pair_softmax_mse_bwd_f32(ptr(y), y.stride(0), ptr(targets), targets.stride(0), B, ptr(g), ptr(dy), 2,
                                                stream()), "rr_pair_softmax_mse_bwd_f32")
        return dy, None


def _pair_rows(x, what, device=None):
    t = torch.as_tensor(x, dtype=torch.float32)
    if device is not None and t.device != device:
        t = t.to(device)
    if t.dim() != 2 or t.shape[1] != 2:
        raise RuntimeError(f"{what}: expected shape [B, 2], got {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) < 2:
        t = t.contiguous()
    return t


def pair_softmax_mse(y_pred, targets):
    """The loss `baseline_pairwise_training_loop` trains on (reference train/train_pairwise.py:33-59): targets [B, 2] ->
    target_p = softmax over the pair, pred_p = y_pred / sum(y_pred), loss = mean_b sum_k (target_p - pred_p)^2.  (The loop's
    variance, KL and annealing terms are computed there and then left out of the loss, :59.)  0-d, differentiable."""
    _lib.require_cuda(y_pred, "y_pred")
    y = _pair_rows(y_pred, "y_pred")
    t = _pair_rows(targets, "targets", y.device)
    if t.shape[0] != y.shape[0]:
        raise RuntimeError("pair_softmax_mse: y_pred and targets hold different numbers of pairs")
    return _PairMseFn.apply(y, t)
