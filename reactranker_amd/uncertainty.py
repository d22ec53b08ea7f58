"""Predictive uncertainty of a trained ranker: T score samples per candidate from MC dropout or from an ensemble of
checkpoints - or the (mean, variance) a distributional head predicts in ONE forward - their statistics on the device, and
whether the uncertainty tracks the error.

The reference authors had this tooling (run_mc_model / run_ensemble_model, spearman_coef, erro_confidence); only its
bytecode names survive (SURVEY.md:35-41), so what follows is defined here and is not a parity port:

  - a sample is one full forward: train mode with a pinned dropout stream (MC dropout) or one checkpoint in eval mode
    (ensemble).  Column 0 of every sample goes into one [T, M] device buffer, with no host round trip between samples.
  - rr_mc_sample_stats_f32 turns the buffer into per-candidate mean / std / p_top1 / mean rank and per-query statistics
    (include/reactranker_hip.h) in one launch.
  - rr_uq_calibration_f64 gives the Spearman correlation of error and uncertainty and the error-confidence curve (MAE and
    RMSE after removing the most uncertain fraction).  Sorting stays torch plumbing (torch.sort(stable=True)).

A model whose head emits a distribution per candidate (heads 3, 4, 6: evidential_ranking, the Gaussian task types, the
NIG ones) needs no samples: rr_analytic_rank_stats_f32 turns one eval-mode forward into the same statistics analytically
under independent Gaussians (analytic_stats / distribution_predict / method='distribution').

Batches have the tuple form of eval.evaluate_top_scores: (r_batch, p_batch, scope, targets, add_features).
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Sequence

import numpy as np
import torch

from . import eval as E
from ._lib import check, lib, ptr, stream
from .loss import _prep
from .utils import load_checkpoint

NQSTATS = 4            # RR_UQ_NQSTATS (include/reactranker_hip.h)
CAL_BLOCK = 256        # RR_UQ_CAL_BLOCK
DEFAULT_FRACTIONS = tuple(i / 10 for i in range(10))
QSTAT_NAMES = ("top1_entropy", "p_top1_of_target_top1", "p_top1_of_mean_top1", "mean_std")
MAX_NODES = 128        # RR_UQ_MAX_NODES
MOMENT_KINDS = {"gaussian": 0, "log_variance": 1, "nig": 2}                 # rr_moment_kind
MOMENT_COLUMNS = {"gaussian": 2, "log_variance": 2, "nig": 4}
MOMENT_KIND_OF_HEAD = {3: "gaussian", 4: "gaussian", 6: "nig"}            # rr_head -> kind; head 5's mean is no score
METHODS = ("MC_dropout", "ensemble", "distribution")

_M64 = (1 << 64) - 1
_GAMMA = 0x9E3779B97F4A7C15


def _mix64(x: int) -> int:
    """splitmix64's output function (Steele, Lea & Flood, OOPSLA 2014) on a 64-bit word."""
    x &= _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sample_seed(seed: int, t: int) -> int:
    """Dropout seed of MC sample `t` (0, 1, ...) under the run seed `seed`: the top 62 bits of
    mix64(mix64(seed mod 2^64) + (t + 1) * 0x9E3779B97F4A7C15 mod 2^64), mix64 being splitmix64's finaliser.
    Pure Python, so the same (seed, t) gives the same stream on every machine and the torch RNG is never touched."""
    t = int(t)
    if t < 0:
        raise ValueError(f"sample index must be >= 0 (got {t})")
    return _mix64(_mix64(int(seed)) + (t + 1) * _GAMMA) >> 2


def _nonempty(x: torch.Tensor) -> torch.Tensor:
    """x, or a one-element stand-in when x has no elements (never hand the library a NULL pointer)."""
    return x if x.numel() > 0 else torch.zeros(1, dtype=x.dtype, device=x.device)


def sample_stats(samples: torch.Tensor, scope, targets, gpu: int = None) -> dict:
    """Statistics of the T score samples `samples` [T, M] (row t = sample t of every candidate) of the lists described by
    `scope` (candidates per query), `targets` [M] - one rr_mc_sample_stats_f32 launch.

    Returns a dict of device tensors: mean, std (ddof = 1), p_top1 (share of samples in which the candidate is its list's
    first maximum), mean_rank (1-based, stable descending order) - each [M] float32 - and qstats [Q, 4] float64: the entropy
    of p_top1 over the list, p_top1 of the target's first maximum, p_top1 of the first maximum of `mean`, the list's mean
    std (QSTAT_NAMES).  T < 2 or a list longer than 8,192 raises (the library's status)."""
    if samples.dim() != 2:
        raise ValueError(f"samples must be [T, M] (got shape {tuple(samples.shape)})")
    T, M = int(samples.shape[0]), int(samples.shape[1])
    row = samples[0] if T > 0 else samples.new_empty(M)
    scope, seg, total, max_len, t = _prep(row, scope, targets, gpu)
    x = samples if samples.dtype == torch.float32 else samples.float()
    if x.stride(1) != 1 or x.stride(0) < M:
        x = x.contiguous()
    dev = x.device
    outs = [torch.empty(max(total, 1), dtype=torch.float32, device=dev) for _ in range(4)]
    qstats = torch.empty(max(len(scope), 1), NQSTATS, dtype=torch.float64, device=dev)
    check(lib().rr_mc_sample_stats_f32(ptr(_nonempty(x)), max(x.stride(0), 1), T, ptr(_nonempty(t)), ptr(seg),
                                       len(scope), max_len, *[ptr(o) for o in outs], ptr(qstats), stream()),
          "rr_mc_sample_stats_f32")
    mean, std, p_top1, mean_rank = (o[:total] for o in outs)
    return dict(mean=mean, std=std, p_top1=p_top1, mean_rank=mean_rank, qstats=qstats[:len(scope)])


def _first_column(out: torch.Tensor) -> torch.Tensor:
    return out[:, 0] if out.dim() > 1 else out


def mc_dropout_predict(model, batches: Iterable, n_samples: int, seed: int = 0, gpu: int = None) -> List[dict]:
    """MC dropout: per batch, `n_samples` train-mode forwards under no_grad, sample t with
    model.dropout_seed = sample_seed(seed, t) (the same T streams serve every batch), column 0 of each into one [T, M]
    device buffer, then sample_stats.  Returns one sample_stats dict per batch with queries, plus `samples` (the buffer).
    model.training and model.dropout_seed are restored afterwards; torch's global RNG is not used."""
    T = int(n_samples)
    if T < 2:
        raise ValueError(f"MC dropout needs n_samples >= 2 (got {n_samples})")
    was_training, old_seed = model.training, getattr(model, "dropout_seed", None)
    results = []
    try:
        model.train()
        with torch.no_grad():
            for r_batch, p_batch, scope, targets, add_features in batches:
                if len(scope) == 0:                        # an empty shard, as in eval._eval_stats
                    continue
                buf = None
                for t in range(T):
                    model.dropout_seed = sample_seed(seed, t)
                    col = _first_column(model(r_batch, p_batch, gpu=gpu, add_features=add_features))
                    if buf is None:
                        buf = torch.empty(T, col.shape[0], dtype=torch.float32, device=col.device)
                    buf[t].copy_(col)
                results.append(dict(sample_stats(buf, scope, targets, gpu), samples=buf))
    finally:
        model.train(was_training)
        model.dropout_seed = old_seed
    return results


def ensemble_predict(model, checkpoints: Sequence[str], batches: Iterable, gpu: int = None) -> List[dict]:
    """Deep ensemble: every checkpoint (utils.save_checkpoint files) is loaded into `model` in turn and run in eval mode over
    all batches; member t is sample t of the same [T, M] buffers and statistics as mc_dropout_predict.  The model keeps the
    last checkpoint's weights; model.training is restored."""
    paths = list(checkpoints)
    if len(paths) < 2:
        raise ValueError(f"an ensemble needs at least 2 checkpoints (got {len(paths)})")
    batches = [b for b in batches if len(b[2]) > 0]
    T = len(paths)
    bufs = [None] * len(batches)
    was_training = model.training
    try:
        model.eval()
        with torch.no_grad():
            for t, path in enumerate(paths):
                load_checkpoint(path, model, map_location="cpu")
                for k, (r_batch, p_batch, scope, targets, add_features) in enumerate(batches):
                    col = _first_column(model(r_batch, p_batch, gpu=gpu, add_features=add_features))
                    if bufs[k] is None:
                        bufs[k] = torch.empty(T, col.shape[0], dtype=torch.float32, device=col.device)
                    bufs[k][t].copy_(col)
    finally:
        model.train(was_training)
    return [dict(sample_stats(buf, b[2], b[3], gpu), samples=buf) for buf, b in zip(bufs, batches)]


def _check_nodes(n_nodes) -> int:
    n = int(n_nodes)
    if n != n_nodes or not (1 <= n <= MAX_NODES):
        raise ValueError(f"n_nodes must be an integer in [1, {MAX_NODES}] (got {n_nodes!r})")
    return n


def _check_kind(kind) -> str:
    if kind not in MOMENT_KINDS:
        raise ValueError(f"kind must be one of {sorted(MOMENT_KINDS)} (got {kind!r})")
    return kind


def quadrature(n_nodes: int = 32):
    """(nodes, weights), float64: the `n_nodes` probabilists' Gauss-Hermite nodes (numpy.polynomial.hermite_e.hermegauss)
    and their weights normalised to sum 1, so that sum_n w_n f(x_n) ~ E f(X) for X ~ N(0, 1)."""
    n = _check_nodes(n_nodes)
    x, w = np.polynomial.hermite_e.hermegauss(n)
    return np.ascontiguousarray(x, np.float64), np.ascontiguousarray(w / w.sum(), np.float64)


_QUAD_CACHE = {}


def _device_quadrature(n: int, dev: torch.device):
    key = (n, str(dev))
    if key not in _QUAD_CACHE:
        x, w = quadrature(n)
        _QUAD_CACHE[key] = (torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev))
    return _QUAD_CACHE[key]


def _check_columns(output, kind: str) -> None:
    need = MOMENT_COLUMNS[kind]
    if output.dim() != 2 or output.shape[1] < need:
        raise ValueError(f"kind {kind!r} reads {need} columns of a [M, k] output (got shape {tuple(output.shape)})")


def analytic_stats(output: torch.Tensor, scope, targets, kind: str, n_nodes: int = 32, gpu: int = None) -> dict:
    """The statistics of sample_stats from ONE forward of a distributional head, analytically under independent Gaussians -
    one rr_analytic_rank_stats_f32 call.  `output` [M, k] is the model's eval-mode output; `kind` says how a row gives the
    predictive mean and variance: 'gaussian' (mean, variance: heads 3 and 4), 'log_variance' (mean, log variance), 'nig'
    (mu, v, alpha, beta: head 6; variance = aleatoric + epistemic).  A strided [M, k] view (unit column stride) is read in
    place.

    Returns a dict of device tensors: mean (column 0), std, p_top1 (Gauss-Hermite with `n_nodes` nodes), mean_rank (the exact
    expected rank) - each [M] float32 - qstats [Q, 4] float64 (QSTAT_NAMES) and mass [Q] float64 = the sum of p_top1 over
    the list, which is 1 when the quadrature resolves the list and is deliberately not normalised away (its limits:
    include/reactranker_hip.h); for 'nig' also aleatoric_std and epistemic_std.  A non-finite mean or a variance that is not
    positive and finite raises ValueError."""
    n = _check_nodes(n_nodes)
    kind = _check_kind(kind)
    _check_columns(output, kind)
    scope, seg, total, max_len, t = _prep(output[:, 0], scope, targets, gpu)
    x = output if output.dtype == torch.float32 else output.float()
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    dev = x.device
    nodes, weights = _device_quadrature(n, dev)
    nig = kind == "nig"
    outs = [torch.empty(max(total, 1), dtype=torch.float32, device=dev) for _ in range(6 if nig else 4)]
    qstats = torch.empty(max(len(scope), 1), NQSTATS, dtype=torch.float64, device=dev)
    mass = torch.empty(max(len(scope), 1), dtype=torch.float64, device=dev)
    check(lib().rr_analytic_rank_stats_f32(ptr(_nonempty(x)), max(x.stride(0), 1), MOMENT_KINDS[kind], ptr(_nonempty(t)),
                                           ptr(seg), len(scope), max_len, ptr(nodes), ptr(weights), n,
                                           *[ptr(o) for o in outs], *([] if nig else [None, None]), ptr(qstats), ptr(mass),
                                           stream()), "rr_analytic_rank_stats_f32")
    outs = [o[:total] for o in outs]
    mean, std = outs[0], outs[1]
    if not bool((torch.isfinite(mean) & torch.isfinite(std) & (std > 0)).all()):
        raise ValueError(f"kind {kind!r}: the output holds a non-finite mean or a variance that is not positive and finite")
    res = dict(mean=mean, std=std, p_top1=outs[2], mean_rank=outs[3], qstats=qstats[:len(scope)], mass=mass[:len(scope)])
    if nig:
        res.update(aleatoric_std=outs[4], epistemic_std=outs[5])
    return res


def _kind_of(model, kind) -> str:
    if kind is not None:
        return _check_kind(kind)
    head = model.ffn.head()
    if head not in MOMENT_KIND_OF_HEAD:
        raise ValueError(f"the model's head ({model.ffn.task_type!r}, head {head}) predicts no (mean, variance) that "
                         f"method 'distribution' knows how to read; pass the `kind` argument ({sorted(MOMENT_KINDS)}) if its "
                         "output does hold one")
    return MOMENT_KIND_OF_HEAD[head]


def distribution_predict(model, batches: Iterable, kind: str = None, n_nodes: int = 32, gpu: int = None) -> List[dict]:
    """Single-forward uncertainty: per batch one eval-mode forward under no_grad, then analytic_stats of its output.
    `kind=None` takes the kind from the model's head (MOMENT_KIND_OF_HEAD); any other head raises ValueError.  Returns one
    analytic_stats dict per batch with queries, plus `output` (the forward's [M, k] output).  model.training is restored;
    no RNG is used."""
    n = _check_nodes(n_nodes)
    kind = _kind_of(model, kind)
    was_training = model.training
    results = []
    try:
        model.eval()
        with torch.no_grad():
            for r_batch, p_batch, scope, targets, add_features in batches:
                if len(scope) == 0:
                    continue
                out = model(r_batch, p_batch, gpu=gpu, add_features=add_features)
                results.append(dict(analytic_stats(out, scope, targets, kind, n, gpu), output=out))
    finally:
        model.train(was_training)
    return results


def _check_fractions(fractions) -> List[float]:
    fr = [float(f) for f in fractions]
    bad = [f for f in fr if not (0.0 <= f < 1.0)]
    if bad:
        raise ValueError(f"fractions must lie in [0, 1) (got {bad})")
    return fr


def uncertainty_calibration(pred, target, uncertainty, fractions=DEFAULT_FRACTIONS) -> dict:
    """Does `uncertainty` track the error |pred - target| (formed once in float32; this array is both sorted and ranked)?

    Returns dict(spearman = Spearman rho of error and uncertainty with tie-averaged ranks (scipy.stats.spearmanr; NaN when
    either is constant), fractions, and per fraction f - with the floor(f * n) most uncertain rows removed (stable
    descending order of the uncertainty, ties by row) - kept (rows left), mae and rmse of what is left).  One
    rr_uq_calibration_f64 call (two launches) after two stable torch sorts; inputs on the CPU are moved to the current
    GPU."""
    fr = _check_fractions(fractions)
    p, y, u = (torch.as_tensor(v) for v in (pred, target, uncertainty))
    p, y, u = p.reshape(-1), y.reshape(-1), u.reshape(-1)
    n = int(p.numel())
    if y.numel() != n or u.numel() != n:
        raise ValueError(f"pred, target and uncertainty differ in length ({n}, {y.numel()}, {u.numel()})")
    if n == 0:
        raise ValueError("calibration needs at least one row")
    dev = next((v.device for v in (p, y, u) if v.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    err = (p.to(dev, torch.float32) - y.to(dev, torch.float32)).abs()
    unc = u.to(dev, torch.float32).contiguous()
    if bool(torch.isnan(err).any()) or bool(torch.isnan(unc).any()):
        raise ValueError("calibration of NaN errors or uncertainties is undefined")
    order_err = torch.sort(err, stable=True).indices
    order_unc = torch.sort(unc, stable=True).indices
    fr_dev = torch.tensor(fr if fr else [0.0], dtype=torch.float64, device=dev)
    nb = (n + CAL_BLOCK - 1) // CAL_BLOCK
    ws = torch.empty(nb * (3 + 2 * len(fr)), dtype=torch.float64, device=dev)
    out = torch.empty(1 + 3 * len(fr), dtype=torch.float64, device=dev)
    check(lib().rr_uq_calibration_f64(ptr(err), ptr(unc), ptr(order_err), ptr(order_unc), n, ptr(fr_dev), len(fr), ptr(ws),
                                      C.c_size_t(ws.numel() * 8), ptr(out), stream()), "rr_uq_calibration_f64")
    o = out.cpu().numpy()
    curve = o[1:].reshape(len(fr), 3)
    return dict(spearman=float(o[0]), fractions=np.asarray(fr, np.float64), kept=curve[:, 0].astype(np.int64),
                mae=curve[:, 1].copy(), rmse=curve[:, 2].copy())


def _standardizer(scaler, target_name):
    """The trainers' target transform (train_listwise.standardize_targets with normalize_target=True) for a checkpoint's
    scaler: sign * (y - mean) / std, the sign flipped unless 'lgk'; identity without a scaler or for 'lgk_bi'."""
    if scaler is None or scaler.get("means") is None or target_name in (None, "lgk_bi"):
        return lambda y: y
    mean, std = float(scaler["means"]), float(scaler["stds"])
    sign = 1.0 if target_name == "lgk" else -1.0
    return lambda y: sign * (y - mean) / std


def _scaler_of(path):
    return torch.load(path, map_location="cpu", weights_only=False).get("data_scaler")


def evaluate_uncertainty(model, test_batches: Sequence[dict], path_checkpoints, gpu: int, method: str = "MC_dropout",
                         n_samples: int = 30, seed: int = 0, target_name: str = "ea",
                         fractions=DEFAULT_FRACTIONS, kind: str = None, n_nodes: int = 32) -> dict:
    """Test-set uncertainty of a trained model - what a loop of T main.test(..., task_type='MC_dropout') calls left to
    the user.  `test_batches` are the dicts main.test takes (r, p, scope, targets, add).  method 'MC_dropout': one
    checkpoint path, n_samples dropout samples from `seed`; 'ensemble': a list of checkpoint paths, one member each (their
    scalers must agree); 'distribution': one checkpoint path of a model with a distributional head, ONE eval-mode forward
    per batch read as `kind` (None: from the head, MOMENT_KIND_OF_HEAD) with `n_nodes` quadrature nodes (analytic_stats).
    Targets are standardised as the trainers do, so errors are in model units.

    Returns dict(top_scores = evaluate_top_scores' triple (top-1, predicted top-25 % in the target top-25 %, the target's
    top-1 in the predicted top-25 %) of the MEAN scores, qstats = the mean over queries of each per-query statistic
    (QSTAT_NAMES), calibration = uncertainty_calibration(mean, targets, std), and the per-candidate arrays of every query
    in order: mean, std, p_top1, mean_rank, targets (standardised), scope).  'distribution' adds mass_worst = the largest
    |mass - 1| over the queries (analytic_stats' quadrature diagnostic) and, for kind 'nig', aleatoric_std and
    epistemic_std."""
    if method == "MC_dropout":
        if not isinstance(path_checkpoints, (str, bytes)) and hasattr(path_checkpoints, "__len__"):
            raise ValueError("method 'MC_dropout' takes one checkpoint path")
        T = int(n_samples)
        if T < 2:
            raise ValueError(f"MC dropout needs n_samples >= 2 (got {n_samples})")
        paths = [path_checkpoints]
    elif method == "ensemble":
        paths = list(path_checkpoints)
        if len(paths) < 2:
            raise ValueError(f"an ensemble needs at least 2 checkpoints (got {len(paths)})")
    elif method == "distribution":
        if not isinstance(path_checkpoints, (str, bytes)) and hasattr(path_checkpoints, "__len__"):
            raise ValueError("method 'distribution' takes one checkpoint path")
        n_nodes = _check_nodes(n_nodes)
        if kind is not None:
            _check_kind(kind)
        paths = [path_checkpoints]
    else:
        raise ValueError("method must be " + ", ".join(repr(m) for m in METHODS[:-1]) + f" or {METHODS[-1]!r} (got {method!r})")
    _check_fractions(fractions)
    scalers = [_scaler_of(p) for p in paths]
    if any(s != scalers[0] for s in scalers[1:]):
        raise ValueError("the ensemble's checkpoints carry different target scalers")
    f = _standardizer(scalers[0], target_name)
    batches = []
    for b in test_batches:
        y = np.asarray(torch.as_tensor(b["targets"]).cpu(), np.float64).reshape(-1)
        batches.append((b["r"], b["p"], b["scope"], torch.tensor(f(y), dtype=torch.float32), b.get("add")))
    model = model.cuda(gpu)
    if method == "MC_dropout":
        load_checkpoint(paths[0], model, map_location="cpu")
        res = mc_dropout_predict(model, batches, T, seed=seed, gpu=gpu)
    elif method == "distribution":
        load_checkpoint(paths[0], model, map_location="cpu")
        res = distribution_predict(model, batches, kind=kind, n_nodes=n_nodes, gpu=gpu)
    else:
        res = ensemble_predict(model, paths, batches, gpu=gpu)
    kept = [b for b in batches if len(b[2]) > 0]
    if not res:
        raise ValueError("no queries to evaluate")
    stats = torch.cat([E.ranking_stats(r["mean"], b[2], b[3], gpu, 0.25)[0] for r, b in zip(res, kept)], 0)
    m = stats.mean(dim=0).cpu().numpy()
    keys = ("mean", "std", "p_top1", "mean_rank") + tuple(k for k in ("aleatoric_std", "epistemic_std") if k in res[0])
    cat = {k: torch.cat([r[k] for r in res]) for k in keys}
    if method == "distribution":
        cat["mass_worst"] = float(torch.cat([r["mass"] for r in res]).sub(1.0).abs().max())
    targets = torch.cat([b[3].reshape(-1) for b in kept]).to(cat["mean"].device)
    qstats = torch.cat([r["qstats"] for r in res], 0)
    return dict(top_scores=(float(m[0]), float(m[11]), float(m[8])),
                qstats=qstats.mean(dim=0).cpu().numpy(),
                calibration=uncertainty_calibration(cat["mean"], targets, cat["std"], fractions),
                targets=targets, scope=[int(c) for b in kept for c in b[2]], **cat)
