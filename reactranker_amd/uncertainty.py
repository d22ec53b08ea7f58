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

Whether the uncertainty has the right SIZE, and whether p_top1 means what it says, is the calibration part:
rr_gauss_calibration_f64 behind probabilistic_calibration / fit_sigma_scale (NLL, CRPS, PIT histogram, a fitted sigma scale),
rr_top1_sets_f32 behind top1_sets (per-list rank, probability mass ahead, prediction set and top-1 statistics), and
conformal_threshold / top1_calibration / evaluate_calibration on top of them.

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


# ------------------------------------------------------------------------------------------------ calibration
GAUSS_CAL_NSUMS = 8    # RR_GAUSS_CAL_NSUMS
GAUSS_CAL_MAX_BINS = 64
TOP1_NSTATS = 9        # RR_TOP1_NSTATS
TOP1_STAT_NAMES = ("hit", "confidence", "p_of_true_top", "rank_of_true_top", "brier", "conformity_score", "set_size", "covered",
                   "mass")


def _gauss_sums(pred, target, std, n_bins: int, sigma_scale: float) -> np.ndarray:
    """One rr_gauss_calibration_f64 call: the 8 raw sums and the n_bins PIT counts, float64 on the host."""
    nb_ = int(n_bins)
    if nb_ != n_bins or not (1 <= nb_ <= GAUSS_CAL_MAX_BINS):
        raise ValueError(f"n_bins must be an integer in [1, {GAUSS_CAL_MAX_BINS}] (got {n_bins!r})")
    s = float(sigma_scale)
    if not (s > 0.0 and np.isfinite(s)):
        raise ValueError(f"sigma_scale must be positive and finite (got {sigma_scale!r})")
    p, y, u = (torch.as_tensor(v).reshape(-1) for v in (pred, target, std))
    n = int(p.numel())
    if y.numel() != n or u.numel() != n:
        raise ValueError(f"pred, target and std differ in length ({n}, {y.numel()}, {u.numel()})")
    if n == 0:
        raise ValueError("calibration needs at least one row")
    dev = next((v.device for v in (p, y, u) if v.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    p, y, u = (v.to(dev, torch.float32).contiguous() for v in (p, y, u))
    nv = GAUSS_CAL_NSUMS + nb_
    ws = torch.empty(((n + CAL_BLOCK - 1) // CAL_BLOCK) * nv, dtype=torch.float64, device=dev)
    out = torch.empty(nv, dtype=torch.float64, device=dev)
    check(lib().rr_gauss_calibration_f64(ptr(p), ptr(u), ptr(y), n, s, nb_, ptr(ws), C.c_size_t(ws.numel() * 8), ptr(out),
                                         stream()), "rr_gauss_calibration_f64")
    return out.cpu().numpy()


def probabilistic_calibration(pred, target, std, n_bins: int = 20, sigma_scale: float = 1.0) -> dict:
    """Does `std` have the right SIZE?  The predictive distribution of row i is N(pred_i, (sigma_scale * std_i)^2); one
    rr_gauss_calibration_f64 call (two launches) gives the raw float64 sums and this forms the means over the VALID rows
    (finite pred and target, finite positive std):

      n_valid, n_invalid
      nll          0.5 ln 2 pi + mean ln sigma + mean z^2 / 2,   z = (target - pred) / sigma
      crps         mean of sigma (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt pi)
      z_mean, z2_mean    0 and 1 for a calibrated Gaussian
      sharpness    sqrt(mean sigma^2);   rmse = sqrt(mean (target - pred)^2): equal when calibrated
      pit_hist     [n_bins] counts of the probability integral transform Phi(z): flat when calibrated
      expected, observed   j / n_bins and the share of the rows with a PIT below it, j = 1..n_bins (the reliability curve)
      miscalibration_area  mean_j |observed_j - expected_j|
      interval_levels, interval_coverage   (even n_bins) the central intervals of level 2k / n_bins, k = 1..n_bins / 2, and
                   the share of the rows inside (bins n_bins / 2 - k ... n_bins / 2 + k - 1)

    Raises ValueError when no row is valid.  Inputs on the CPU are moved to the current GPU."""
    o = _gauss_sums(pred, target, std, n_bins, sigma_scale)
    nb_ = int(n_bins)
    n = float(o[0])
    if n < 1:
        raise ValueError(f"no valid row: all {int(o[1])} have a non-finite mean or target or a std that is not positive and finite")
    hist = o[GAUSS_CAL_NSUMS:].copy()
    expected = np.arange(1, nb_ + 1, dtype=np.float64) / nb_
    observed = np.cumsum(hist) / n
    res = dict(n_valid=int(o[0]), n_invalid=int(o[1]), sigma_scale=float(sigma_scale),
               nll=0.5 * float(np.log(2.0 * np.pi)) + o[4] / n + 0.5 * o[3] / n, crps=o[7] / n, z_mean=o[2] / n,
               z2_mean=o[3] / n, sharpness=float(np.sqrt(o[5] / n)), rmse=float(np.sqrt(o[6] / n)),
               pit_hist=hist.astype(np.int64), expected=expected, observed=observed,
               miscalibration_area=float(np.mean(np.abs(observed - expected))))
    if nb_ % 2 == 0:
        h = nb_ // 2
        ks = np.arange(1, h + 1)
        res["interval_levels"] = 2.0 * ks / nb_
        res["interval_coverage"] = np.array([hist[h - k:h + k].sum() / n for k in ks])
    return {k: float(v) if isinstance(v, np.floating) else v for k, v in res.items()}


def fit_sigma_scale(pred, target, std) -> float:
    """The scalar s that minimises the Gaussian negative log-likelihood of N(pred, (s std)^2) over the valid rows, in closed
    form: sqrt(mean z^2) at sigma_scale = 1.  One rr_gauss_calibration_f64 call."""
    o = _gauss_sums(pred, target, std, 1, 1.0)
    if o[0] < 1:
        raise ValueError("no valid row to fit a sigma scale on")
    return float(np.sqrt(o[3] / o[0]))


def top1_sets(p_top1: torch.Tensor, scope, targets, tau: float, gpu: int = None) -> dict:
    """Per-list calibration and prediction sets of a top-1 probability - one rr_top1_sets_f32 launch.  `p_top1` [M] (device;
    a strided column is read in place) are non-negative and sum to about 1 per list of `scope`; `tau` >= 0 (inf allowed).

    Returns a dict of device tensors: rank [M] int32 (1-based, stable descending p, ties by list position), before [M] float64
    (the probability mass ranked strictly ahead of the candidate, summed in ascending position), in_set [M] bool
    (before <= tau: the smallest prefix of the predicted order whose mass ahead of its last member is still <= tau) and
    stats [Q, 9] float64 (TOP1_STAT_NAMES; the true top is the first maximum of the targets).  covered == (E <= tau)
    exactly.  A NaN or negative probability or a NaN target raises ValueError."""
    tau = float(tau)
    if not tau >= 0.0:
        raise ValueError(f"tau must be >= 0 (got {tau!r})")
    if p_top1.dim() != 1:
        raise ValueError(f"p_top1 must be [M] (got shape {tuple(p_top1.shape)})")
    scope, seg, total, max_len, t = _prep(p_top1, scope, targets, gpu, "p_top1")
    p = p_top1.detach()
    p = p if p.dtype == torch.float32 else p.float()
    if total and (not bool((p >= 0).all()) or bool(torch.isnan(t).any())):
        raise ValueError("top1_sets: p_top1 holds a NaN or a negative value, or the targets hold a NaN")
    dev, Q, m = p.device, len(scope), max(total, 1)
    rank = torch.empty(m, dtype=torch.int32, device=dev)
    before = torch.empty(m, dtype=torch.float64, device=dev)
    in_set = torch.empty(m, dtype=torch.uint8, device=dev)
    stats = torch.empty(max(Q, 1), TOP1_NSTATS, dtype=torch.float64, device=dev)
    check(lib().rr_top1_sets_f32(ptr(_nonempty(p)), max(p.stride(0), 1) if total else 1, ptr(_nonempty(t)), ptr(seg), Q, max_len,
                                 tau, ptr(rank), ptr(before), ptr(in_set), ptr(stats), stream()), "rr_top1_sets_f32")
    return dict(rank=rank[:total], before=before[:total], in_set=in_set[:total].bool(), stats=stats[:Q])


def conformal_threshold(scores, alpha: float) -> float:
    """Split-conformal threshold of the conformity scores E of n calibration queries (NaNs, the empty lists, dropped): the
    k-th smallest with k = ceil((n + 1) (1 - alpha)), or inf when k > n.  A fresh exchangeable query then has E <= tau with
    probability >= 1 - alpha (Vovk et al. 2005), and top1_sets' `covered` IS E <= tau."""
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must lie in (0, 1) (got {alpha!r})")
    e = scores.detach().cpu().numpy() if torch.is_tensor(scores) else np.asarray(scores)
    e = np.sort(np.asarray(e, np.float64).reshape(-1))
    e = e[~np.isnan(e)]
    n = int(e.size)
    k = int(np.ceil((n + 1) * (1.0 - alpha)))
    return float(e[k - 1]) if k <= n else float("inf")


def top1_calibration(stats, n_bins: int = 10) -> dict:
    """Is p_top1 = 0.8 right 80 % of the time?  From top1_sets' per-query `stats` [Q, 9] (rows of empty lists, NaN, dropped):
    accuracy (mean hit), confidence (mean p of the predicted top), brier (mean), and ece = sum_b (n_b / Q) |acc_b - conf_b|
    over `n_bins` equal-width confidence bins (bin = min(n_bins - 1, floor(confidence * n_bins))) with the per-bin arrays
    bin_count, bin_accuracy, bin_confidence (NaN for an empty bin).  Torch operations on Q numbers; no kernel."""
    nb_ = int(n_bins)
    if nb_ != n_bins or nb_ < 1:
        raise ValueError(f"n_bins must be a positive integer (got {n_bins!r})")
    s = torch.as_tensor(stats, dtype=torch.float64)
    s = s[~torch.isnan(s[:, 0])]
    Q = int(s.shape[0])
    if Q == 0:
        raise ValueError("no query with candidates")
    hit, conf = s[:, 0], s[:, 1]
    b = torch.clamp(torch.floor(conf * nb_), 0, nb_ - 1).long()
    zero = torch.zeros(nb_, dtype=torch.float64, device=s.device)
    count = zero.index_add(0, b, torch.ones_like(conf))
    acc = zero.index_add(0, b, hit) / count
    cnf = zero.index_add(0, b, conf) / count
    gap = torch.where(count > 0, (acc - cnf).abs(), zero)
    return dict(n=Q, accuracy=float(hit.sum()) / Q, confidence=float(conf.sum()) / Q, brier=float(s[:, 4].sum()) / Q,
                ece=float((count / Q * gap).sum()), bin_count=count.long().cpu().numpy(), bin_accuracy=acc.cpu().numpy(),
                bin_confidence=cnf.cpu().numpy())


def evaluate_calibration(model, calib_batches: Sequence[dict], test_batches: Sequence[dict], path_checkpoints, gpu: int,
                         method: str = "MC_dropout", alpha: float = 0.1, n_bins: int = 20, **kw) -> dict:
    """Calibrate on one set of queries, report on another.  evaluate_uncertainty(model, batches, path_checkpoints, gpu,
    method=method, **kw) runs on `calib_batches` and on `test_batches`; on the calibration set this fits
    sigma_scale = fit_sigma_scale(mean, targets, std) and tau = conformal_threshold(E, alpha), E being the probability mass
    ranked strictly ahead of each query's true top (top1_sets); on the test set it reports

      probabilistic   dict(before=probabilistic_calibration at scale 1, after=... at sigma_scale), `n_bins` PIT bins
      top1            top1_calibration of the test queries
      tau, coverage (share of the test queries whose true top is in its set), mean_set_size, and per candidate in_set, rank
      stats [Q, 9], p_top1, targets, scope, mean, std of the test set

    and calibration_set = dict(probabilistic=dict(before, after), coverage, mean_set_size, p_top1, targets, scope) of the
    calibration set itself (its coverage is at least 1 - alpha by construction).
    The sigma scale changes the POINTWISE numbers only: p_top1 is left as the method produced it (it is not recomputed under
    the scaled sigma), and the conformal threshold is what calibrates the ranking side - with exchangeable calibration and
    test queries the coverage is at least 1 - alpha in expectation whatever p_top1 is."""
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must lie in (0, 1) (got {alpha!r})")
    cal = evaluate_uncertainty(model, calib_batches, path_checkpoints, gpu, method=method, **kw)
    test = evaluate_uncertainty(model, test_batches, path_checkpoints, gpu, method=method, **kw)
    scale = fit_sigma_scale(cal["mean"], cal["targets"], cal["std"])
    tau = conformal_threshold(top1_sets(cal["p_top1"], cal["scope"], cal["targets"], 0.0, gpu)["stats"][:, 5], alpha)

    def report(r):
        sets = top1_sets(r["p_top1"], r["scope"], r["targets"], tau, gpu)
        st = sets["stats"]
        live = st[~torch.isnan(st[:, 0])]
        prob = {k: probabilistic_calibration(r["mean"], r["targets"], r["std"], n_bins, s)
                for k, s in (("before", 1.0), ("after", scale))}
        n = max(int(live.shape[0]), 1)                       # (integer sums divided on the host: correctly rounded quotients)
        return sets, dict(probabilistic=prob, coverage=float(live[:, 7].sum()) / n, mean_set_size=float(live[:, 6].sum()) / n)

    on_cal = dict(report(cal)[1], p_top1=cal["p_top1"], targets=cal["targets"], scope=cal["scope"])
    sets, on_test = report(test)
    return dict(method=method, alpha=alpha, sigma_scale=scale, tau=tau, **on_test, top1=top1_calibration(sets["stats"]),
                in_set=sets["in_set"], rank=sets["rank"], stats=sets["stats"], p_top1=test["p_top1"], targets=test["targets"],
                scope=test["scope"], mean=test["mean"], std=test["std"], calibration_set=on_cal)
