"""Bootstrap intervals and paired significance tests for the per-query ranking statistics.

`eval.ranking_stats` and `eval.rank_correlation_stats` leave one row of statistics per query on the device; every consumer so
far collapsed them to one mean per column.  This module keeps the spread: it resamples the QUERIES (the unit that is
independent in a ranking evaluation), thousands of times, in one launch of rr_resample_means_f64 - a counter-based draw
stream that numpy restates (tests/resample_ref.py) and ordered float64 sums that give the same bits on every run.

  resample_means     the kernel: B resampled column means of a [Q, M] float64 device table, bootstrap or sign flip
  bootstrap_ci       estimate, standard error and a percentile or BCa interval per column (or per output of `statistic`)
  paired_test        two models on the same queries: the difference, its bootstrap interval, wins / ties / losses and the
                     two-sided sign-flip randomisation p-value
  query_table        one eval-mode pass of a model -> the [Q, 12] table of the metric and rank-agreement columns
  metric_intervals   query_table + bootstrap_ci, with the pooled Kendall tau-b as a ratio statistic
  compare_models     query_table of two models + paired_test

Single process only: a resample draws from ALL queries, so under data-parallel evaluation the caller gathers the per-query
rows of every rank first (dp.py does not do that).  What an interval means: the queries are treated as a sample of the
population of queries the model will meet; with a few dozen queries the bootstrap distribution is coarse and its intervals
run narrow (the percentile interval of a mean under-covers roughly like a normal interval with n instead of n - 1), and no
amount of resamples mends that - B only removes the Monte-Carlo noise of the limits themselves.  No correction for looking at
many columns at once is applied.
"""
from __future__ import annotations

from typing import Callable, Iterable, Optional, Sequence

import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .eval import rank_correlation_stats, ranking_stats
from .uncertainty import sample_seed

MAX_COLS = _lib.RR_RESAMPLE_MAX_COLS
MAX_ROWS = _lib.RR_RESAMPLE_MAX_ROWS
MODES = {"bootstrap": _lib.RR_RESAMPLE_BOOTSTRAP, "signflip": _lib.RR_RESAMPLE_SIGNFLIP}
METRIC_NAMES = ("top1", "top1_in_target_top25", "recall25", "ndcg1", "ndcg2", "ndcg25", "ndcg_all", "ndcg_at_10")
AGREEMENT_NAMES = ("kendall_tau", "spearman", "mrr", "regret")
TABLE_NAMES = METRIC_NAMES + AGREEMENT_NAMES
_M64 = (1 << 64) - 1
_BOOT_STREAM, _FLIP_STREAM = 0, 1                 # sample_seed(seed, t): the two resampling streams of one user seed


def _as_table(x: torch.Tensor, what: str) -> torch.Tensor:
    _lib.require_cuda(x, what)
    if x.dtype != torch.float64:
        raise ValueError(f"{what}: a float64 table is expected (got {x.dtype}); the per-query statistics are float64")
    if x.dim() == 1:
        x = x[:, None]
    if x.dim() != 2:
        raise ValueError(f"{what}: expected [Q, M] or [Q] (got {tuple(x.shape)})")
    return x.detach()


def resample_means(x: torch.Tensor, n_resamples: int, seed: int = 0, mode: str = "bootstrap", first: int = 0):
    """B = n_resamples resampled column means of the float64 device table x [Q, M] (or [Q]) -> (means [B, M] float64, counts
    [B, M] int32: the non-NaN entries behind each mean; a mean with count 0 is NaN).  mode 'bootstrap': resample b draws Q rows
    with replacement; 'signflip': it keeps every row and flips its sign with probability 1/2.  Output row k is resample
    first + k of the stream `seed`, so a call may be cut into pieces.  include/reactranker_hip.h states the arithmetic
    (rr_resample_means_f64); the bits depend on the values, Q, seed and the resample's number only.  Rows are read in place by
    their stride; a table whose columns are not adjacent in memory is made contiguous first.  One launch, no synchronisation."""
    x = _as_table(x, "resample_means: `x`")
    if mode not in MODES:
        raise ValueError(f"resample_means: mode must be one of {sorted(MODES)} (got {mode!r})")
    B, first = int(n_resamples), int(first)
    Q, M = int(x.shape[0]), int(x.shape[1])
    if B < 0 or first < 0:
        raise ValueError(f"resample_means: n_resamples and first must be >= 0 (got {n_resamples!r}, {first!r})")
    if M < 1 or M > MAX_COLS:
        raise ValueError(f"resample_means: 1 to {MAX_COLS} columns (got {M})")
    if Q > MAX_ROWS:
        raise ValueError(f"resample_means: at most 2^20 rows (got {Q}): above that (draw * Q) >> 32 is too far from uniform")
    if (M > 1 and x.stride(1) != 1) or (Q > 1 and x.stride(0) < M):
        x = x.contiguous()
    means = torch.empty(B, M, dtype=torch.float64, device=x.device)
    counts = torch.empty(B, M, dtype=torch.int32, device=x.device)
    if B == 0:
        return means, counts
    with torch.cuda.device(x.device):
        check(lib().rr_resample_means_f64(ptr(x) if Q > 0 else None, x.stride(0) if Q > 1 else M, Q, M, MODES[mode],
                                          int(seed) & _M64, first, B, ptr(means), ptr(counts), stream()),
              "rr_resample_means_f64")
    return means, counts


# ---------------------------------------------------------------------------------------------- intervals
def _nan_stats(x: torch.Tensor):
    """per column of a table: (sum over the entries that are not NaN, their count as float64, the mask)"""
    ok = ~torch.isnan(x)
    return torch.where(ok, x, torch.zeros_like(x)).sum(dim=0), ok.sum(dim=0).to(torch.float64), ok


def _nanmean(x: torch.Tensor) -> torch.Tensor:
    s, n, _ = _nan_stats(x)
    return torch.where(n > 0, s / n.clamp(min=1.0), torch.full_like(s, float("nan")))


def _acceleration(x: torch.Tensor, statistic) -> torch.Tensor:
    """BCa's acceleration from the jackknife in closed form: leaving query i out moves a column mean to (S - x_i) / (n - 1) -
    a NaN entry leaves its column where it is.  Without `statistic` a column's own entries count; with it, every row."""
    s, n, ok = _nan_stats(x)
    full = s / n
    loo = torch.where(ok, (s - torch.where(ok, x, torch.zeros_like(x))) / (n - 1.0), full.expand_as(x))
    if statistic is None:
        bar = torch.where(ok, loo, torch.zeros_like(loo)).sum(dim=0) / n
        u = torch.where(ok, bar - loo, torch.zeros_like(loo))
        rows = n
    else:
        theta = statistic(loo)
        bar = theta.mean(dim=0)
        u = bar - theta
        rows = float(theta.shape[0])
    a = (u ** 3).sum(dim=0) / (6.0 * (u ** 2).sum(dim=0) ** 1.5)              # 0 / 0 = NaN for a constant column: the fallback
    # a column that is constant up to the rounding of its own sum (n additions) has no acceleration either
    return torch.where(u.abs().amax(dim=0) <= rows * 2.0 ** -53 * bar.abs(), torch.full_like(a, float("nan")), a)


def _intervals(m: torch.Tensor, est: torch.Tensor, level: float, method: str, accel: Optional[torch.Tensor]) -> dict:
    """m [B, K] resample values, est [K] -> {se, lo, hi, n_nan_resamples: [K] float64 tensors}.  Works on any device."""
    if method not in ("percentile", "bca"):
        raise ValueError(f"method must be 'percentile' or 'bca' (got {method!r})")
    if not 0.0 < level < 1.0:
        raise ValueError(f"level must lie inside (0, 1) (got {level!r})")
    K = m.shape[1]
    alpha = torch.tensor([(1.0 - level) / 2.0, 1.0 - (1.0 - level) / 2.0], dtype=torch.float64, device=m.device)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=m.device)
    se, lo, hi, bad = [], [], [], []
    for c in range(K):
        col = m[:, c]
        fin = col[torch.isfinite(col)]
        nb = fin.numel()
        bad.append(float(m.shape[0] - nb))
        if nb == 0:
            for v in (se, lo, hi):
                v.append(nan)
            continue
        q = alpha
        if method == "bca":
            below = (fin < est[c]).sum().to(torch.float64) + 0.5 * (fin == est[c]).sum().to(torch.float64)
            z0 = torch.special.ndtri(below / nb)
            z = z0 + torch.special.ndtri(alpha)
            adj = torch.special.ndtr(z0 + z / (1.0 - accel[c] * z))
            q = torch.where(torch.isfinite(z0) & torch.isfinite(accel[c]) & torch.isfinite(adj), adj, alpha)
        lohi = torch.quantile(fin, q, interpolation="linear")
        lo.append(lohi[0])
        hi.append(lohi[1])
        se.append(fin.std(unbiased=True) if nb > 1 else nan)
    return dict(se=torch.stack(se), lo=torch.stack(lo), hi=torch.stack(hi),
                n_nan_resamples=torch.tensor(bad, dtype=torch.float64, device=m.device))


def _names(names, K: int, what: str):
    if names is None:
        return [f"col{c}" for c in range(K)]
    names = list(names)
    if len(names) != K or len(set(names)) != K:
        raise ValueError(f"{what}: `names` must hold {K} distinct names (got {names})")
    return names


def _rows_to_dicts(names, fields: dict, ints=()) -> dict:
    """{name: {field: Python number}} from {field: [K] tensor}: the one copy to the host"""
    keys = list(fields)
    host = torch.stack([fields[k].to(torch.float64) for k in keys]).cpu().tolist()
    return {name: {k: (int(host[i][c]) if k in ints else float(host[i][c])) for i, k in enumerate(keys)}
            for c, name in enumerate(names)}


def bootstrap_ci(x: torch.Tensor, n_resamples: int = 2000, level: float = 0.95, method: str = "percentile", seed: int = 0,
                 statistic: Optional[Callable] = None, names: Optional[Sequence[str]] = None) -> dict:
    """Bootstrap over the rows (queries) of the float64 device table x [Q, M]: {name: {estimate, se, lo, hi, n,
    n_nan_resamples}} per column (names default to col0, col1, ...).
      estimate         the column's mean over its entries that are not NaN
      se               standard deviation (ddof 1) of the finite resample means
      lo, hi           percentile: torch.quantile (linear) of the finite resample means at (1 - level) / 2 and 1 - (1 - level) / 2;
                       'bca': the same quantiles at the bias-corrected and accelerated levels
                       Phi(z0 + (z0 + z_alpha) / (1 - a (z0 + z_alpha))), z0 = ndtri((#{m_b < est} + #{m_b == est} / 2) / B),
                       a from the closed-form jackknife; the percentile levels where z0 or a is not finite (a constant column)
      n                entries that are not NaN;  n_nan_resamples: resamples whose mean was not finite (they drew only NaN rows)
    statistic: a callable on [B, M] means returning [B, K], for ratio statistics such as the pooled tau-b; it is applied to the
    row of estimates as well, `names` then name its K outputs and n is the number of rows.  The resamples are stream
    sample_seed(seed, 0).  Synchronises the host (the result is Python numbers)."""
    x = _as_table(x, "bootstrap_ci: `x`")
    means, _ = resample_means(x, n_resamples, seed=sample_seed(seed, _BOOT_STREAM), mode="bootstrap")
    s, n, _ = _nan_stats(x)
    est = _nanmean(x)
    if statistic is not None:
        means, est = statistic(means), statistic(est[None, :])[0]
        n = torch.full_like(est, float(x.shape[0]))
    accel = _acceleration(x, statistic) if method == "bca" else None
    out = _intervals(means, est, level, method, accel)
    fields = dict(estimate=est, se=out["se"], lo=out["lo"], hi=out["hi"], n=n, n_nan_resamples=out["n_nan_resamples"])
    return _rows_to_dicts(_names(names, est.numel(), "bootstrap_ci"), fields, ints=("n", "n_nan_resamples"))


def paired_test(a: torch.Tensor, b: torch.Tensor, n_resamples: int = 10000, level: float = 0.95, seed: int = 0,
                names: Optional[Sequence[str]] = None, method: str = "percentile") -> dict:
    """Two models scored on the same queries in the same order: a, b [Q, M] float64 device tables -> {name: {mean_a, mean_b,
    diff, se, lo, hi, wins, ties, losses, n, p_value}} per column.  d = a - b is NaN where either entry is; mean_a, mean_b and
    diff are means over the n rows where d is defined; (lo, hi) is the bootstrap interval of diff (bootstrap_ci on d, stream
    sample_seed(seed, 0)); wins / ties / losses count d > 0, == 0, < 0.
    p_value: the two-sided sign-flip randomisation p.  Under the null hypothesis that the two models are exchangeable on every
    query the signs of d are fair coins, so T_b = mean(sign_b * d) over B = n_resamples sign vectors (stream sample_seed(seed, 1))
    is a sample of the null distribution of T_obs = mean(d):  p = (1 + #{b : |T_b| >= |T_obs| - tol}) / (B + 1), with
    tol = n 2^-52 mean|d| so that a T_b equal to T_obs up to the rounding of its sum counts (the slack only ever makes p
    larger; on integer-valued d every sum is exact).  NaN where no row is defined.  Synchronises the host."""
    a, b = _as_table(a, "paired_test: `a`"), _as_table(b, "paired_test: `b`")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"paired_test: the two tables must have one shape on one device (got {tuple(a.shape)}, {tuple(b.shape)})")
    d = a - b
    s, n, ok = _nan_stats(d)
    zero = torch.zeros_like(d)
    nn = n.clamp(min=1.0)
    nan = torch.full_like(s, float("nan"))
    diff = torch.where(n > 0, s / nn, nan)
    mean_a = torch.where(n > 0, torch.where(ok, a, zero).sum(dim=0) / nn, nan)
    mean_b = torch.where(n > 0, torch.where(ok, b, zero).sum(dim=0) / nn, nan)
    boot, _ = resample_means(d, n_resamples, seed=sample_seed(seed, _BOOT_STREAM), mode="bootstrap")
    accel = _acceleration(d, None) if method == "bca" else None
    ci = _intervals(boot, diff, level, method, accel)
    flips, _ = resample_means(d, n_resamples, seed=sample_seed(seed, _FLIP_STREAM), mode="signflip")
    tol = n * 2.0 ** -52 * (torch.where(ok, d.abs(), zero).sum(dim=0) / nn)
    hits = (flips.abs() >= diff.abs() - tol).sum(dim=0).to(torch.float64)
    p = torch.where(n > 0, (1.0 + hits) / torch.full_like(hits, float(flips.shape[0]) + 1.0), nan)     # (tensor / tensor: a true division)
    fields = dict(mean_a=mean_a, mean_b=mean_b, diff=diff, se=ci["se"], lo=ci["lo"], hi=ci["hi"],
                  wins=(d > 0).sum(dim=0), ties=(d == 0).sum(dim=0), losses=(d < 0).sum(dim=0), n=n, p_value=p)
    return _rows_to_dicts(_names(names, d.shape[1], "paired_test"), fields, ints=("wins", "ties", "losses", "n"))


# ---------------------------------------------------------------------------------------------- models
def _query_tables(model, gpu, batches: Iterable) -> torch.Tensor:
    """[Q, 16] float64: the 8 metric columns of ranking_stats, then the 8 columns of rank_correlation_stats"""
    was_training = model.training
    model.eval()
    rows = []
    try:
        with torch.no_grad():
            for r_batch, p_batch, scope, targets, add_features in batches:
                if len(scope) == 0:
                    continue
                out = model(r_batch, p_batch, gpu=gpu, add_features=add_features)
                rows.append(torch.cat([ranking_stats(out, scope, targets, gpu)[0][:, :len(METRIC_NAMES)],
                                       rank_correlation_stats(out, scope, targets, gpu)], dim=1))
    finally:
        model.train(was_training)
    if rows:
        return torch.cat(rows, 0)
    dev = torch.device("cuda", torch.cuda.current_device() if gpu is None else gpu)
    return torch.zeros(0, len(METRIC_NAMES) + 8, dtype=torch.float64, device=dev)


def query_table(model, gpu, batches: Iterable):
    """One eval-mode pass of `model` over (r_batch, p_batch, scope, targets, add_features) batches of whole queries -> (table
    [Q, 12] float64 on the device, names): per query top1, predicted top-1 in the target's top 25 %, recall@25 %, NDCG1, NDCG2,
    NDCG25 %, NDCG_all, NDCG@10, then Kendall tau-b, Spearman rho, the reciprocal rank and the regret (NaN where a coefficient
    is undefined).  The caller's train / eval mode is restored, as ranking_metrics does."""
    return _query_tables(model, gpu, batches)[:, :len(TABLE_NAMES)], list(TABLE_NAMES)


def _pooled_tau(m: torch.Tensor) -> torch.Tensor:
    """[B, 4] means of the pair counts P, D, X, Y -> [B, 1] tau-b of the pooled counts (a ratio: the common 1 / Q cancels)"""
    P, D, X, Y = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    den = (P + D + X) * (P + D + Y)
    return torch.where(den > 0, (P - D) / den.clamp(min=0.0).sqrt(), torch.full_like(den, float("nan")))[:, None]


def metric_intervals(model, gpu, batches: Iterable, n_resamples: int = 2000, level: float = 0.95, method: str = "percentile",
                     seed: int = 0) -> dict:
    """query_table + bootstrap_ci: {name: {estimate, se, lo, hi, n, n_nan_resamples}} for the twelve columns of query_table and
    for `kendall_tau_pooled`, the tau-b of the pair counts summed over the queries, whose interval comes from the resampled
    counts through `statistic=` (the same resamples of the queries: one seed, one stream)."""
    full = _query_tables(model, gpu, batches)
    out = bootstrap_ci(full[:, :len(TABLE_NAMES)], n_resamples, level, method, seed, names=TABLE_NAMES)
    out.update(bootstrap_ci(full[:, len(TABLE_NAMES):], n_resamples, level, method, seed, statistic=_pooled_tau,
                            names=["kendall_tau_pooled"]))
    return out


def compare_models(model_a, model_b, gpu, batches, n_resamples: int = 10000, level: float = 0.95, seed: int = 0,
                   method: str = "percentile") -> dict:
    """query_table of two models over the same batches (a list: it is walked twice) + paired_test: per column of query_table
    {mean_a, mean_b, diff, se, lo, hi, wins, ties, losses, n, p_value}."""
    batches = list(batches)
    ta, names = query_table(model_a, gpu, batches)
    tb, _ = query_table(model_b, gpu, batches)
    return paired_test(ta, tb, n_resamples, level, seed, names=names, method=method)
