"""Float64 restatement of rr_analytic_rank_stats_f32 (include/reactranker_hip.h): the statistics of a list of independent
Gaussian scores from their means and variances.  There is no reference code for this, so the header's definition is
restated here with torch.special.erfc on float64 CPU tensors; tests/test_analytic_uq_cpu.py pins it to closed forms and to
sampling, tests/test_gpu_analytic_uq.py holds the kernel to it.

`pair_dtype=torch.float32` gives the same formulas with the kernel's arithmetic split - margin and erfc in float32, the
product over rivals, the node sum and the rank sum in float64 - which measures what float32 margins alone cost."""
import math

import numpy as np
import torch

from reactranker_amd.uncertainty import MOMENT_COLUMNS, quadrature

SQRT_HALF_F32 = np.float32(0.70710678)


def moments_ref(output, kind):
    """(mu, var, aleatoric, epistemic) in float64 from the float32 rows of a head's output; the last two are None unless
    kind is 'nig'."""
    o = np.asarray(output, np.float32).astype(np.float64)
    assert o.ndim == 2 and o.shape[1] >= MOMENT_COLUMNS[kind]
    mu = o[:, 0].copy()
    if kind == "gaussian":
        return mu, o[:, 1].copy(), None, None
    if kind == "log_variance":
        return mu, np.exp(o[:, 1]), None, None
    assert kind == "nig"
    v, alpha, beta = o[:, 1], o[:, 2], o[:, 3]
    ale = beta / (alpha - 1.0)
    epi = beta / (v * (alpha - 1.0))
    return mu, ale + epi, ale, epi


def _phi(z):
    return 0.5 * torch.special.erfc(-z / math.sqrt(2.0))


def list_ref(mu, var, n_nodes=32, rows=None, pair_dtype=torch.float64):
    """(p_top1, mean_rank) in float64 of the candidates `rows` (default: all) of ONE list with means mu and variances var."""
    mu_t, var_t = torch.as_tensor(np.asarray(mu, np.float64)), torch.as_tensor(np.asarray(var, np.float64))
    C = int(mu_t.numel())
    rows_t = torch.arange(C) if rows is None else torch.as_tensor(np.asarray(rows, np.int64))
    R = int(rows_t.numel())
    x, w = quadrature(n_nodes)
    sd = torch.sqrt(var_t)
    not_self = torch.ones(R, C, dtype=torch.bool)
    not_self[torch.arange(R), rows_t] = False
    p = torch.zeros(R, dtype=torch.float64)
    if pair_dtype == torch.float64:
        d = (mu_t[None, :] - mu_t[rows_t, None]) / torch.sqrt(var_t[rows_t, None] + var_t[None, :])
        rank = 1.0 + torch.where(not_self, _phi(d), torch.zeros(())).sum(dim=1)
        for xn, wn in zip(x, w):
            t = mu_t[rows_t] + sd[rows_t] * float(xn)
            f = _phi((t[:, None] - mu_t[None, :]) / sd[None, :])
            p += float(wn) * torch.where(not_self, f, torch.ones((), dtype=torch.float64)).prod(dim=1)
        return p.numpy(), rank.numpy()
    assert pair_dtype == torch.float32
    k = torch.tensor(SQRT_HALF_F32)
    mu_f, var_f, sd_f, inv_f = mu_t.float(), var_t.float(), sd.float(), (1.0 / sd).float()
    d = (mu_f[rows_t, None] - mu_f[None, :]) / torch.sqrt(var_f[rows_t, None] + var_f[None, :])
    f = 0.5 * torch.special.erfc(d * k)
    rank = 1.0 + torch.where(not_self, f.double(), torch.zeros((), dtype=torch.float64)).sum(dim=1)
    for xn, wn in zip(x, w):
        t = mu_f[rows_t] + sd_f[rows_t] * torch.tensor(np.float32(xn))
        f = 0.5 * torch.special.erfc((mu_f[None, :] - t[:, None]) * inv_f[None, :] * k)
        p += float(wn) * torch.where(not_self, f.double(), torch.ones((), dtype=torch.float64)).prod(dim=1)
    return p.numpy(), rank.numpy()


def qstats_ref(mean, std, p_top1, scope, targets):
    """(qstats [Q, 4], mass [Q]) in float64 from the float32 per-candidate arrays, in list order."""
    mean, std, p = (np.asarray(a, np.float32) for a in (mean, std, p_top1))
    tg = np.asarray(targets, np.float32).reshape(-1)
    qstats, mass = np.zeros((len(scope), 4)), np.zeros(len(scope))
    off = 0
    for q, c in enumerate(scope):
        if c == 0:
            continue
        pq = p[off:off + c].astype(np.float64)
        nz = pq[pq > 0]
        qstats[q] = [-(nz * np.log(nz)).sum(), pq[int(np.argmax(tg[off:off + c]))], pq[int(np.argmax(mean[off:off + c]))],
                     std[off:off + c].astype(np.float64).mean()]
        mass[q] = pq.sum()
        off += c
    return qstats, mass


def analytic_ref(output, scope, targets, kind, n_nodes=32):
    """What rr_analytic_rank_stats_f32 defines, every number in float64 except `mean` (the float32 column 0); qstats and
    mass are formed from the float32 roundings of mean, std and p_top1, as the kernel forms them from its own outputs."""
    out = np.asarray(output, np.float32)
    mu, var, ale, epi = moments_ref(out, kind)
    M = len(mu)
    p, rank = np.zeros(M), np.zeros(M)
    off = 0
    for c in scope:
        if c:
            p[off:off + c], rank[off:off + c] = list_ref(mu[off:off + c], var[off:off + c], n_nodes)
        off += c
    std = np.sqrt(var)
    res = dict(mean=out[:, 0].copy(), std=std, p_top1=p, mean_rank=rank)
    if kind == "nig":
        res.update(aleatoric_std=np.sqrt(ale), epistemic_std=np.sqrt(epi))
    res["qstats"], res["mass"] = qstats_ref(res["mean"], std.astype(np.float32), p.astype(np.float32), scope, targets)
    return res


def sampled_p_top1(mu, var, n_samples, seed, chunk=20000):
    """Share of `n_samples` seeded numpy draws of the list in which each candidate is the first maximum."""
    rng = np.random.default_rng(seed)
    mu, sd = np.asarray(mu, np.float64), np.sqrt(np.asarray(var, np.float64))
    wins = np.zeros(len(mu), np.int64)
    done = 0
    while done < n_samples:
        n = min(chunk, n_samples - done)
        s = mu[None, :] + sd[None, :] * rng.standard_normal((n, len(mu)))
        wins += np.bincount(np.argmax(s, axis=1), minlength=len(mu))
        done += n
    return wins / n_samples
