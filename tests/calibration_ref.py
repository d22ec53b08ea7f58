"""Numpy / scipy restatement in float64 of the calibration entries (include/reactranker_hip.h: rr_gauss_calibration_f64 and
rr_top1_sets_f32), with the input generators, shared by tests/test_calibration_cpu.py and
tests/test_gpu_calibration.py.

Written from the header's definitions, not from the kernels.  `before` is an ORDERED sum: np.cumsum (sequential, unlike the
pairwise np.sum) over the list with the candidates that are not ahead replaced by 0.0 - adding +0.0 changes no bit of a
non-negative partial sum - so it is bit-comparable with the library; so are the Brier score and the mass.  The pointwise sums
are summed in row order here and in block order there: they agree to the summation-order bound only, and each sum comes with
the sum of its terms' magnitudes for that bound."""
import numpy as np
from scipy.special import erfc

GAUSS_NSUMS = 8
TOP1_NSTATS = 9
BLOCK = 512
SUM_NAMES = ("n_valid", "n_invalid", "sum z", "sum z^2", "sum ln sigma", "sum sigma^2", "sum err^2", "sum crps")
INV_SQRT_2PI = 0.3989422804014327       # 1 / sqrt(2 pi)
INV_SQRT_PI = 0.5641895835477563        # 1 / sqrt pi
EDGE = 1e-9


# ------------------------------------------------------------------------------------------------ pointwise
def gauss_rows(seed, n, spread=1.3):
    """(mean, std, target) float32: mean ~ N(0, 1), std ~ U(0.05, 3), target = mean + spread * std * N(0, 1)"""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal(n)
    std = rng.uniform(0.05, 3.0, n)
    target = mean + spread * std * rng.standard_normal(n)
    return mean.astype(np.float32), std.astype(np.float32), target.astype(np.float32)


def inject_invalid(mean, std, target):
    """copies with up to four invalid rows spread over the array: a NaN mean, a zero, a negative and an infinite std"""
    mean, std, target = mean.copy(), std.copy(), target.copy()
    n = len(mean)
    rows = sorted({0, n // 3, (2 * n) // 3, n - 1})
    for k, r in enumerate(rows):
        if k == 0:
            mean[r] = np.nan
        else:
            std[r] = (0.0, -1.0, np.inf)[k - 1]
    return mean, std, target, len(rows)


def gauss_calibration(mean, std, target, sigma_scale=1.0, n_bins=20):
    """dict(sums [8], mags [8] = the sums of the terms' magnitudes, hist [n_bins] int64, edge = the number of valid rows whose
    pit * n_bins lies within 1e-9 of an interior integer, bins and edge_mask per valid row)."""
    m, s, t = (np.asarray(v, np.float32).reshape(-1).astype(np.float64) for v in (mean, std, target))
    valid = np.isfinite(m) & np.isfinite(t) & np.isfinite(s) & (s > 0)
    m, s, t = m[valid], s[valid], t[valid]
    sigma = np.float64(sigma_scale) * s
    err = t - m
    z = err / sigma
    pit = 0.5 * erfc(-z / np.sqrt(2.0))
    pdf = INV_SQRT_2PI * np.exp(-0.5 * (z * z))
    crps = sigma * (z * (2.0 * pit - 1.0) + 2.0 * pdf - INV_SQRT_PI)
    terms = [np.ones_like(z), None, z, z * z, np.log(sigma), sigma * sigma, err * err, crps]
    sums, mags = np.zeros(GAUSS_NSUMS), np.zeros(GAUSS_NSUMS)
    for k, v in enumerate(terms):
        if v is not None and len(v):
            sums[k], mags[k] = np.cumsum(v)[-1], np.cumsum(np.abs(v))[-1]
    sums[1] = mags[1] = float((~valid).sum())
    x = pit * n_bins
    bins = np.minimum(n_bins - 1, np.floor(x).astype(np.int64))
    near = np.rint(x)
    edge_mask = (np.abs(x - near) < EDGE) & (near >= 1) & (near <= n_bins - 1)
    return dict(sums=sums, mags=mags, hist=np.bincount(bins, minlength=n_bins).astype(np.int64), edge=int(edge_mask.sum()),
                bins=bins, edge_mask=edge_mask)


def probabilistic(ref):
    """The means reactranker_amd.uncertainty.probabilistic_calibration forms, from gauss_calibration's dict."""
    o, hist = ref["sums"], ref["hist"].astype(np.float64)
    n, nb = o[0], len(hist)
    expected = np.arange(1, nb + 1) / nb
    observed = np.cumsum(hist) / n
    return dict(nll=0.5 * np.log(2 * np.pi) + o[4] / n + 0.5 * o[3] / n, crps=o[7] / n, z_mean=o[2] / n, z2_mean=o[3] / n,
                sharpness=np.sqrt(o[5] / n), rmse=np.sqrt(o[6] / n), observed=observed, expected=expected,
                miscalibration_area=float(np.mean(np.abs(observed - expected))))


# ------------------------------------------------------------------------------------------------ top-1 sets
def list_targets(rng, scope, ties):
    """float32 targets of every list: N(0, 1), rounded to halves when `ties` (the first maximum then decides)"""
    t = rng.standard_normal(int(sum(scope))).astype(np.float32)
    return (np.round(t * 2) / 2).astype(np.float32) if ties else t


def sample_share_window(seed, scope, T=32, noise=1.0, ties=False):
    """(p, targets) float32.  p_i = the share of T synthetic score samples in which candidate i is its list's first maximum:
    multiples of 1 / T, with many ties and zeros, and every partial sum exactly representable.  Scores and targets are the
    same latent utility plus independent N(0, noise^2), so p is informative and imperfect."""
    rng = np.random.default_rng(seed)
    ps, ts = [], []
    for c in scope:
        u = rng.standard_normal(c)
        s = u[None, :] + noise * rng.standard_normal((T, c))
        p = np.bincount(np.argmax(s, axis=1), minlength=c) / T if c else np.zeros(0)
        t = u + noise * rng.standard_normal(c)
        ps.append(p.astype(np.float32))
        ts.append((np.round(t * 2) / 2 if ties else t).astype(np.float32))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.float32)
    return cat(ps), cat(ts)


def softmax_window(seed, scope, scale=4.0, ties=False):
    """(p, targets) float32.  p = the float64 softmax of scale * N(0, 1) per list, rounded to float32: continuous, no ties to
    speak of, values down to 1e-15 in a long list."""
    rng = np.random.default_rng(seed)
    ps = []
    for c in scope:
        x = scale * rng.standard_normal(c)
        e = np.exp(x - x.max()) if c else x
        ps.append((e / e.sum() if c else e).astype(np.float32))
    p = np.concatenate(ps) if ps else np.zeros(0, np.float32)
    return p, list_targets(rng, scope, ties)


def list_core(p, t):
    """What does not depend on tau, for one list of C >= 1: rank [C] int32, before [C] float64, the true top, the predicted
    top, the Brier score and the mass."""
    p, t = np.asarray(p, np.float32).reshape(-1), np.asarray(t, np.float32).reshape(-1)
    C = len(p)
    p64, pos = p.astype(np.float64), np.arange(C)
    rank, before = np.zeros(C, np.int32), np.zeros(C, np.float64)
    for lo in range(0, C, BLOCK):
        hi = min(C, lo + BLOCK)
        pi = p[lo:hi, None]
        ahead = (p[None, :] > pi) | ((p[None, :] == pi) & (pos[None, :] < pos[lo:hi, None]))
        rank[lo:hi] = 1 + ahead.sum(1)
        before[lo:hi] = np.cumsum(np.where(ahead, p64[None, :], 0.0), axis=1)[:, -1]     # ascending j, one chain per row
    it = int(np.argmax(t))                                                             # the first maximum
    is_ = int(np.flatnonzero(rank == 1)[0])
    d = p64 - (pos == it)
    return rank, before, it, is_, np.cumsum(d * d)[-1], np.cumsum(p64)[-1]


def window_core(p, scope, t):
    """list_core of every list of the window (None for an empty list); independent of tau, so computed once per window"""
    cores, off = [], 0
    for c in scope:
        cores.append(list_core(p[off:off + c], t[off:off + c]) if c else None)
        off += c
    return cores


def window_sets(p, scope, t, tau, cores=None):
    """(rank [M] int32, before [M] float64, in_set [M] bool, stats [Q, 9] float64) of rr_top1_sets_f32"""
    p = np.asarray(p, np.float32).reshape(-1)
    cores = window_core(p, scope, t) if cores is None else cores
    M = int(sum(scope))
    rank, before = np.zeros(M, np.int32), np.zeros(M, np.float64)
    stats = np.zeros((len(scope), TOP1_NSTATS), np.float64)
    off = 0
    for q, (c, core) in enumerate(zip(scope, cores)):
        if c == 0:
            stats[q, :6] = np.nan
            continue
        r, b, it, is_, brier, mass = core
        rank[off:off + c], before[off:off + c] = r, b
        inside = b <= tau
        stats[q] = (float(is_ == it), np.float64(p[off + is_]), np.float64(p[off + it]), r[it], brier, b[it], inside.sum(),
                    float(inside[it]), mass)
        off += c
    return rank, before, before <= tau, stats


def conformal_threshold(scores, alpha):
    """the ceil((n + 1)(1 - alpha))-th smallest of the n scores that are not NaN; inf when there is no such score"""
    e = np.sort(np.asarray(scores, np.float64).reshape(-1))
    e = e[~np.isnan(e)]
    k = int(np.ceil((len(e) + 1) * (1.0 - alpha)))
    return float(e[k - 1]) if k <= len(e) else float("inf")


def ece(stats, n_bins=10):
    """expected calibration error of the per-query (hit, confidence) over equal-width confidence bins"""
    s = np.asarray(stats, np.float64).reshape(-1, TOP1_NSTATS)
    s = s[~np.isnan(s[:, 0])]
    b = np.minimum(n_bins - 1, np.floor(s[:, 1] * n_bins).astype(np.int64))
    total = 0.0
    for k in range(n_bins):
        sel = b == k
        if sel.any():
            total += sel.sum() / len(s) * abs(s[sel, 0].mean() - s[sel, 1].mean())
    return total
