"""reactranker_amd.uncertainty without a GPU: the C-ABI exports, the sample seeds, the argument checks that come before any
launch, and the numpy restatements the GPU tests (tests/test_gpu_uncertainty.py) hold the kernels to - the Spearman one
pinned to scipy.stats.spearmanr here."""
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from reactranker_amd import uncertainty as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rr_mc_sample_stats_f32", "rr_uq_calibration_f64")


# ---------------------------------------------------------------------------------------------- numpy restatements
def stable_desc_order(x):
    """Stable descending order: larger first, ties by position."""
    x = np.asarray(x, np.float64)
    return np.lexsort((np.arange(len(x)), -x))


def rankdata_avg(x):
    """1-based ranks with ties averaged (scipy.stats.rankdata's 'average')."""
    x = np.asarray(x, np.float64)
    n = len(x)
    order = np.argsort(x, kind="stable")
    xs = x[order]
    starts = np.r_[0, np.flatnonzero(xs[1:] != xs[:-1]) + 1] if n else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], n]
    r = np.empty(n)
    r[order] = np.repeat((starts + ends + 1) / 2.0, ends - starts)
    return r


def spearman_ref(a, b):
    ra, rb = rankdata_avg(a), rankdata_avg(b)
    da, db = ra - ra.mean(), rb - rb.mean()
    sxx, syy = float((da * da).sum()), float((db * db).sum())
    if sxx == 0.0 or syy == 0.0:
        return math.nan
    return float(np.clip((da * db).sum() / math.sqrt(sxx * syy), -1.0, 1.0))


def curve_ref(err, unc, fractions):
    """(kept, mae, rmse) per fraction: the floor(f * n) most uncertain rows (stable descending order) removed."""
    n = len(err)
    e = np.abs(np.asarray(err, np.float64))
    desc = stable_desc_order(unc)
    kept, mae, rmse = [], [], []
    for f in fractions:
        k = min(math.floor(f * n), n - 1)
        rest = e[desc[k:]]
        kept.append(n - k)
        mae.append(rest.sum() / (n - k))
        rmse.append(math.sqrt((rest * rest).sum() / (n - k)))
    return np.array(kept), np.array(mae), np.array(rmse)


def stats_ref(samples, scope, targets):
    """What rr_mc_sample_stats_f32 computes, from a [T, M] float32 array."""
    x = np.asarray(samples, np.float32)
    T, M = x.shape
    acc = np.zeros(M)
    for t in range(T):                                  # f64, in sample order
        acc += x[t].astype(np.float64)
    m = acc / T
    ss = np.zeros(M)
    for t in range(T):
        d = x[t].astype(np.float64) - m
        ss += d * d
    mean, std = m.astype(np.float32), np.sqrt(ss / (T - 1)).astype(np.float32)
    top1, rsum = np.zeros(M, np.int64), np.zeros(M, np.int64)
    tg = np.asarray(targets, np.float32).reshape(-1)
    qstats = np.zeros((len(scope), 4))
    off = 0
    for q, c in enumerate(scope):
        if c == 0:
            continue
        for t in range(T):
            order = stable_desc_order(x[t, off:off + c])
            rank = np.empty(c, np.int64)
            rank[order] = np.arange(c)
            rsum[off:off + c] += rank
            top1[off + order[0]] += 1
        p = top1[off:off + c] / T
        nz = p[p > 0]
        qstats[q] = [-(nz * np.log(nz)).sum(), p[int(np.argmax(tg[off:off + c]))],
                     p[int(np.argmax(mean[off:off + c]))], std[off:off + c].astype(np.float64).mean()]
        off += c
    return dict(mean=mean, std=std, p_top1=(top1 / T).astype(np.float32), mean_rank=((rsum + T) / T).astype(np.float32),
                qstats=qstats)


# ---------------------------------------------------------------------------------------------- tests
def test_new_symbols_are_declared_and_exported():
    missing = [s for s in NEW_SYMBOLS if s not in _lib.EXPORTED_SYMBOLS]
    assert not missing, missing
    hdr = open(os.path.join(REPO, "include", "reactranker_hip.h")).read()
    declared = set(re.findall(r"\b(rr_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW_SYMBOLS) <= declared
    assert "#define RR_UQ_NQSTATS 4" in hdr and U.NQSTATS == 4
    assert re.search(r"#define RR_UQ_CAL_BLOCK (\d+)", hdr).group(1) == str(U.CAL_BLOCK)


def test_library_loads_the_new_entries():
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert getattr(lib, s).argtypes is not None


def test_sample_seed_is_deterministic_and_62_bit():
    seeds = [U.sample_seed(s, t) for s in (0, 1, 7, 2 ** 63, -1) for t in range(64)]
    assert seeds == [U.sample_seed(s, t) for s in (0, 1, 7, 2 ** 63, -1) for t in range(64)]
    assert all(isinstance(v, int) and 0 <= v < 2 ** 62 for v in seeds)
    assert len(set(seeds)) == len(seeds)
    # the documented mix: splitmix64's finaliser, twice
    m = (1 << 64) - 1

    def mix(x):
        x &= m
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
        return x ^ (x >> 31)
    assert U.sample_seed(5, 3) == mix(mix(5) + 4 * 0x9E3779B97F4A7C15) >> 2
    with pytest.raises(ValueError):
        U.sample_seed(0, -1)


def test_too_few_samples_are_refused_before_any_launch():
    with pytest.raises(ValueError, match="n_samples"):
        U.mc_dropout_predict(object(), [], 1)                  # not even a model: nothing may be touched
    with pytest.raises(ValueError, match="n_samples"):
        U.evaluate_uncertainty(object(), [], "x.pt", 0, method="MC_dropout", n_samples=1)
    with pytest.raises(ValueError, match="2 checkpoints"):
        U.ensemble_predict(object(), ["a.pt"], [])
    with pytest.raises(ValueError, match="method"):
        U.evaluate_uncertainty(object(), [], "x.pt", 0, method="bootstrap")


@pytest.mark.parametrize("fractions", [(0.0, 1.0), (-0.1,), (0.5, float("nan"))])
def test_fractions_outside_the_unit_interval_are_refused(fractions):
    x = torch.zeros(5)                                          # CPU tensors: any launch attempt would fail differently
    with pytest.raises(ValueError, match="fractions"):
        U.uncertainty_calibration(x, x, x, fractions)


def test_lengths_that_differ_are_refused():
    a, b = torch.zeros(5), torch.zeros(4)
    for args in ((a, a, b), (a, b, a), (b, a, a)):
        with pytest.raises(ValueError, match="length"):
            U.uncertainty_calibration(*args)
    with pytest.raises(ValueError, match="at least one"):
        U.uncertainty_calibration(torch.zeros(0), torch.zeros(0), torch.zeros(0))


def test_ensemble_with_different_scalers_is_refused(tmp_path):
    paths = []
    for i, (m, s) in enumerate([(1.0, 2.0), (1.5, 2.0)]):
        p = str(tmp_path / f"{i}.pt")
        torch.save({"state_dict": {}, "data_scaler": {"means": m, "stds": s}}, p)
        paths.append(p)
    with pytest.raises(ValueError, match="scalers"):
        U.evaluate_uncertainty(object(), [], paths, 0, method="ensemble")


def test_spearman_restatement_matches_scipy_with_heavy_ties():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(3)
    for n in (2, 3, 17, 1000, 20000):
        a = np.round(rng.standard_normal(n) * 2).astype(np.float32)        # ~10 distinct values
        b = (np.round(a + rng.standard_normal(n)) * 0.5).astype(np.float32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                     # (scipy warns on a constant input, n = 2 may be one)
            want = stats.spearmanr(a, b).statistic
        got = spearman_ref(a, b)
        assert (math.isnan(want) and math.isnan(got)) or abs(got - want) <= 1e-12, (n, got, want)
        assert np.array_equal(rankdata_avg(a), stats.rankdata(a))
    assert math.isnan(spearman_ref(np.ones(10), np.arange(10.0)))


def test_curve_restatement_removes_the_most_uncertain_rows_first():
    err = np.array([1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    unc = np.array([0.5, 0.9, 0.9, 0.1, 0.2], np.float32)
    # stable descending order of unc: rows 1, 2 (tie, row order), 0, 4, 3
    assert list(stable_desc_order(unc)) == [1, 2, 0, 4, 3]
    kept, mae, rmse = curve_ref(err, unc, [0.0, 0.2, 0.4, 0.99])
    assert list(kept) == [5, 4, 3, 1]
    assert mae[1] == (1 + 3 + 4 + 5) / 4 and mae[2] == (1 + 4 + 5) / 3 and mae[3] == 4.0
    assert rmse[3] == 4.0


def test_stats_restatement_on_a_hand_example():
    s = np.array([[1, 3, 3, 0, 2], [2, 1, 2, 5, 5]], np.float32)      # lists [3, 2]
    r = stats_ref(s, [3, 2], np.array([0, 1, 2, 3, 3], np.float32))
    assert r["p_top1"].tolist() == [0.5, 0.5, 0.0, 0.5, 0.5]            # first maximum: rows 1 then 0; 4 then 3
    assert r["mean_rank"].tolist() == [2.0, 2.0, 2.0, 1.5, 1.5]
    assert r["qstats"][0, 1] == 0.0 and r["qstats"][1, 1] == 0.5      # the target's first maximum: row 2; row 3
