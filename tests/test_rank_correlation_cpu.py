"""CPU-side checks of the per-query rank correlation: the numpy restatement of tests/rank_correlation_ref.py against scipy and
against answers worked by hand, the three entry points declared, exported, bound and rejecting bad arguments before any
launch, the new save metrics' names, and the restatement of eval._nanmean_stats (a NaN row moves no mean; the sums of the
shards of a window are the window's).

Bound against scipy: 1e-14 absolute.  Both sides hold exact integers up to the last two or three float64 operations on
magnitudes <= 1 (measured: 5.6e-17 for tau, 1.1e-16 for rho); the bound leaves room for another scipy build's summation order
in spearmanr, which correlates float64 ranks."""
import ctypes
import math
import os
import re
import warnings

import numpy as np
import pytest

from tests import rank_correlation_ref as RC

from reactranker_amd import _lib
from reactranker_amd import train_listwise as TL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rr_rank_correlation_f32", "rr_rank_correlation_waves", "rr_rank_correlation_set_waves"]
LENGTHS = [2, 3, 5, 63, 64, 65, 255, 256, 257, 300, 1000, 4097, 8192]
SCIPY_BOUND = 1e-14


@pytest.mark.parametrize("ties", RC.TIE_LEVELS)
def test_restatement_agrees_with_scipy(ties):
    stats = pytest.importorskip("scipy.stats")
    worst = [0.0, 0.0]
    for n, c in enumerate(LENGTHS):
        s, t = RC.window(100 + n, [c], ties)
        got = RC.query_stats(s, t)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                       # (a constant key: scipy warns and returns NaN, as we do)
            want = (float(stats.kendalltau(s, t).statistic), float(stats.spearmanr(s, t).statistic))
        for k in (0, 1):
            assert math.isnan(got[k]) == math.isnan(want[k]), (c, ties, k, got[k], want[k])
            if not math.isnan(want[k]):
                worst[k] = max(worst[k], abs(got[k] - want[k]))
                assert abs(got[k] - want[k]) <= SCIPY_BOUND, (c, ties, k, got[k], want[k])
        assert got[4:].sum() <= c * (c - 1) // 2
        if ties == 0 and c <= 1000:                               # (float32 normals may collide in a longer list)
            assert got[6] == 0 and got[7] == 0, c
    print(f"[rank_correlation] ties {ties}: worst |tau - scipy| {worst[0]:.2e}, |rho - scipy| {worst[1]:.2e} (bound {SCIPY_BOUND:g})")


def test_known_answers():
    got = RC.query_stats([1, 2, 3, 4], [1, 2, 2, 5])
    assert list(got[4:]) == [5, 0, 0, 1]
    assert got[0] == 0.9128709291752769 and got[1] == 0.9486832980505138
    assert got[2] == 1.0 and got[3] == 0.0
    got = RC.query_stats([1, 2], [2, 1])
    assert got[0] == -1.0 and got[1] == -1.0 and list(got[4:]) == [0, 1, 0, 0]
    assert got[2] == 0.5 and got[3] == 1.0                           # the best target is ranked second; the regret is 2 - 1
    got = RC.query_stats([1, 1, 1], [1, 2, 3])
    assert math.isnan(got[0]) and math.isnan(got[1]) and list(got[4:]) == [0, 0, 3, 0]
    assert got[2] == 1.0 / 3.0 and got[3] == 2.0                     # ties by position: the target's maximum comes last
    got = RC.query_stats([0.25], [7.0])                              # a list of one
    assert math.isnan(got[0]) and math.isnan(got[1]) and list(got[2:]) == [1.0, 0.0, 0, 0, 0, 0]
    got = RC.query_stats([], [])                                     # an empty list
    assert np.isnan(got[:4]).all() and list(got[4:]) == [0, 0, 0, 0]


def test_a_nan_is_tied_with_everything():
    s = np.array([3, np.nan, 1, 2], np.float32)
    t = np.array([4, 3, 2, 1], np.float32)
    got = RC.query_stats(s, t)
    # the three pairs with the NaN are tied in the score only; of the others (3, 1), (3, 2) agree and (1, 2) does not
    assert list(got[4:]) == [2, 1, 3, 0]
    assert got[0] == 1.0 / math.sqrt(3 * 6)
    assert got[2] == 1.0 and got[3] == 0.0


def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(REPO, "include", "reactranker_hip.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\b(rr_\w+)\s*\(", text))
    assert re.search(r"#define\s+RR_RANK_CORR_NSTATS\s+8\b", text)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert getattr(_lib.lib(), s).argtypes is not None
    assert _lib.lib().rr_version() == _lib.ABI_VERSION == 8          # additive: new symbols only
    from reactranker_amd import eval as RE
    assert RE.RANK_CORR_NSTATS == RC.NSTATS == 8 and RE.NSTATS == 12


def test_entry_point_rejects_bad_arguments_before_any_launch():
    fn = _lib.lib().rr_rank_correlation_f32
    one = ctypes.c_void_p(256)
    #   score, stride, targets, seg_off, Q, max_len, stats
    assert fn(None, 1, one, one, 1, 4, one, None) == -1                               # null scores
    assert fn(one, 1, None, one, 1, 4, one, None) == -1                               # null targets
    assert fn(one, 1, one, None, 1, 4, one, None) == -1                               # null seg_off
    assert fn(one, 1, one, one, 1, 4, None, None) == -1                               # null stats
    assert fn(one, 0, one, one, 1, 4, one, None) == -1                                # stride < 1
    assert fn(one, 1, one, one, -1, 4, one, None) == -1                               # Q < 0
    assert fn(one, 1, one, one, 1, 8193, one, None) == -4                             # list too long: nothing launched
    assert fn(one, 1, one, one, 0, 4, one, None) == 0                                 # no queries: nothing launched


def test_wave_count_setter():
    l = _lib.lib()
    assert l.rr_rank_correlation_waves() == 0                                         # by max_len
    try:
        for w in (1, 4, 0):
            assert l.rr_rank_correlation_set_waves(w) == 0 and l.rr_rank_correlation_waves() == w
        for w in (-1, 2, 3, 8):
            assert l.rr_rank_correlation_set_waves(w) == -1 and l.rr_rank_correlation_waves() == 0
    finally:
        l.rr_rank_correlation_set_waves(0)
    assert l.rr_approx_ndcg_waves() == 0                                              # (a word of its own)


def test_save_metric_names():
    assert TL.RANK_CORR_METRICS == ("kendall_tau", "spearman", "mrr")
    assert not set(TL.RANK_CORR_METRICS) & set(TL.NDCG_METRICS)
    # the validation targets of these metrics go through the standardisation (monotone: tau, rho and MRR do not see it)
    _, va, _, _ = TL.standardize_targets([1.0, 2.0, 4.0], [1.0, 3.0], "lgk", True, "kendall_tau")
    assert not np.array_equal(va, [1.0, 3.0]) and va[0] < va[1]


def test_a_nan_row_moves_no_mean_and_shards_add_up():
    scope = [5, 1, 0, 7, 3, 64, 2]
    s, t = RC.window(7, scope)
    t[5 + 1:5 + 1 + 7] = 0.5                                         # query 3: constant targets - tau and rho undefined
    stats = RC.window_stats(s, scope, t)
    assert np.isnan(stats[1, 0]) and np.isnan(stats[2]).sum() == 4 and np.isnan(stats[3, :2]).all() and not np.isnan(stats[3, 2:]).any()
    sums, counts = RC.nanmean_stats(stats)
    assert list(counts) == [4, 4, 6, 6, 7, 7, 7, 7]
    defined = [0, 4, 5, 6]
    assert sums[0] == np.sum(stats[defined, 0]) and sums[1] == np.sum(stats[defined, 1])
    d = RC.summary(sums, counts)
    assert d["kendall_tau"] == sums[0] / 4 and d["n_defined"] == 4 and d["mrr"] == sums[2] / 6
    # dropping the rows without a defined tau changes neither its sum nor its count
    s2, c2 = RC.nanmean_stats(stats[defined])
    assert s2[0] == sums[0] and c2[0] == counts[0] and s2[1] == sums[1]
    # two shards: the integer columns add exactly, the float columns to rounding
    a, b = RC.nanmean_stats(stats[:3]), RC.nanmean_stats(stats[3:])
    assert np.array_equal(a[1] + b[1], counts) and np.array_equal(a[0][4:] + b[0][4:], sums[4:])
    assert np.max(np.abs(a[0][:4] + b[0][:4] - sums[:4])) <= 1e-15 * 7
    both = RC.summary(a[0] + b[0], a[1] + b[1])
    assert both["pairs"] == d["pairs"] and both["kendall_tau_pooled"] == d["kendall_tau_pooled"] and both["n_defined"] == 4
    # nothing defined anywhere: NaN means, not an error
    e = RC.summary(*RC.nanmean_stats(RC.window_stats(s[:1], [1, 0], t[:1])))
    assert math.isnan(e["kendall_tau"]) and math.isnan(e["spearman"]) and e["mrr"] == 1.0 and e["n_defined"] == 0
    assert math.isnan(e["kendall_tau_pooled"]) and e["pairs"] == [0.0] * 4
    e = RC.summary(*RC.nanmean_stats(np.zeros((0, 8))))
    assert math.isnan(e["mrr"]) and math.isnan(e["regret"]) and e["n_defined"] == 0
