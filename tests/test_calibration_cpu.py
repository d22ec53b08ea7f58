"""CPU-side checks of the calibration entries: the four new symbols declared, exported, bound and rejecting
bad arguments before any launch; the properties of the float64 restatement tests/calibration_ref.py (covered <=> E <= tau, the
set is a rank prefix that grows with tau, the closed-form sigma scale); that the GPU tests' pointwise inputs have no row on a
PIT bin edge; and the split-conformal guarantee on the restatement alone.

Bounds.  fit: the standard error of a standard deviation estimated from n samples is s / sqrt(2 n); three of them.  Coverage:
with n test queries the covered share has standard deviation at most sqrt(alpha (1 - alpha) / n) around a mean >= 1 - alpha;
three of them, 0.773 at alpha = 0.2 and n = 2,000."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import calibration_ref as CR

from reactranker_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rr_gauss_calibration_f64", "rr_top1_sets_f32", "rr_top1_sets_waves", "rr_top1_sets_set_waves"]
GAUSS_SIZES = (1, 255, 256, 257, 65537)       # tests/test_gpu_calibration.py runs these
GAUSS_BINS = (1, 10, 20, 64)
GAUSS_SCALES = (1.0, 1.7)
TAUS = (0.0, 0.5, 0.9375, 1.0, float("inf"))


# ------------------------------------------------------------------------------------------------ symbols and statuses
def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(REPO, "include", "reactranker_hip.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\b(rr_\w+)\s*\(", text))
    assert re.search(r"#define\s+RR_GAUSS_CAL_NSUMS\s+8\b", text) and re.search(r"#define\s+RR_TOP1_NSTATS\s+9\b", text)
    assert re.search(r"#define\s+RR_GAUSS_CAL_MAX_BINS\s+64\b", text)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert getattr(_lib.lib(), s).argtypes is not None
    assert _lib.lib().rr_version() == _lib.ABI_VERSION == 8          # additive: new symbols only
    from reactranker_amd import uncertainty as U
    assert U.GAUSS_CAL_NSUMS == CR.GAUSS_NSUMS == 8 and U.TOP1_NSTATS == CR.TOP1_NSTATS == len(U.TOP1_STAT_NAMES) == 9
    assert U.GAUSS_CAL_MAX_BINS == 64 and U.CAL_BLOCK == 256


def test_gauss_entry_rejects_bad_arguments_before_any_launch():
    fn = _lib.lib().rr_gauss_calibration_f64
    one, big = ctypes.c_void_p(256), ctypes.c_size_t(1 << 20)
    #   mean, std, target, n, sigma_scale, n_bins, workspace, workspace_bytes, out
    assert fn(None, one, one, 4, 1.0, 10, one, big, one, None) == -1
    assert fn(one, None, one, 4, 1.0, 10, one, big, one, None) == -1
    assert fn(one, one, None, 4, 1.0, 10, one, big, one, None) == -1
    assert fn(one, one, one, 4, 1.0, 10, None, big, one, None) == -1
    assert fn(one, one, one, 4, 1.0, 10, one, big, None, None) == -1
    assert fn(one, one, one, 0, 1.0, 10, one, big, one, None) == -1                   # n < 1
    for bins in (0, -1, 65):
        assert fn(one, one, one, 4, 1.0, bins, one, big, one, None) == -1
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert fn(one, one, one, 4, scale, 10, one, big, one, None) == -1
    # two blocks of 256 rows, 8 + 10 doubles each: 288 bytes are needed
    assert fn(one, one, one, 257, 1.0, 10, one, ctypes.c_size_t(2 * 18 * 8 - 1), one, None) == -5     # RR_ERR_WORKSPACE


def test_top1_entry_rejects_bad_arguments_before_any_launch():
    fn = _lib.lib().rr_top1_sets_f32
    one = ctypes.c_void_p(256)
    #   p, stride, targets, seg_off, Q, max_len, tau, rank, before, in_set, stats
    good = [one, 1, one, one, 1, 4, 0.5, one, one, one, one, None]
    for k in (0, 2, 3, 7, 8, 9, 10):                                                  # each pointer null in turn
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, k
    for k, bad in ((1, 0), (4, -1), (5, -1), (6, -0.25), (6, float("nan")), (6, float("-inf"))):
        args = list(good)
        args[k] = bad
        assert fn(*args) == -1, (k, bad)
    args = list(good)
    args[5] = 8193
    assert fn(*args) == -4                                                            # list too long: nothing launched
    args = list(good)
    args[4], args[6] = 0, float("inf")
    assert fn(*args) == 0                                                             # no queries: nothing launched


def test_wave_count_setter():
    l = _lib.lib()
    assert l.rr_top1_sets_waves() == 0                                                # by max_len
    try:
        for w in (1, 4, 0):
            assert l.rr_top1_sets_set_waves(w) == 0 and l.rr_top1_sets_waves() == w
        for w in (-1, 2, 3, 8):
            assert l.rr_top1_sets_set_waves(w) == -1 and l.rr_top1_sets_waves() == 0
    finally:
        l.rr_top1_sets_set_waves(0)
    assert l.rr_rank_correlation_waves() == 0                                         # (a word of its own)


def test_python_layer_checks_its_arguments_without_a_gpu():
    from reactranker_amd import uncertainty as U
    for alpha in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            U.conformal_threshold([0.1, 0.2], alpha)
    e = [0.5, float("nan"), 0.0, 0.25, 1.0]                                           # n = 4 after the NaN is dropped
    assert U.conformal_threshold(e, 0.5) == CR.conformal_threshold(e, 0.5) == 0.5     # k = ceil(5 * 0.5) = 3
    assert U.conformal_threshold(e, 0.25) == 1.0                                      # k = 4
    assert U.conformal_threshold(e, 0.1) == math.inf                                  # k = 5 > n
    assert U.conformal_threshold([], 0.5) == math.inf
    stats = np.zeros((5, 9))
    stats[:, 0] = [1, 0, 1, 1, np.nan]                                                # the last row: an empty list
    stats[:, 1] = [0.95, 0.95, 0.5, 1.0, np.nan]
    stats[:, 4] = [0.1, 0.9, 0.5, 0.0, np.nan]
    got = U.top1_calibration(stats, 10)
    assert got["n"] == 4 and got["accuracy"] == 0.75 and got["brier"] == 0.375
    # bins 9 (0.95, 0.95, 1.0: accuracy 2/3, confidence 2.9/3) and 5 (0.5: accuracy 1)
    want = 0.75 * abs(2 / 3 - 2.9 / 3) + 0.25 * 0.5
    assert abs(got["ece"] - want) <= 1e-15 and abs(CR.ece(stats, 10) - want) <= 1e-15
    assert list(got["bin_count"]) == [0, 0, 0, 0, 0, 1, 0, 0, 0, 3] and np.isnan(got["bin_accuracy"][0])
    with pytest.raises(ValueError):
        U.top1_sets(np.zeros(3), [3], np.zeros(3), -1.0)                              # tau is checked first


# ------------------------------------------------------------------------------------------------ the restatement
def test_known_answers_of_the_restatement():
    #            p: ranks 2, 1, 4, 3 (the tie at 0.25 by position); the true top (first maximum of the targets) is position 2
    p, t = np.array([0.25, 0.5, 0.0, 0.25], np.float32), np.array([1, 0, 3, 3], np.float32)
    rank, before, inside, stats = CR.window_sets(p, [4, 0], t, 0.75)
    assert list(rank) == [2, 1, 4, 3] and list(before) == [0.5, 0.0, 1.0, 0.75] and list(inside) == [True, True, False, True]
    brier = 0.25 ** 2 + 0.5 ** 2 + 1.0 + 0.25 ** 2
    assert list(stats[0]) == [0.0, 0.5, 0.0, 4.0, brier, 1.0, 3.0, 0.0, 1.0]
    assert np.isnan(stats[1, :6]).all() and list(stats[1, 6:]) == [0, 0, 0]           # an empty list
    _, _, inside, stats = CR.window_sets(p, [4], t, 1.0)                              # E = 1 <= tau = 1: every candidate
    assert inside.all() and stats[0, 6] == 4 and stats[0, 7] == 1


@pytest.mark.parametrize("kind", ["shares", "softmax"])
def test_covered_is_e_below_tau_and_the_set_is_a_growing_rank_prefix(kind):
    scope = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 300]
    p, t = (CR.sample_share_window if kind == "shares" else CR.softmax_window)(3, scope, ties=True)
    cores = CR.window_core(p, scope, t)
    last = None
    for tau in TAUS:
        rank, before, inside, stats = CR.window_sets(p, scope, t, tau, cores)
        live = ~np.isnan(stats[:, 0])
        assert np.array_equal(stats[live, 7] == 1, stats[live, 5] <= tau)             # covered <=> E <= tau
        off = 0
        for q, c in enumerate(scope):
            r, b, s = rank[off:off + c], before[off:off + c], inside[off:off + c]
            off += c
            if c == 0:
                continue
            assert sorted(r) == list(range(1, c + 1))                                 # a permutation: the order is total
            order = np.argsort(r)
            assert np.all(np.diff(b[order]) >= 0)                                     # before is non-decreasing in rank
            size = int(stats[q, 6])
            assert size >= 1 and set(r[s]) == set(range(1, size + 1))                 # a non-empty prefix of the order
        if last is not None:
            assert np.all(stats[:, 6] >= last)                                        # the set grows with tau
        last = stats[:, 6].copy()
    assert np.array_equal(last[1:], scope[1:])                                        # tau = inf: every candidate
    if kind == "shares":                                                              # dyadic: 0.9375 is hit exactly
        _, before, _, _ = CR.window_sets(p, scope, t, 0.0, cores)
        assert (before == 0.9375).any() and np.all(before * 32 == np.round(before * 32))


def test_closed_form_sigma_scale():
    n = 20000
    rng = np.random.default_rng(11)
    mu, sd = rng.standard_normal(n), rng.uniform(0.05, 3.0, n)
    y = mu + 1.5 * sd * rng.standard_normal(n)
    o = CR.gauss_calibration(mu, sd, y, 1.0, 1)["sums"]
    fit = math.sqrt(o[3] / o[0])
    print(f"[calibration] fitted sigma scale {fit:.4f} (true 1.5, bound {3 * 1.5 / math.sqrt(2 * n):.4f})")
    assert abs(fit - 1.5) <= 3 * 1.5 / math.sqrt(2 * n)
    after = CR.probabilistic(CR.gauss_calibration(mu, sd, y, fit, 20))
    assert abs(after["z2_mean"] - 1.0) <= 1e-9
    before = CR.probabilistic(CR.gauss_calibration(mu, sd, y, 1.0, 20))
    assert after["nll"] < before["nll"] and after["miscalibration_area"] < before["miscalibration_area"]


def test_the_gpu_tests_pointwise_inputs_have_no_row_on_a_bin_edge():
    for n in GAUSS_SIZES:
        rows = CR.gauss_rows(n, n)                                                    # (the seed is the size)
        for scale in GAUSS_SCALES:
            for bins in GAUSS_BINS:
                ref = CR.gauss_calibration(*rows, scale, bins)
                assert ref["edge"] == 0, (n, scale, bins)
                assert ref["hist"].sum() == ref["sums"][0] == n
    mean, std, target, bad = CR.inject_invalid(*CR.gauss_rows(257, 257))
    ref = CR.gauss_calibration(mean, std, target, 1.0, 10)
    assert bad == 4 and list(ref["sums"][:2]) == [253, 4] and ref["hist"].sum() == 253


# ------------------------------------------------------------------------------------------------ the conformal guarantee
def conformal_run(seed, alpha, n=2000, noise=1.0):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(2):                                                                # calibration, test: the same law
        scope = [int(c) for c in rng.integers(2, 41, n)]
        p, t = CR.sample_share_window(int(rng.integers(1 << 30)), scope, T=32, noise=noise)
        out.append((p, scope, t, CR.window_core(p, scope, t)))
    (pc, sc, tc, cc), (pt, st, tt, ct) = out
    tau = CR.conformal_threshold(CR.window_sets(pc, sc, tc, 0.0, cc)[3][:, 5], alpha)
    _, _, inside, stats = CR.window_sets(pt, st, tt, tau, ct)
    return tau, stats, np.asarray(st)


def test_conformal_coverage_on_the_restatement():
    alpha, n = 0.2, 2000
    bound = 1 - alpha - 3 * math.sqrt(alpha * (1 - alpha) / n)
    assert abs(bound - 0.773) < 5e-4
    tau, stats, scope = conformal_run(5, alpha, n)
    coverage, size = stats[:, 7].mean(), stats[:, 6].mean()
    print(f"[calibration] alpha {alpha}: tau {tau:.5f}, test coverage {coverage:.4f} (bound {bound:.4f}), mean set size {size:.2f} "
          f"of {scope.mean():.2f} candidates")
    assert coverage >= bound
    assert 1.0 <= size < scope.mean()                                                 # the sets are not the whole lists


def test_a_true_top_of_probability_zero_puts_tau_at_one():
    # with 32 noisy samples per list (noise 1.5 against a unit spread of the utilities) more than a tenth of the true tops are
    # never sampled as the top: p = 0, every positive p is ahead, E = 1 exactly (a sum of 32nds), so at alpha = 0.1 tau = 1
    # and the set is the whole list - honest, not useful
    tau, stats, scope = conformal_run(5, 0.1, noise=1.5)
    assert (stats[:, 2] == 0).mean() > 0.1 and np.all(stats[stats[:, 2] == 0, 5] == 1.0)
    assert tau == 1.0
    assert np.array_equal(stats[:, 6], scope) and stats[:, 7].all()
