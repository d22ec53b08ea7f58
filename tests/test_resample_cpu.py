"""Resampled means without a GPU: the host's draw function against the numpy restatement (tests/resample_ref.py), the stream's
fitness for resampling as CONDITIONS (with the dropout hash as the negative control), the restated chain against exactly
rounded sums, NaN handling, the interval / p-value arithmetic of the oracle and of reactranker_amd.significance on CPU
tensors, the new symbols' declaration, export and binding, and every status code the header lists (all before any launch)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import dropout_ref
from reactranker_amd import _lib
from reactranker_amd import significance as S
from reactranker_amd import uncertainty as U
from tests import resample_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rr_resample_means_f64", "rr_resample_blocks", "rr_resample_set_blocks", "rr_resample_draw_host")
OK, ARG, UNSUPPORTED = 0, -1, -4
PTR = C.c_void_p(4096)          # a non-null pointer that is never followed: every call below returns before a launch
SEEDS = (0, 1, 12345, 2 ** 63 + 7)
u64 = np.uint64


# ---------------------------------------------------------------------------------------------- the stream
def test_host_draw_equals_the_numpy_restatement():
    j = np.concatenate([np.arange(4000, dtype=u64),
                        u64(2 ** 32 - 24) + np.arange(48, dtype=u64),
                        u64(2 ** 63 - 2 - 47) + np.arange(48, dtype=u64)])
    assert len(j) == 4096 and int(j[-1]) == 2 ** 63 - 2
    L = _lib.lib()
    for seed in SEEDS:
        want = R.draws(seed, j)
        got = np.array([L.rr_resample_draw_host(seed, int(v)) for v in j], u64)
        assert np.array_equal(got, want), seed
    # the two halves of one word, by hand
    w = int(R.words(12345, np.array([3], u64))[0])
    assert L.rr_resample_draw_host(12345, 6) == w >> 32 and L.rr_resample_draw_host(12345, 7) == w & 0xFFFFFFFF


def test_mix64_is_the_generator_of_sample_seed():
    vals = [0, 1, 12345, 2 ** 63 + 7, 2 ** 64 - 1, 0x9E3779B97F4A7C15]
    assert [int(v) for v in R.mix64(np.array(vals, u64))] == [U._mix64(v) for v in vals]
    for seed in SEEDS:
        for t in (0, 1, 7):
            assert int(R.words(seed, np.array([t], u64))[0]) >> 2 == U.sample_seed(seed, t)


def test_positions_of_a_resample_start_on_a_word_boundary():
    # Q = 5: Qe = 6, resample 2 starts at j = 12; Q = 4: Qe = 4
    assert np.array_equal(R.resample_draws(9, 2, 5), R.draws(9, np.arange(12, 17, dtype=u64)))
    assert np.array_equal(R.resample_draws(9, 3, 4), R.draws(9, np.arange(12, 16, dtype=u64)))
    big = R.resample_draws(9, 2 ** 33, 5)                              # j crosses 2^32 inside the 64-bit product
    assert np.array_equal(big, R.draws(9, u64(6 * 2 ** 33) + np.arange(5, dtype=u64)))
    assert (R.rows(9, 7, 5) < 5).all() and set(np.unique(R.signs(9, 7, 64))) == {-1.0, 1.0}


def _flat_draws(seed, Q, B):
    Qe = (Q + 1) & ~1
    j = (np.arange(B, dtype=u64)[:, None] * u64(Qe) + np.arange(Q, dtype=u64)[None, :])
    return R.draws(seed, j)                                            # [B, Q]


def _z(chi2, df):
    return (chi2 - df) / math.sqrt(2.0 * df)


def _cells_z(a, b):
    """z of the chi-square of the 8 x 8 table of two 3-bit symbols"""
    n = np.bincount((a * u64(8) + b).astype(np.int64), minlength=64).astype(np.float64)
    e = n.sum() / 64.0
    return _z(float(((n - e) ** 2 / e).sum()), 63)


def _top(d):
    return d >> u64(29)


@pytest.mark.parametrize("Q", [3, 16, 257, 1000])
@pytest.mark.parametrize("seed", SEEDS)
def test_the_stream_is_fit_for_resampling(seed, Q):
    B = 4000
    d = _flat_draws(seed, Q, B)
    rows = ((d * u64(Q)) >> u64(32)).astype(np.int64)
    # every row is drawn equally often
    n = np.bincount(rows.ravel(), minlength=Q).astype(np.float64)
    assert abs(_z(float(((n - B) ** 2 / B).sum()), Q - 1)) <= 4
    # no dependence between a draw and the next ones, between the halves of a word, or in the low bits
    f = d.ravel()
    for lag in (1, 2, 3, 4):
        assert abs(_cells_z(_top(f[:-lag]), _top(f[lag:]))) <= 4, lag
    w = R.words(seed, np.arange(B * Q // 2, dtype=u64))
    assert abs(_cells_z(_top(w >> u64(32)), _top(w & u64(0xFFFFFFFF)))) <= 4
    assert abs(_cells_z(f[:-1] & u64(7), f[1:] & u64(7))) <= 4
    # the resampled mean of a fixed vector has the variance theory gives it
    x = np.random.default_rng(Q).standard_normal(Q)
    slack = 5.0 * math.sqrt(2.0 / B)
    ratio = x[rows].mean(axis=1).var() / (x.var() / Q)
    assert abs(ratio - 1.0) <= slack, ratio
    sign = np.where((d >> u64(31)) == 0, 1.0, -1.0)
    ratio = (sign * x).mean(axis=1).var() / ((x * x).mean() / Q)
    assert abs(ratio - 1.0) <= slack, ratio


def test_the_dropout_hash_is_not_fit_for_resampling():
    """Why rr_hash_u32 was not used: the four elements that share a first-level word are correlated (harmless for a keep mask).
    The same pair tests at Q = 1000, B = 4000 (10^6 groups), measured for seeds 0, 1, 12345, 2^63 + 7: elements (0, 3) z = 31 to 35
    in the low three bits (-1.3 to -0.1 in the top three), elements (1, 2) z = 68 to 76 in the top three bits, adjacent draws
    z = 15 to 18 in the top three bits and 62 to 68 in the low three."""
    g = np.arange(1000 * 4000 // 4, dtype=u64) * u64(4)
    e = [dropout_ref.hash_u32(12345, g + u64(k)) for k in range(4)]
    assert _cells_z(e[0] & u64(7), e[3] & u64(7)) > 10
    assert _cells_z(_top(e[1]), _top(e[2])) > 10
    f = dropout_ref.hash_u32(12345, np.arange(1000 * 4000, dtype=u64))
    assert _cells_z(_top(f[:-1]), _top(f[1:])) > 10


# ---------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("mode", [R.BOOTSTRAP, R.SIGNFLIP])
def test_chain_is_exact_on_integers_and_near_fsum_on_floats(mode):
    rng = np.random.default_rng(3)
    for Q, M in ((1, 1), (63, 3), (129, 12), (1000, 2)):
        xi = rng.integers(-8, 9, (Q, M)).astype(np.float64)
        m, n = R.means_chain(xi, 5, seed=7, mode=mode)
        mf, nf, _ = R.means_fsum(xi, 5, seed=7, mode=mode)
        assert np.array_equal(m, mf) and np.array_equal(n, nf) and (n == Q).all()
        xf = rng.standard_normal((Q, M)) * np.exp(rng.standard_normal((Q, M)))
        m, n = R.means_chain(xf, 5, seed=7, mode=mode)
        mf, nf, mass = R.means_fsum(xf, 5, seed=7, mode=mode)
        assert np.array_equal(n, nf)
        assert (np.abs(m - mf) <= Q * 2.0 ** -53 * mass / n + 2.0 ** -53 * np.abs(mf)).all()
    # by hand: Q = 3, resample rows from the stream
    x = np.array([1.0, 10.0, 100.0])
    m, _ = R.means_chain(x, 4, seed=5)
    assert m[:, 0].tolist() == [x[R.rows(5, b, 3)].sum() / 3 for b in range(4)]
    # a later start is the tail of the uncut call
    a, _ = R.means_chain(xf, 6, seed=2, mode=mode)
    b, _ = R.means_chain(xf, 4, seed=2, mode=mode, first=2)
    assert np.array_equal(a[2:], b)


@pytest.mark.parametrize("mode", [R.BOOTSTRAP, R.SIGNFLIP])
def test_nan_entries_are_left_out_and_counted(mode):
    rng = np.random.default_rng(4)
    x = rng.integers(-8, 9, (40, 4)).astype(np.float64)
    x[rng.random((40, 4)) < 0.2] = np.nan
    x[:, 2] = np.nan                                                   # an all-NaN column
    m, n = R.means_chain(x, 9, seed=1, mode=mode)
    mf, nf, _ = R.means_fsum(x, 9, seed=1, mode=mode)
    assert np.array_equal(m, mf, equal_nan=True) and np.array_equal(n, nf)
    assert np.isnan(m[:, 2]).all() and (n[:, 2] == 0).all() and (n[:, [0, 1, 3]] > 0).all()
    if mode == R.SIGNFLIP:
        assert (n == (~np.isnan(x)).sum(axis=0)).all()
    # a column finite in one row only: a resample that never draws that row has nothing to average
    y = np.full((3, 2), np.nan)
    y[1, 0], y[:, 1] = 5.0, [1.0, 2.0, 3.0]
    m, n = R.means_chain(y, 64, seed=3)
    hit = np.array([(R.rows(3, b, 3) == 1).sum() for b in range(64)])
    assert np.array_equal(n[:, 0], hit) and (hit == 0).any() and (hit > 0).any()
    assert np.array_equal(np.isnan(m[:, 0]), hit == 0) and (m[hit > 0, 0] == 5.0).all()
    # no rows at all
    m, n = R.means_chain(np.zeros((0, 3)), 2)
    assert np.isnan(m).all() and (n == 0).all() and m.shape == (2, 3)


# ---------------------------------------------------------------------------------------------- statistics
def _module_ci(x, m, level, method):
    """reactranker_amd.significance's own interval arithmetic on CPU tensors (the same code the device tables go through)"""
    tx, tm = torch.from_numpy(np.asarray(x, np.float64).reshape(len(x), -1)), torch.from_numpy(np.asarray(m, np.float64).reshape(len(m), -1))
    accel = S._acceleration(tx, None) if method == "bca" else None
    out = S._intervals(tm, S._nanmean(tx), level, method, accel)
    return float(out["lo"][0]), float(out["hi"][0])


@pytest.mark.parametrize("value", [3.0, 0.71])
def test_a_constant_column_has_an_interval_of_one_point(value):
    x = np.full(100, value)
    m, _ = R.means_chain(x, 200, seed=1)
    # every resample adds the same numbers; 63 butterfly additions of at most half an ulp each sum to 6 * 2^-47 on a sum near 71,
    # 4.2 spacings of 0.71 once divided by 100, and the quotient rounds once more
    assert np.ptp(m) == 0.0 and abs(m[0, 0] - value) <= 6 * np.spacing(value)
    for method in ("percentile", "bca"):
        lo, hi = _module_ci(x, m, 0.95, method)
        assert lo == hi == m[0, 0]
    assert R.percentile_ci(m[:, 0]) == (m[0, 0], m[0, 0])
    lo, hi, fell_back = R.bca_ci(x, m[:, 0])
    assert lo == hi == m[0, 0] and fell_back                           # the acceleration is 0 / 0: the percentile levels
    if value == 3.0:
        assert m[0, 0] == value
    assert math.isnan(float(S._acceleration(torch.from_numpy(x)[:, None], None)[0]))


def test_equal_models_give_p_one_and_a_hand_counted_p():
    d = np.zeros(50)
    t, _ = R.means_chain(d, 99, seed=2, mode=R.SIGNFLIP)
    assert R.signflip_p(d, t[:, 0]) == 1.0
    d = np.ones(4)                                                     # |T_b| reaches |T_obs| = 1 only when all four signs agree
    t, _ = R.means_chain(d, 64, seed=11, mode=R.SIGNFLIP)
    agree = sum(1 for b in range(64) if abs(R.signs(11, b, 4).sum()) == 4)
    assert R.signflip_p(d, t[:, 0]) == (1 + agree) / 65 and 0 < agree < 64
    assert math.isnan(R.signflip_p(np.full(3, np.nan), np.full(8, np.nan)))


def test_bca_is_percentile_on_a_symmetric_table():
    x = np.array([-3.0, -1.0, 0.0, 1.0, 3.0])                          # symmetric about its mean: a = 0
    half = np.random.default_rng(0).uniform(0.1, 2.0, 250)
    m = np.concatenate([-half, half])                                  # symmetric about the estimate: z0 = 0
    z0, a = R.bca_terms(x, m, 0.0)
    assert z0 == 0.0 and a == 0.0
    want = R.percentile_ci(m, 0.9)
    lo, hi, fell_back = R.bca_ci(x, m, 0.9)
    assert not fell_back and lo == pytest.approx(want[0], abs=1e-12) and hi == pytest.approx(want[1], abs=1e-12)
    assert _module_ci(x, m, 0.9, "bca") == pytest.approx(want, abs=1e-12)
    assert _module_ci(x, m, 0.9, "percentile") == pytest.approx(want, abs=1e-12)


@pytest.mark.parametrize("method", ["percentile", "bca"])
def test_the_module_and_the_oracle_agree_and_wider_levels_give_wider_intervals(method):
    rng = np.random.default_rng(8)
    x = rng.exponential(1.0, 64)                                       # skewed: z0 and a are both away from 0
    m, _ = R.means_chain(x, 500, seed=4)
    last = None
    for level in (0.5, 0.8, 0.95, 0.99):
        want = R.percentile_ci(m[:, 0], level) if method == "percentile" else R.bca_ci(x, m[:, 0], level)[:2]
        assert _module_ci(x, m, level, method) == pytest.approx(want, abs=1e-12)
        assert want[0] < x.mean() < want[1]
        if last is not None:
            assert want[0] < last[0] and want[1] > last[1]
        last = want
    if method == "bca":
        z0, a = R.bca_terms(x, m[:, 0], float(x.mean()))
        assert a > 0.01 and not R.bca_ci(x, m[:, 0])[2]


# ---------------------------------------------------------------------------------------------- the binding
def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "reactranker_hip.h")).read()
    declared = set(re.findall(r"\b(rr_[a-z0-9_]+)\s*\(", hdr))
    l = _lib.lib()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert getattr(l, s).argtypes is not None, s
    assert l.rr_version() == 8 == _lib.ABI_VERSION
    assert "#define RR_RESAMPLE_MAX_COLS 32" in hdr and _lib.RR_RESAMPLE_MAX_COLS == 32 == S.MAX_COLS
    assert "#define RR_RESAMPLE_BOOTSTRAP 0" in hdr and "#define RR_RESAMPLE_SIGNFLIP  1" in hdr
    assert S.MODES == {"bootstrap": 0, "signflip": 1} and S.MAX_ROWS == 2 ** 20
    assert "resample.hip" in open(os.path.join(REPO, "reactranker_amd", "csrc", "Makefile")).read()


def _rs(x=PTR, ld=8, Q=100, M=8, mode=0, seed=1, b0=0, B=5, mean=PTR, count=PTR):
    return _lib.lib().rr_resample_means_f64(x, ld, Q, M, mode, seed, b0, B, mean, count, None)


def test_status_codes_come_back_before_any_launch():
    l = _lib.lib()
    assert _rs(x=None) == ARG and _rs(mean=None) == ARG
    assert _rs(Q=-1) == ARG and _rs(B=-1) == ARG and _rs(b0=-1) == ARG
    assert _rs(M=0) == ARG and _rs(M=-3) == ARG and _rs(ld=7) == ARG
    assert _rs(mode=2) == ARG and _rs(mode=-1) == ARG
    assert _rs(M=33, ld=33) == UNSUPPORTED
    assert _rs(Q=2 ** 20 + 1) == UNSUPPORTED
    assert _rs(Q=4, b0=2 ** 61 - 5, B=5) == UNSUPPORTED                # (b0 + B) * Qe == 2^63
    assert _rs(Q=3, b0=2 ** 62, B=2 ** 62) == UNSUPPORTED
    assert _rs(Q=2 ** 20, b0=2 ** 43, B=1) == UNSUPPORTED
    # B == 0 has nothing to fill and launches nothing - also right below the limits, and without a table when Q == 0
    assert _rs(B=0) == OK and _rs(B=0, count=None) == OK
    assert _rs(Q=4, b0=2 ** 61 - 1, B=0) == OK
    assert _rs(Q=2 ** 20, M=32, ld=32, B=0) == OK
    assert _rs(x=None, Q=0, B=0) == OK
    for b in (0, 1, 7, 4096):
        assert l.rr_resample_set_blocks(b) == OK and l.rr_resample_blocks() == b
    assert l.rr_resample_set_blocks(-1) == ARG and l.rr_resample_set_blocks(4097) == ARG and l.rr_resample_blocks() == 4096
    assert l.rr_resample_set_blocks(0) == OK


def test_python_argument_checks():
    x = torch.zeros(4, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU"):
        S.resample_means(x, 3)
    with pytest.raises(ValueError, match="method"):
        S._intervals(x, x[0], 0.95, "normal", None)
    with pytest.raises(ValueError, match="level"):
        S._intervals(x, x[0], 1.0, "percentile", None)
    with pytest.raises(ValueError, match="names"):
        S._names(["a", "a"], 2, "t")
    assert S._names(None, 2, "t") == ["col0", "col1"]
    assert len(S.TABLE_NAMES) == 12 and S.TABLE_NAMES[8:] == ("kendall_tau", "spearman", "mrr", "regret")
