"""The CPU half of the value-range tests (tests/loss_range.py, tests/test_gpu_loss_range.py): that the inputs do what the
device tests assume, with no kernel involved - every float64 reference finite where a pair is not skipped, the float32
oracle's finite / non-finite pattern in each documented case, the distance of the hand-built cases' exp arguments from the
float32 thresholds, the stable restatement against the reference's pair form, and every yardstick figure against the one
recorded in tests/loss_range.py."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import loss_range as L
from tests import loss_variants_ref as R


def test_window_and_targets():
    assert L.SCOPE == [1, 2, 7, 64, 65, 130, 300] and L.M == 569
    t, off = L.base()["targets"], 0
    for c in L.SCOPE:
        assert len(np.unique(t[off:off + c])) == c                         # no ties
        off += c
    v = L.inputs("var_floor")["var"]
    assert np.all(v[::2] == L.VAR_FLOOR) and abs(float(L.VAR_FLOOR) - 1.002e-6) < 1e-9
    assert 45 < float(L.inputs("var_wide")["var"].max()) < 70 and 140 < float(L.inputs("var_over")["var"].max()) < 200
    assert float(L.inputs("far_targets")["targets"].min()) > L.EXP_OVERFLOW + L.MARGIN      # un-shifted float32 gains: all inf


def test_every_pair_reads_what_its_regime_changes_and_the_skipped_ones_are_the_non_finite_ones():
    assert len(L.PAIRS) == 166 and len(L.FINITE_PAIRS) == 166 - len(L.SKIPPED) - len(L.F32_OVERFLOW)
    for kind in L.KINDS:                                                   # every kernel meets every regime of its columns
        assert any(k == kind for k, _ in L.FINITE_PAIRS), kind
    bad = {p for p in L.PAIRS if not L.is_finite(L.reference(*p))}
    assert bad == set(L.SKIPPED), bad ^ set(L.SKIPPED)
    for p in L.CASE2_PAIRS:
        assert L.is_finite(L.reference(*p)) and L.is_finite(L.float32_run(*p)), p


def test_every_yardstick_is_within_its_recorded_figure():
    """prints the float32 CPU figure of every pair next to the bound it gives; none may exceed what the module records"""
    for kind, regime in L.FINITE_PAIRS + L.CASE2_PAIRS:
        assert L.is_finite(L.float32_run(kind, regime)), (kind, regime)
        e, bound = L.yardstick(kind, regime)
        cap = L.YARDSTICK_ABOVE.get((kind, regime), 1.25e-6)
        print(f"[loss range] {kind} {regime}: float32 CPU error {e:.3e} (recorded: at most {cap:g}) -> bound {bound:g}")
        assert e <= cap, (kind, regime, e, cap)
        assert bound == (L.BOUND if e <= 1.25e-6 or kind in L.DOUBLE_KERNELS else 8 * e)
    for pair, cap in L.YARDSTICK_ABOVE.items():                            # and nothing is recorded larger than it need be
        assert L.yardstick(*pair)[0] > min(1.25e-6, cap / 1.5), pair


@pytest.mark.parametrize("kind", L.FACTORISED)
def test_stable_restatement_is_the_reference_form_in_float64(kind):
    for regime in ("base", "up20", "spread8", "var_wide", "var_over", "up120"):
        if (kind, regime) in L.SKIPPED:
            continue
        a = L.evaluate(kind, L.inputs(regime), torch.float64, stable=True)
        b = L.evaluate(kind, L.inputs(regime), torch.float64)
        assert max(L.errors(kind, a, b)) <= 1e-12, (kind, regime)


def test_nig_restatement_is_loss_variants_ref_in_float64():
    for regime in ("base", "evidence_small", "evidence_large"):
        d = L.inputs(regime)
        a = L.nig([d[c] for c in L.KINDS["nig"][0]], d["targets"], True)
        b = R.nig_cross(d["score"], d["nu"], d["alpha"], d["beta"], d["targets"], L.NIG_LAM, L.NIG_EPS)
        assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0])
        for x, y in zip(a[1], b[1:]):
            assert L.grad_error(x, y) <= 1e-10, regime                     # (nig_cross's own digamma series: 1.5e-12)


def _distance(args):
    args = np.asarray(args, np.float64).reshape(-1)
    return min(float(np.min(np.abs(args - th))) for th in (L.EXP_OVERFLOW, L.EXP_SUBNORMAL, L.EXP_ZERO))


@pytest.mark.parametrize("regime", ["up120", "down120"])
def test_case_1_listmle_at_120(regime):
    """float32 oracle: the loss finite and that of up20, no gradient entry finite (inf * 0 at +120, 0 * inf at -120), and
    LogCumsumExp alone the same.  Its exp arguments: x - max (in [-8, 0]), x itself and -fd.  At +-120 the closest of them
    to a float32 threshold is 13 away from the zero threshold (-103.3), not 15: |z| reaches 3.3 over 569 draws and the case is
    fixed at 120; exp() there is 1e-51 .. 1e-54 against a smallest subnormal of 1.4e-45, five orders of magnitude beyond
    what a 1-ulp expf or a flush to zero can change.  Held at 12."""
    d = L.inputs(regime)
    f32, f64 = L.evaluate("mle", d, torch.float32), L.evaluate("mle", d, torch.float64)
    assert np.isfinite(f32[0]) and int(np.isfinite(f32[1][0]).sum()) == 0
    assert L.is_finite(f64) and abs(f64[0] - L.reference("mle", "up20")[0]) <= L.BOUND * f64[0]
    assert abs(f32[0] - f64[0]) <= 1.25e-6 * f64[0]
    x = torch.tensor(np.array(d["score"]), requires_grad=True)
    y = O.LogCumsumExp.apply(x)
    y.sum().backward()
    assert bool(torch.isfinite(y).all()) and int(torch.isfinite(x.grad).sum()) == 0
    s = d["score"].astype(np.float64)
    fd, off = [], 0
    for c in L.SCOPE:                                                      # fd of each list sorted by target
        q = s[off:off + c][np.argsort(-d["targets"][off:off + c], kind="stable")]
        fd.append(np.logaddexp.accumulate(q[::-1])[::-1])
        off += c
    dist = _distance(np.concatenate([s, -np.concatenate(fd)]))
    print(f"[loss range] case 1 {regime}: closest exp argument to a float32 threshold {dist:.2f}")
    assert dist >= 12.0


def test_case_3_listnet_at_spread_60():
    """float32 oracle: loss +inf (log of an underflowed softmax), 3 of 569 autograd gradient entries finite - the
    one- and two-candidate lists; float64 finite"""
    d = L.inputs("spread60")
    f32, f64 = L.evaluate("listnet", d, torch.float32), L.evaluate("listnet", d, torch.float64)
    assert f32[0] == float("inf")
    assert np.nonzero(np.isfinite(f32[1][0]))[0].tolist() == [0, 1, 2]
    assert L.is_finite(f64)
    s = d["score"].astype(np.float64)
    off = np.concatenate([[0], np.cumsum(L.SCOPE)])
    for i in range(2, len(L.SCOPE)):                                       # every longer list has a softmax entry that is zero
        q = s[off[i]:off[i + 1]]
        assert float(np.min(q - q.max())) < L.EXP_ZERO - L.MARGIN, L.SCOPE[i]
    q = s[1:3]
    assert _distance([-abs(q[0] - q[1])]) >= L.MARGIN                       # the two-candidate list is clear of every threshold


def test_case_4_ranknet_list_has_one_overflowing_pair():
    scope, s, t = L.ranknet_overflow_case()
    assert scope == [70] and len(np.unique(t)) == 70
    args = L.ranknet_case_arguments()
    assert len(args) == 70 * 69 // 2 and int((args > L.EXP_OVERFLOW).sum()) == 1 and _distance(args) >= L.MARGIN
    assert float(s.max() - s[40]) > 145
    ts, tt = torch.tensor(np.array(s)), torch.tensor(np.array(t))
    loss, pairs = O.ranknet_sum_session(ts, scope, tt, 1.0)
    # (the oracle multiplies the masked half of the pair matrix by zero: its 0 * inf makes the non-finite loss a NaN, where a
    # sum over the pairs alone gives +inf)
    assert not np.isfinite(float(loss)) and pairs == 70 * 69
    assert bool(torch.isfinite(O.ranknet_lambda(ts, scope, tt, 1.0)).all())
    l64, _ = O.ranknet_sum_session(ts.double(), scope, tt.double(), 1.0)
    assert np.isfinite(float(l64))


@pytest.mark.parametrize("kind", L.FACTORISED)
def test_case_5_pair_form_overflows_in_float32_under_var_over(kind):
    wide = L.evaluate(kind, L.inputs("var_wide"), torch.float32)           # the reference's own pair form: finite, and useless
    assert L.is_finite(wide) and max(L.errors(kind, wide, L.reference(kind, "var_wide"))) > 1e-4
    f32 = L.evaluate(kind, L.inputs("var_over"), torch.float32)
    assert f32[0] == float("inf") or not all(np.isfinite(g).all() for g in f32[1])
    assert L.is_finite(L.reference(kind, "var_over")) and L.is_finite(L.float32_run(kind, "var_over"))


def test_exp_mse_leaves_float32_with_raw_targets():
    for regime, finite_entries in (("raw_targets", L.M), ("far_targets", 0)):
        f32 = L.float32_run("exp_mse", regime)
        assert f32[0] == float("inf") and int(np.isfinite(f32[1][0]).sum()) == finite_entries
        assert L.is_finite(L.reference("exp_mse", regime))


def test_case_6_kl_is_nan_for_the_one_query():
    s, t = L.kl_case(), L.base()["targets"]
    assert s[L.KL_AT] == L.KL_SCORE > 104 and L.KL_SCORE >= L.EXP_OVERFLOW + L.MARGIN
    assert float(np.delete(np.abs(s), L.KL_AT).max()) < L.EXP_OVERFLOW - L.MARGIN
    off = np.concatenate([[0], np.cumsum(L.SCOPE)])
    assert off[L.KL_QUERY] <= L.KL_AT < off[L.KL_QUERY + 1]
    _, _, rows = O.calculate_ndcg_from_scores([np.array(s[a:b]) for a, b in zip(off[:-1], off[1:])],
                                              [np.array(t[a:b]) for a, b in zip(off[:-1], off[1:])], 0.5)
    assert np.isnan(rows[L.KL_QUERY, 1]) and np.isfinite(np.delete(rows[:, 1], L.KL_QUERY)).all() and np.isfinite(rows[:, 0]).all()


def test_case_7_head_inputs_are_clear_of_the_thresholds():
    """+-50 is 37 away from every threshold.  The case fixes the other pair at +-110, 6.7 beyond the zero threshold: exp(-110) is
    1.7e-48, 1/800 of the smallest subnormal, so it is zero under either denormal mode, and nothing asserted depends on it -
    it is added to 1e-6 or compared absolutely; the gradient's exp(110) is 21 beyond overflow."""
    assert _distance([50.0, -50.0]) >= L.MARGIN and L.HEAD_RAWS == (50.0, -50.0, 110.0, -110.0)
    assert -110.0 < L.EXP_ZERO - 6 and 110.0 > L.EXP_OVERFLOW + L.MARGIN
    raw = np.array([[110.0, -110.0]])
    out, slope, col_in, act = L.head_reference(raw, 3)                      # (score, softplus + 1e-6)
    assert col_in.tolist() == [0, 1] and act == [False, True]
    assert out[0, 0] == 110.0 and np.float32(out[0, 1]) == np.float32(1e-6) and slope[0, 1] < 1e-47
