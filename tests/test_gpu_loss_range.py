"""Every per-list and pointwise loss kernel over the numeric range training reaches, against float64: the value-range
counterpart of tests/test_gpu_long_lists.py.  The window, the regimes, the skipped pairs, the references, the measure and the
rule that sets every bound are in tests/loss_range.py (its docstring also holds every float32 CPU figure a bound comes
from); tests/test_loss_range_cpu.py holds, without a kernel, that the inputs are what these tests assume.

Finite regimes: every kernel x regime of loss_range.FINITE_PAIRS through the public autograd entry points, loss and every
gradient column within the pair's bound of float64.  The losses with a one-launch step run with FusedStep on and off and
must give the same bits.  up20 and var_wide also go through rr_task_loss_step_f32 for the eight composite task types, under
the contract of tests/test_gpu_task_step.py (composite launch against the separate kernels at 1e-5 * (1 + |ref|), two
launches bit for bit).

Documented non-finite behaviour (DESIGN H4 and the factorised pair sums), one test per case.  In each the element-wise
finite / non-finite pattern of the kernel's loss and gradients equals the float32 CPU oracle's - +inf told apart from NaN
only where the test says so - and every finite element is within the bound of float64:
  1  ListMLE and LogCumsumExp at score +- 120: loss finite, no gradient entry finite
  2  the losses whose forms see only differences, or shift, at +- 120: all finite (loss_range.CASE2_PAIRS)
  3  ListNet at 60 z: loss +inf; the kernel's closed-form gradient is finite everywhere (the oracle's autograd gradient is
     finite in 3 of 569 entries) and is pinned to float64 - the deviation DESIGN H4 records
  4  RankNet, one overflowing pair in a 70-candidate list: loss +inf, pair count exact, lambda and backward finite
  5  var_over for the three factorised kernels: finite where the reference's float32 pair form is not
  6  calculate_ndcg's KL with a score of 120: NaN for that query alone
  7  the heads at raw = +-50, +-110
and the regression_exploss expression with raw targets, whose float64 value is finite and whose float32 value is not."""
import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import loss_range as L

from oracle import ref_cpu as O
from reactranker_amd import functions as Fn
from reactranker_amd import loss as RL
from reactranker_amd import train_listwise as TL

pytestmark = pytest.mark.gpu
SCOPE = L.SCOPE
VARIANTS = {"mledis": RL.MLEDisLoss, "listnet_gauss": RL.Listnet_For_Gauss, "listnet_lognorm": RL.Listnetlognorm,
            "listnet_evidential": RL.Listnet_For_evidential, "listnet_uq": RL.Listnet_with_uq, "dirichlet_uq": RL.Dirichlet_uq}


def dev(a, grad=False):
    return torch.tensor(np.array(a)).cuda().requires_grad_(grad)


def host(x):
    return x.detach().double().cpu().numpy().reshape(-1)


def check(what, err, bound):
    Hh.record(what, err, bound)
    print(f"[loss range] {what}: err {err:.3e} (bound {bound:g})")
    assert err <= bound, f"{what}: err {err:.3e} > {bound:g}"


def run(kind, d, fused=True):
    """(value, [gradient per input column]) of `kind` on the columns d through its autograd entry point, as float64 numpy:
    what loss_range.evaluate returns for the CPU"""
    tt = torch.tensor(np.array(d["targets"]))
    leaves = [dev(d[c], True) for c in L.KINDS[kind][0]]
    old = RL.FusedStep.enabled
    RL.FusedStep.enabled = fused
    try:
        hits = RL.FusedStep.hits
        if kind in ("mle", "listnet"):
            l = (RL.MLEloss() if kind == "mle" else RL.ListnetLoss())(leaves[0], SCOPE, tt, 0)
        elif kind == "evid":
            x = torch.stack([leaves[0].detach(), leaves[1].detach()], 1).requires_grad_(True)
            l = RL.evidential_ranking()(x, SCOPE, tt, None, None, None, 0)
            RL.backward(l)
            assert RL.FusedStep.hits == hits + (1 if fused else 0)
            return float(l.detach().double().sum()), [host(x.grad[:, 0]), host(x.grad[:, 1])]
        elif kind == "ranknet":
            ls, pairs = RL.ranknet_loss(leaves[0], SCOPE, tt, 1.0, 0)
            assert int(pairs) == L.ranknet_pairs()                         # exactly
            l = ls / int(pairs)
            l.backward()
            lam = RL.ranknet_lambda(leaves[0].detach(), SCOPE, tt, 1.0, 0) / int(pairs)
            return float(l.detach().double()), [host(leaves[0].grad), host(lam)]
        elif kind in ("listnet_uq", "dirichlet_uq"):
            l = VARIANTS[kind]()(leaves[0], SCOPE, tt, 0.5, 2, 5, 0)
        elif kind in VARIANTS:
            l = VARIANTS[kind]()(*[x[:, None] for x in leaves], SCOPE, tt, 0)
        elif kind == "gauss_nll":
            l = RL.GaussDisLoss()(leaves[0], leaves[1], tt, 0)
        elif kind == "lognorm":
            l = RL.Lognorm()(leaves[0], leaves[1], tt, 0)
        elif kind == "mse":
            l = RL.MSELoss()(leaves[0], tt)
        elif kind == "exp_mse":
            l = RL.ExpMSELoss()(leaves[0], tt)
        elif kind in ("nig", "nig_cross"):
            l = RL.evidential_loss_new(*[x[:, None] if kind == "nig_cross" else x for x in leaves], tt, 0, lam=L.NIG_LAM, epsilon=L.NIG_EPS)
        elif kind.startswith("lambdarank"):
            l, pairs = RL.lambdarank_loss(leaves[0], SCOPE, tt, 1.0, int(kind.split("_k")[1]), 0)
            assert int(pairs) == L.ranknet_pairs()
        elif kind.startswith("approx_ndcg"):
            l, ranked = RL.approx_ndcg_loss(leaves[0], SCOPE, tt, 1.0, int(kind.split("_k")[1]), 0)
            assert int(ranked) == len(SCOPE) - 1
        elif kind == "soft_rank":
            r = RL.soft_rank(leaves[0], SCOPE, 1.0, 0)
            (r * dev(L.soft_rank_upstream())).sum().backward()
            return host(r), [host(leaves[0].grad)]
        else:
            fn = RL.betanet_loss if kind == "betanet" else RL.beta_evidential_loss
            l, pairs = fn(leaves[0], SCOPE, tt, L.BETA_PARAM[kind], 0)
            assert int(pairs) == L.ranknet_pairs()
        if kind in L.STEP_KINDS:
            RL.backward(l)
            assert RL.FusedStep.hits == hits + (1 if fused else 0), (kind, fused)
        else:
            l.sum().backward()
        return float(l.detach().double().sum()), [host(x.grad) for x in leaves]
    finally:
        RL.FusedStep.enabled = old


def same_bits(a, b):
    """two runs' (value, gradients) agree bit for bit where finite and in their finite / non-finite pattern elsewhere"""
    xs = [np.atleast_1d(np.asarray(a[0]))] + list(a[1])
    ys = [np.atleast_1d(np.asarray(b[0]))] + list(b[1])
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(xs, ys))


def run_both_paths(kind, d, log=None):
    """the step launch, and for the losses that have one also forward kernel + backward kernel, which must give its bits"""
    got = run(kind, d, fused=True)
    if kind in L.STEP_KINDS:
        two = run(kind, d, fused=False)
        assert same_bits(got, two), f"{kind}: the one-launch step and the two-kernel path differ"
        if log:
            log(f"{kind}: fused step == two-kernel path bit for bit")
    return got


# ------------------------------------------------------------------------------------------------ the finite regimes, and case 2
@pytest.mark.parametrize("kind,regime", L.FINITE_PAIRS + L.CASE2_PAIRS, ids=lambda v: v)
def test_kernel_against_float64_in_regime(kind, regime, parity_log):
    ref = L.reference(kind, regime)
    assert L.is_finite(ref)
    e32, bound = L.yardstick(kind, regime)
    Hh.record(f"{kind} {regime}: float32 CPU restatement, sets the bound beside it", e32, bound)
    print(f"[loss range] {kind} {regime}: float32 CPU error {e32:.3e} -> bound {bound:g}")
    got = run_both_paths(kind, L.inputs(regime), parity_log)
    assert L.is_finite(got), (kind, regime)
    for label, err in zip(L.labels(kind), L.errors(kind, got, ref)):
        check(f"{kind} {regime} {label}", err, bound)


# ------------------------------------------------------------------------------------------------ the composite task step
TASKS = ["mle_gaussian", "listnet_gauss", "mle_regression", "listnet_regression", "mledis_gaussian", "listnetdis_gauss",
         "listnet_uq", "dirichlet_uq"]


def task_output(task, regime):
    d = L.inputs(regime)
    if task in ("mle_regression", "listnet_regression"):
        return np.array(d["score"])
    if task == "listnet_uq":
        return np.array(d["pos"])
    if task == "dirichlet_uq":                               # a score regime's positive scores serve as concentrations
        return np.array(d["pos"] if "score" in L.changed(regime) else d["conc"])
    if task == "mledis_gaussian":                            # the second column is log(variance) for the list term and the
        return np.stack([d["score"], np.log1p(d["var"])], 1).astype(np.float32)      # variance itself for the Gaussian term: > 0
    return np.stack([d["score"], d["var"]], 1)


def close(got, ref, what, tol=1e-5):                         # tests/test_gpu_task_step.py's
    got, ref = host(got), host(ref)
    err = float(np.max(np.abs(got - ref) / (1 + np.abs(ref))))
    check(what, err, tol)


@pytest.mark.parametrize("regime", ["up20", "var_wide"])
@pytest.mark.parametrize("task", TASKS)
def test_task_step_against_its_separate_kernels_in_regime(task, regime):
    o_np, tt = task_output(task, regime), torch.tensor(np.array(L.inputs(regime)["targets"]))

    def once(fused):
        old = RL.FusedStep.enabled
        RL.FusedStep.enabled = fused
        try:
            o = dev(o_np, True)
            hits = RL.FusedStep.hits
            l = TL.batch_loss(task, o, SCOPE, tt, 0, 2, 5, 0.5)
            RL.backward(l)
            assert RL.FusedStep.hits == hits + (1 if fused else 0)
            return l.detach(), o.grad
        finally:
            RL.FusedStep.enabled = old

    lp, gp = once(False)
    l1, g1 = once(True)
    l2, g2 = once(True)
    assert torch.equal(l1, l2) and torch.equal(g1, g2), "two launches differ"
    assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(g1).all()) and bool(torch.isfinite(gp).all())
    close(l1, lp, f"{task} {regime} fused_vs_per_term.loss")
    close(g1, gp, f"{task} {regime} fused_vs_per_term.grad")


# ------------------------------------------------------------------------------------------------ case 1
@pytest.mark.parametrize("regime", ["up120", "down120"])
def test_case_1_listmle_at_120_has_a_finite_loss_and_no_finite_gradient(regime):
    d = L.inputs(regime)
    ref = L.evaluate("mle", d, torch.float64)
    oracle = L.evaluate("mle", d, torch.float32)
    assert np.isfinite(oracle[0]) and not np.isfinite(oracle[1][0]).any()
    for fused in (True, False):
        got = run("mle", d, fused)
        check(f"mle {regime} loss (fused {fused})", L.value_error("mle", got[0], ref[0]), L.BOUND)
        assert not np.isfinite(got[1][0]).any(), int(np.isfinite(got[1][0]).sum())
    x = dev(d["score"], True)                               # LogCumsumExp.apply alone, the whole window as one list
    y = RL.LogCumsumExp.apply(x)
    y.sum().backward()
    xr = torch.tensor(np.array(d["score"])).double()
    yr = torch.logcumsumexp(xr.flip(0), 0).flip(0).numpy()
    check(f"logcumsumexp {regime} value", L.grad_error(host(y), yr), L.BOUND)
    assert not np.isfinite(host(x.grad)).any()


# ------------------------------------------------------------------------------------------------ case 3
def test_case_3_listnet_at_spread_60_is_inf_with_a_finite_closed_form_gradient(parity_log):
    d = L.inputs("spread60")
    ref = L.evaluate("listnet", d, torch.float64)
    oracle = L.evaluate("listnet", d, torch.float32)
    assert oracle[0] == float("inf") and int(np.isfinite(oracle[1][0]).sum()) == 3
    # the yardstick of the closed form softmax(s) * sum(softmax(t)) - softmax(t) over M, in float32 on the CPU
    s32, t32 = torch.tensor(np.array(d["score"])), torch.tensor(np.array(d["targets"]))
    closed = torch.cat([torch.softmax(a, 0) * torch.softmax(b, 0).sum() - torch.softmax(b, 0)
                        for a, b in zip(s32.split(SCOPE), t32.split(SCOPE))]) / L.M
    e32 = L.grad_error(closed.double().numpy(), ref[1][0])
    bound = L.rule(e32)
    Hh.record("listnet spread60: float32 CPU closed form, sets the bound beside it", e32, bound)
    got = run_both_paths("listnet", d, parity_log)
    assert got[0] == float("inf"), got[0]                   # log of an underflowed softmax, as loss.py:339 gives
    assert np.isfinite(got[1][0]).all()
    check("listnet spread60 d score (closed form, finite where autograd is NaN)", L.grad_error(got[1][0], ref[1][0]), bound)


# ------------------------------------------------------------------------------------------------ case 4
def test_case_4_ranknet_with_one_overflowing_pair():
    scope, s, t = L.ranknet_overflow_case()
    tt = torch.tensor(np.array(t))
    ts = torch.tensor(np.array(s)).double().requires_grad_(True)
    ref_sum, pairs = O.ranknet_sum_session(ts, scope, tt.double(), 1.0)
    ref_g, = torch.autograd.grad(ref_sum, ts)
    ref_lam = O.ranknet_lambda(ts.detach(), scope, tt.double(), 1.0).numpy()
    lam32 = O.ranknet_lambda(torch.tensor(np.array(s)), scope, tt, 1.0).double().numpy()
    e32 = L.grad_error(lam32, ref_lam)
    bound = L.rule(e32)
    Hh.record("ranknet overflow: float32 CPU lambda, sets the bound beside it", e32, bound)
    x = dev(s, True)
    ls, n = RL.ranknet_loss(x, scope, tt, 1.0, 0)
    assert float(ls.detach()) == float("inf") and int(n) == pairs == 70 * 69
    ls.backward()
    lam = RL.ranknet_lambda(dev(s), scope, tt, 1.0, 0)
    assert bool(torch.isfinite(lam).all()) and bool(torch.isfinite(x.grad).all())
    check("ranknet overflow lambda", L.grad_error(host(lam), ref_lam), bound)
    check("ranknet overflow backward", L.grad_error(host(x.grad), ref_g.numpy()), bound)


# ------------------------------------------------------------------------------------------------ case 5
@pytest.mark.parametrize("kind", L.FACTORISED)
def test_case_5_factorised_kernels_stay_finite_under_var_over(kind):
    pair_form = L.evaluate(kind, L.inputs("var_over"), torch.float32)
    assert not L.is_finite(pair_form)                       # the claimed territory: the reference's float32 pair form is not
    ref = L.reference(kind, "var_over")
    e32, bound = L.yardstick(kind, "var_over")
    got = run(kind, L.inputs("var_over"))
    assert np.isfinite(got[0]) and all(np.isfinite(g).all() for g in got[1])
    for label, err in zip(L.labels(kind), L.errors(kind, got, ref)):
        check(f"{kind} var_over {label}", err, bound)


@pytest.mark.parametrize("regime", ["raw_targets", "far_targets"])
def test_exp_mse_with_raw_targets_has_the_float32_pattern(regime):
    """(exp(t) - exp(o))^2 leaves float32 where t > 44.4: the loss is +inf as in the float32 evaluation on the CPU; with
    raw_targets every exp(t) is finite and so is every gradient entry, within the bound of float64; with far_targets exp(t)
    is inf and every entry -inf"""
    ref, oracle = L.reference("exp_mse", regime), L.float32_run("exp_mse", regime)
    got = run("exp_mse", L.inputs(regime))
    assert got[0] == oracle[0] == float("inf")
    assert np.array_equal(np.isfinite(got[1][0]), np.isfinite(oracle[1][0]))
    if regime == "raw_targets":
        e32 = L.grad_error(oracle[1][0], ref[1][0])
        Hh.record("exp_mse raw_targets: float32 CPU gradient, sets the bound beside it", e32, L.rule(e32))
        check("exp_mse raw_targets d score", L.grad_error(got[1][0], ref[1][0]), L.rule(e32))
    else:
        assert np.all(got[1][0] == -np.inf) and np.all(oracle[1][0] == -np.inf)


# ------------------------------------------------------------------------------------------------ case 6
def test_case_6_kl_of_a_query_with_a_score_above_104_is_nan_and_the_rest_is_untouched():
    from reactranker_amd import eval as RE
    s, t = L.kl_case(), L.base()["targets"]
    off = np.concatenate([[0], np.cumsum(SCOPE)])
    _, _, rows = O.calculate_ndcg_from_scores([np.array(s[a:b]) for a, b in zip(off[:-1], off[1:])],
                                              [np.array(t[a:b]) for a, b in zip(off[:-1], off[1:])], 0.5)
    stats, _ = RE.ranking_stats(dev(s), SCOPE, np.array(t), 0, 0.25, 0.5)
    stats = stats.cpu().numpy()
    others = np.arange(len(SCOPE)) != L.KL_QUERY
    assert np.isnan(stats[L.KL_QUERY, 10]) and np.isnan(rows[L.KL_QUERY, 1])
    assert np.allclose(stats[others, 10], rows[others, 1], rtol=1e-6, atol=1e-6)      # test_gpu_losses.py's bounds
    assert np.allclose(stats[:, 9], rows[:, 0], rtol=0, atol=1e-6)
    assert np.isfinite(stats[:, 9]).all() and np.isfinite(stats[L.KL_QUERY, :10]).all()       # every NDCG of that query too
    plain, _ = RE.ranking_stats(dev(L.base()["score"]), SCOPE, np.array(t), 0, 0.25, 0.5)
    assert np.array_equal(stats[others], plain.cpu().numpy()[others], equal_nan=True)           # the other queries: the same bits


# ------------------------------------------------------------------------------------------------ case 7
@pytest.mark.parametrize("head,n", L.HEADS)
def test_case_7_heads_at_saturating_inputs(head, n):
    """rr_head_fwd_f32 / rr_head_bwd_f32 at raw = +-50 and +-110 against float64 softplus and sigmoid: finite; an activated
    column is exactly its floor at -110 (softplus there is 1.7e-48) and exactly raw (+ floor) at +50 and +110 in float32; the
    gradient factor is exactly 0 at -110 and exactly 1 at +50 and +110 (1 - sigmoid is below half an ulp of 1)."""
    raw = np.tile(np.asarray(L.HEAD_RAWS, np.float32)[:, None], (1, n))
    out_ref, slope_ref, col_in, act = L.head_reference(raw, head)
    out = Fn.head_fwd(dev(raw), head)
    assert bool(torch.isfinite(out).all())
    got = out.double().cpu().numpy()
    err = float(np.max(np.abs(got - out_ref) / (1 + np.abs(out_ref))))
    check(f"head {head} x {n} forward", err, L.BOUND)
    go = np.random.default_rng(L.SEED + head + n).standard_normal(raw.shape).astype(np.float32)
    draw = Fn.head_bwd(dev(go), dev(raw), head)
    assert bool(torch.isfinite(draw).all())
    want = np.empty_like(out_ref)
    want[:, col_in] = go.astype(np.float64) * slope_ref
    g = draw.double().cpu().numpy()
    check(f"head {head} x {n} backward", float(np.max(np.abs(g - want) / (1 + np.abs(want)))), L.BOUND)
    G = len(act)
    for c in range(n):
        if not act[c % G]:
            continue
        floor = np.float32(out_ref[3, c])                   # softplus(-110) + floor rounds to the floor itself
        assert out[3, c].item() == float(floor) and floor in (np.float32(0), np.float32(1e-6), np.float32(1.0), np.float32(1e-6) + np.float32(1.0))
        assert out[2, c].item() == float(np.float32(110.0) + floor) and out[0, c].item() == float(np.float32(50.0) + floor)
        ci = col_in[c]
        assert draw[3, ci].item() == 0.0 and draw[2, ci].item() == float(go[2, c]) and draw[0, ci].item() == float(go[0, c])
