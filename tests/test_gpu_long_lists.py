"""Every per-list loss at the lengths where its launch changes: up to kMaxLen = 8192 candidates (csrc/wave_util.h), against
float64.

What changes above the 300 - 2000 candidates of the other loss tests: a launch that stages more than 64 KiB of LDS has to opt
in per kernel and per template instantiation (set_lds: above 3276 candidates at 20 bytes each, 4096 at 16, 5461 at 12);
every lane's sequential share of a scan or a pair count grows with C; and the per-element forms of csrc/loss_list.h stand in
for C x C pair sums that have only been compared with the reference's form up to C = 300.

Windows.  CAP = [8192].  MIXED = [3277, 64, 5462, 0, 4097, 1]: one launch with array pitch 5462 and shorter lists in it, an
empty and a one-candidate query beside long ones.  A launch's LDS is sized by the window's longest list, so every MIXED
launch stages 5462 candidates: past the thresholds of the 20- and 16-byte kernels, and the first length of the 12-byte ones.
The 20- and 16-byte thresholds themselves (3277, 4097) are the launch size only in the opt-in test's one-list windows.  BETA = [5462, 3] for the two
C x C double-precision kernels (the first length that needs their opt-in; they evaluate six lgamma per pair on one wave).
Inputs as in tests/test_gpu_losses.py::test_losses_against_oracle_random: scores N(0, 2^2), targets a standardised
permutation per query (no ties), variances softplus + 1e-6, fixed seeds.

Measure.  Loss: |loss - ref| / |ref|.  Gradient: max |g - ref| / max |ref| per input column over the window - scaled to the
column's largest entry, because 1e-5 * (1 + |ref|) is an absolute 1e-5 for entries that are ~1e-5 themselves once divided by
C * Q (an all-zero ListNet gradient passes it at 8192).  The reference is float64 throughout: oracle/ref_cpu.py on .double()
tensors for the core losses, tests/listwise_variants_ref.py and tests/pairwise_variants_ref.py (the reference's own pair-sum
forms, row-blocked) for the rest.  A query without candidates adds zero and counts in Q (the kernels' rule; the reference's
mean of nothing is NaN), so the oracle is evaluated on the non-empty queries and rescaled by their share of Q.

Bound.  1e-5, the project's parity bound.  For the four core losses the float32 CPU oracle stays within 1.4e-7 (loss) and
3.4e-7 (gradient) of the float64 one on these windows, which leaves ~30x for the device's expf / logf and summation order.
For the variants and the Beta losses the module measures the same number itself (f32_error: the restatement in float32 on
the CPU against its float64 run): at most 1.25e-6 gives the bound 1e-5, more gives 8x that error (4 for summation order, 2
for the device's transcendentals) - never anything derived from the kernel.  Measured on the CPU for the windows below:
  mledis 1.2e-7, listnet_gauss 1.2e-7, listnet_lognorm 2.2e-7, listnet_evidential 6.2e-7, listnet_uq 1.5e-7,
  dirichlet_uq 3.0e-7 (the larger of CAP and MIXED, loss and gradients): bound 1e-5 for all six;
  beta_evidential 5.7e-7 on BETA: bound 1e-5;  betanet 8.3e-6 on BETA (its lt - lp adds six terms of magnitude up to
  lgamma(100) = 359, each rounded to float32), which by the rule would give 6.6e-5.  The two Beta kernels compute in double
  precision, though, so float32 rounding of the formula says nothing about them: they are held to 1e-5 whatever the rule
  allows, and the float32 figure is logged for information.

The LDS opt-in.  The HIP runtime that this was written against launches a kernel with more than 64 KiB of dynamic LDS
whether or not it opted in, so a kernel or template instantiation without the opt-in passes every comparison above; a runtime
that enforces it would reject the launch, and every test here that launches the kernel would fail with that status.  Until
then the library counts its opt-ins (rr_lds_opt_ins) and test_every_launch_above_64_KiB_opts_in reads the count around each
family's forward and backward, on MIXED / BETA and at the first length that needs it and the last that does not.

RankNet's pair count is compared exactly: with the oracle's, and with sum C (C - 1) - the targets have no ties - which is
67,100,672 for CAP."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import listwise_variants_ref as LV
from tests import pairwise_variants_ref as PV

from oracle import ref_cpu as O
from reactranker_amd import _lib
from reactranker_amd import loss as RL
from reactranker_amd import train_listwise as TL

pytestmark = pytest.mark.gpu
BOUND = 1e-5
WINDOWS = {"cap": [8192], "mixed": [3277, 64, 5462, 0, 4097, 1], "beta": [5462, 3],
           "at20": [3277], "below20": [3276], "at16": [4097], "below16": [4096], "below12": [5461]}   # the opt-in test's
SEEDS = {"cap": 31, "mixed": 32, "beta": 33, "at20": 34, "below20": 35, "at16": 36, "below16": 37, "below12": 38}
UQ_COEF = 0.5 * (2 / 4) ** 3                # annealing_coef(0.5, 2, 5)
BETA_PARAM = {"betanet": 100.0, "beta_evidential": 0.01}


def _softplus(x):
    return np.log1p(np.exp(x))


@functools.lru_cache(maxsize=None)
def inputs(win):
    """read-only float32 columns of a window: score, targets, var (drawn in test_losses_against_oracle_random's order), then
    the positive columns the variants need, as tools/make_golden_loss_variants.py draws them"""
    scope = WINDOWS[win]
    rng = np.random.default_rng(SEEDS[win])
    m = sum(scope)
    d = dict(score=(rng.standard_normal(m) * 2).astype(np.float32))
    t = np.concatenate([rng.permutation(c) for c in scope]).astype(np.float32)
    d["targets"] = ((t - t.mean()) / (t.std() + 1e-6)).astype(np.float32)
    d["var"] = (_softplus(rng.standard_normal(m)) + 1e-6).astype(np.float32)
    d["pos"] = (_softplus(rng.standard_normal(m)) + 0.1).astype(np.float32)
    d["conc"] = (_softplus(rng.standard_normal(m)) + 1.0 + 1e-6).astype(np.float32)
    d["nu"] = (_softplus(rng.standard_normal(m)) + 1e-6).astype(np.float32)
    d["alpha"] = (_softplus(rng.standard_normal(m)) + 1.0 + 1e-6).astype(np.float32)
    for a in d.values():
        a.setflags(write=False)
    return d


def dev(a, grad=False):
    return torch.tensor(np.array(a)).cuda().requires_grad_(grad)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def loss_error(got, ref):
    got = float(got.detach().double().sum()) if torch.is_tensor(got) else float(got)
    return abs(got - ref) / abs(ref)


def grad_error(got, ref):
    g = got.detach().double().cpu().numpy().reshape(-1) if torch.is_tensor(got) else np.asarray(got, np.float64).reshape(-1)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    return float(np.max(np.abs(g - ref)) / np.max(np.abs(ref)))          # (a NaN anywhere makes this NaN, which fails)


def check(what, err, bound=BOUND):
    Hh.record(what, err, bound)
    print(f"[long lists] {what}: err {err:.3e} (bound {bound:g})")
    assert err <= bound, f"{what}: err {err:.3e} > {bound:g}"


# ------------------------------------------------------------------------------------------------ float64 references, cached
CORE = ("mle", "listnet", "evid", "ranknet")


@functools.lru_cache(maxsize=None)
def core_reference(kind, win):
    """(loss, [gradient per input column]) of a core loss from the float64 oracle; for 'ranknet' the loss is loss_sum / pairs
    and a third entry holds (pairs, accelerate_grad's lambdas / pairs)"""
    scope, d = WINDOWS[win], inputs(win)
    live = [c for c in scope if c > 0]                                     # (no query is empty in the middle of a list)
    share = len(live) / len(scope)
    ts = torch.tensor(np.array(d["score"])).double().requires_grad_(True)
    tv = torch.tensor(np.array(d["var"])).double().requires_grad_(True)
    tt = torch.tensor(np.array(d["targets"])).double()
    if kind == "mle":
        ref = O.listmle_loss(ts, live, tt).sum() * share
        g, = torch.autograd.grad(ref, ts)
        out = float(ref.detach()), frozen(g.numpy())
    elif kind == "listnet":
        ref = O.listnet_loss(ts, live, tt)                                 # ONE mean over all candidates: no share
        g, = torch.autograd.grad(ref, ts)
        out = float(ref.detach()), frozen(g.numpy())
    elif kind == "evid":
        ref = O.evidential_ranking_loss(torch.stack([ts, tv], 1), live, tt).sum() * share
        gs, gv = torch.autograd.grad(ref, [ts, tv])
        out = float(ref.detach()), frozen(gs.numpy(), gv.numpy())
    else:
        ref, pairs = O.ranknet_sum_session(ts, live, tt, 1.0)
        g, = torch.autograd.grad(ref / pairs, ts)
        with torch.no_grad():
            lam = O.ranknet_lambda(ts.detach(), live, tt, 1.0) / pairs
        out = float(ref.detach()) / pairs, frozen(g.numpy()), (int(pairs), frozen(lam.numpy())[0])
    assert np.isfinite(out[0]) and all(np.isfinite(g).all() for g in out[1]), (kind, win)
    return out


VARIANTS = {      # kind -> (the module of reactranker_amd.loss, its input columns)
    "mledis": (RL.MLEDisLoss, ("score", "var")),
    "listnet_gauss": (RL.Listnet_For_Gauss, ("score", "var")),
    "listnet_lognorm": (RL.Listnetlognorm, ("pos", "var")),
    "listnet_evidential": (RL.Listnet_For_evidential, ("score", "nu", "alpha")),
    "listnet_uq": (RL.Listnet_with_uq, ("pos",)),
    "dirichlet_uq": (RL.Dirichlet_uq, ("conc",)),
}


@functools.lru_cache(maxsize=None)
def variant_reference(kind, win, dtype=torch.float64):
    d = inputs(win)
    loss, grads = LV.variant_loss(kind, [d[c] for c in VARIANTS[kind][1]], WINDOWS[win], d["targets"], UQ_COEF, dtype=dtype)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads), (kind, win, dtype)
    return loss, frozen(*grads)


@functools.lru_cache(maxsize=None)
def beta_reference(kind, dtype=torch.float64):
    d = inputs("beta")
    x = d["score"] if kind == "betanet" else d["pos"]
    loss, pairs, g = PV.sq_loss(kind, x, WINDOWS["beta"], d["targets"], BETA_PARAM[kind], dtype=dtype, block=512)
    assert np.isfinite(loss) and np.isfinite(g).all(), (kind, dtype)
    return loss, pairs, frozen(g)[0]


def f32_error(what, ref64, ref32):
    """the restatement's own float32 error under the module's measure, and the bound it gives (module docstring); logged
    next to that bound"""
    e = max([abs(ref32[0] - ref64[0]) / abs(ref64[0])] + [grad_error(a, b) for a, b in zip(ref32[1], ref64[1])])
    bound = BOUND if e <= 1.25e-6 else 8 * e
    Hh.record(f"{what}: float32 CPU restatement, sets the bound beside it", e, bound)
    print(f"[long lists] {what}: float32 CPU error {e:.3e} -> bound {bound:g}")
    return e, bound


# ------------------------------------------------------------------------------------------------ 1. the core losses
def run_core(kind, win, fused=True, how="plain", strided=False):
    """(loss, [gradient columns], pairs or None) through the autograd entry points"""
    scope, d = WINDOWS[win], inputs(win)
    tt = torch.tensor(np.array(d["targets"]))
    old = RL.FusedStep.enabled
    RL.FusedStep.enabled = fused
    try:
        pairs = None
        if kind == "evid":
            x = torch.stack([dev(d["score"]), dev(d["var"])], 1).requires_grad_(True)
            l = RL.evidential_ranking()(x, scope, tt, None, None, None, 0)
        else:
            if strided:                                                    # column 0 of an [m, 2] tensor, read in place
                x = torch.stack([dev(d["score"]), dev(d["var"])], 1).requires_grad_(True)
                col = x[:, 0]
                assert col.stride(0) == 2
            else:
                x = col = dev(d["score"], True)
            if kind == "ranknet":
                ls, pairs = RL.ranknet_loss(col, scope, tt, 1.0, 0)
                l = ls / pairs
            else:
                l = (RL.MLEloss() if kind == "mle" else RL.ListnetLoss())(col, scope, tt, 0)
        if how == "unit":
            RL.backward(l)
        else:
            l.sum().backward()
        g = x.grad
        cols = [g[:, 0], g[:, 1]] if g.dim() == 2 else [g]
        if strided:
            assert float(cols[1].abs().max()) == 0.0                       # the column the loss does not read
            cols = cols[:1]
        return l.detach().clone(), [c.contiguous() for c in cols], (None if pairs is None else int(pairs))
    finally:
        RL.FusedStep.enabled = old


@pytest.mark.parametrize("win", ["cap", "mixed"])
@pytest.mark.parametrize("kind", CORE)
def test_core_losses_against_the_float64_oracle(kind, win):
    ref = core_reference(kind, win)
    l, gs, pairs = run_core(kind, win)
    if kind == "ranknet":
        assert pairs == ref[2][0], (pairs, ref[2][0])                      # exactly
        assert pairs == sum(c * c - c for c in WINDOWS[win]) and (win != "cap" or pairs == 67_100_672)     # no ties
    check(f"{kind} {win} loss", loss_error(l, ref[0]))
    for name, g, r in zip(("d score", "d var"), gs, ref[1]):
        check(f"{kind} {win} {name}", grad_error(g, r))
    if kind == "ranknet":                                                  # accelerate_grad's closed-form lambdas
        d = inputs(win)
        lam = RL.ranknet_lambda(dev(d["score"]), WINDOWS[win], torch.tensor(np.array(d["targets"])), 1.0, 0) / pairs
        check(f"ranknet_lambda {win}", grad_error(lam, ref[2][1]))


def test_logcumsumexp_op_at_8192():
    """LogCumsumExp.apply on 8192 values (128 sequential float32 additions per lane, 64 KiB of LDS) against the float64
    torch.logcumsumexp of the flipped vector; gradient of sum(y) from autograd (for an upstream gradient of ones the
    reference's backward formula is the true gradient).  Both are vectors: max |. - ref| / max |ref|."""
    x = dev(inputs("cap")["score"], True)
    y = RL.LogCumsumExp.apply(x)
    y.sum().backward()
    xr = torch.tensor(np.array(inputs("cap")["score"])).double().requires_grad_(True)
    yr = torch.logcumsumexp(xr.flip(0), 0).flip(0)
    gr, = torch.autograd.grad(yr.sum(), xr)
    check("logcumsumexp 8192 value", grad_error(y, yr.detach().numpy()))
    check("logcumsumexp 8192 gradient", grad_error(x.grad, gr.numpy()))


@pytest.mark.parametrize("win", ["cap", "mixed"])
@pytest.mark.parametrize("kind", ["mle", "listnet", "evid"])
def test_fused_step_has_the_bits_of_the_two_kernel_path_on_long_lists(kind, win, parity_log):
    """the contract of test_fused_loss_step_has_the_bits_of_the_two_kernel_path where both paths need the LDS opt-in: the
    step kernel (mode 2) against forward kernel + reduction + backward kernel, and the step twice in a row (the ticket word
    re-arms)"""
    l0, g0, _ = run_core(kind, win, fused=False, how="unit")
    for launch in range(2):
        hits = RL.FusedStep.hits
        l1, g1, _ = run_core(kind, win, fused=True, how="unit")
        assert RL.FusedStep.hits == hits + 1
        assert torch.equal(l0, l1), (kind, win, launch, float(l0.sum()), float(l1.sum()))
        for a, b in zip(g0, g1):
            assert torch.equal(a, b), (kind, win, launch, float((a - b).abs().max()))
    ref = core_reference(kind, win)                                         # and the handed-out gradient is the right one
    check(f"{kind} {win} step loss", loss_error(l1, ref[0]))
    for name, g, r in zip(("d score", "d var"), g1, ref[1]):
        check(f"{kind} {win} step {name}", grad_error(g, r))
    parity_log(f"{kind} on {win}: fused step == two-kernel path bit for bit, two launches")


@pytest.mark.parametrize("kind", ["mle", "listnet", "ranknet"])
def test_strided_score_column_gives_the_bits_of_the_contiguous_call(kind):
    la, ga, pa = run_core(kind, "mixed", strided=True)
    lb, gb, pb = run_core(kind, "mixed")
    assert torch.equal(la, lb) and torch.equal(ga[0], gb[0]) and pa == pb


@pytest.mark.parametrize("kind", ["listmle", "listnet", "evidential_ranking", "ranknet"])
def test_every_gradient_entry_is_written_on_long_lists(kind):
    """the C entry points write into buffers preset to NaN - step and backward forms, on MIXED (lists shorter than the array
    pitch, an empty and a one-candidate query): every entry must come back finite and equal the float64 gradient"""
    from reactranker_amd._lib import lib, check as status, ptr, stream
    scope, d = WINDOWS["mixed"], inputs("mixed")
    Q, m = len(scope), sum(scope)
    cols = 2 if kind == "evidential_ranking" else 1
    x = torch.stack([dev(d["score"]), dev(d["var"])], 1) if cols == 2 else dev(d["score"])
    t = dev(d["targets"])
    seg, total, max_len = RL._segments(tuple(scope), str(x.device))
    one = torch.ones(1, device="cuda")
    nan = lambda: torch.full_like(x, float("nan"))                          # noqa: E731
    if kind == "ranknet":
        ref = core_reference("ranknet", "mixed")
        dd = nan()
        status(lib().rr_ranknet_bwd_f32(ptr(x), 1, ptr(t), ptr(seg), Q, max_len, 1.0, 0, ptr(one), ptr(dd), 1, stream()), kind)
        assert bool(torch.isfinite(dd).all())
        check("ranknet bwd into NaN", grad_error(dd / ref[2][0], ref[1][0]))
        return
    ref = core_reference({"listmle": "mle", "listnet": "listnet", "evidential_ranking": "evid"}[kind], "mixed")
    ins = [ptr(x[:, 0]), ptr(x[:, 1]), x.stride(0)] if cols == 2 else [ptr(x), x.stride(0)]
    args = ins + [ptr(t), ptr(seg), Q, max_len] + ([total] if kind == "listnet" else [])
    for form in ("step", "bwd"):
        dd = nan()
        outs = [ptr(dd[:, 0]), ptr(dd[:, 1]), 2] if cols == 2 else [ptr(dd), 1]
        if form == "step":
            loss = torch.full((1,), float("nan"), device="cuda")
            part = torch.full((Q,), float("nan"), device="cuda")
            counter = torch.zeros(1, dtype=torch.int32, device="cuda")
            status(getattr(lib(), f"rr_{kind}_step_f32")(*args, ptr(loss), ptr(part), ptr(counter), *outs, stream()), kind)
            assert int(counter) == 0
            check(f"{kind} step loss", loss_error(loss, ref[0]))
        else:
            status(getattr(lib(), f"rr_{kind}_bwd_f32")(*args, ptr(one), *outs, stream()), kind)
        assert bool(torch.isfinite(dd).all()), (kind, form)
        for c, r in enumerate(ref[1]):
            check(f"{kind} {form} into NaN, column {c}", grad_error(dd[:, c] if cols == 2 else dd, r))


# ------------------------------------------------------------------------------------------------ 2. the six listwise variants
def run_variant(kind, win, cols=None):
    """(loss, gradients per input column) of a variant's own kernels on the window's columns, or on `cols` in their place"""
    cls, names = VARIANTS[kind]
    d = inputs(win)
    leaves = [dev(c, True) for c in (cols if cols is not None else [d[c] for c in names])]
    tt = torch.tensor(np.array(d["targets"]))
    if kind in ("listnet_uq", "dirichlet_uq"):
        l = cls()(leaves[0], WINDOWS[win], tt, 0.5, 2, 5, 0)
    else:
        l = cls()(*[x[:, None] for x in leaves], WINDOWS[win], tt, 0)
    gs = torch.autograd.grad(l.sum(), leaves)
    return l.detach(), gs


@pytest.mark.parametrize("win", ["cap", "mixed"])
@pytest.mark.parametrize("kind", list(VARIANTS))
def test_listwise_variants_against_their_pair_sum_restatements(kind, win):
    """each variant's forward and backward kernel against the reference's own (pair-sum) form in float64; the bound by the
    module's rule from the restatement's float32 CPU error - 1e-5 for all six (measured values: module docstring)"""
    ref = variant_reference(kind, win)
    _, bound = f32_error(f"{kind} {win}", ref, variant_reference(kind, win, torch.float32))
    l, gs = run_variant(kind, win)
    assert l.shape == (1,)
    check(f"{kind} {win} loss", loss_error(l, ref[0]), bound)
    for name, g, r in zip(VARIANTS[kind][1], gs, ref[1]):
        check(f"{kind} {win} d {name}", grad_error(g, r), bound)


# ------------------------------------------------------------------------------------------------ 3. the composite task step
TASKS = ["mledis_gaussian", "listnetdis_gauss", "listnet_uq", "dirichlet_uq", "mle_mse"]


def task_output(task):
    d = inputs("mixed")
    if task == "listnet_uq":
        return np.array(d["pos"])
    if task == "dirichlet_uq":
        return np.array(d["conc"])
    if task == "mle_mse":
        return np.array(d["score"])
    # mean and a second column >= 1: the Gaussian term divides by it, and below ~0.1 its gradient (d^2 / 2 v^2) would be 1e4
    # times the list term's, which the column's largest entry would then hide.  mledis_gaussian reads it as log(variance):
    # kept below ~2.1, since exp(s + variance / 2) with variances in the hundreds is out of float32's range on any machine
    if task == "mledis_gaussian":
        return np.stack([d["score"], np.float32(1.0) + np.float32(0.25) * d["var"]], 1)
    return np.stack([d["score"], d["var"] + np.float32(1.0)], 1)


LIST_TERM = {"mledis_gaussian": "mledis", "listnetdis_gauss": "listnet_gauss"}


@functools.lru_cache(maxsize=None)
def list_term_columns(task):
    """the float32 (mean, variance) columns that the list term of a two-column task type sees (train_listwise._loss_terms)"""
    o = task_output(task)
    return frozen(o[:, 0].copy(), np.exp(o[:, 1]).astype(np.float32) if task == "mledis_gaussian" else o[:, 1].copy())


@functools.lru_cache(maxsize=None)
def list_term_reference(task, dtype=torch.float64):
    loss, grads = LV.variant_loss(LIST_TERM[task], list(list_term_columns(task)), WINDOWS["mixed"], inputs("mixed")["targets"],
                                  0.0, dtype=dtype)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads), (task, dtype)
    return loss, frozen(*grads)


def run_task(task, fused):
    """(loss, d loss / d output) of a composite task type on MIXED: the one-launch step (fused) or its terms' own kernels"""
    scope, d = WINDOWS["mixed"], inputs("mixed")
    o = dev(task_output(task), True)
    tt = torch.tensor(np.array(d["targets"]))
    if task == "mle_mse" and fused:                                        # the entry point itself, terms chosen by hand
        o2 = o.detach().reshape(-1, 1)
        seg, total, max_len = RL._segments(tuple(scope), str(o.device))
        dout = torch.full_like(o2, float("nan"))
        l = RL.task_loss_step(_lib.RR_LIST_MLE, _lib.RR_POINT_MSE, o2, dev(d["targets"]), seg, len(scope), max_len, 0.0,
                              len(scope), total, dout)
        return l.detach(), dout.reshape(-1)
    old = RL.FusedStep.enabled
    RL.FusedStep.enabled = fused
    try:
        hits = RL.FusedStep.hits
        if task == "mle_mse":
            l = RL.MLEloss()(o, scope, tt, 0) + RL.MSELoss()(o, tt)
        else:
            l = TL.batch_loss(task, o, scope, tt, 0, 2, 5, 0.5)
        RL.backward(l) if fused else l.sum().backward()
        assert RL.FusedStep.hits == hits + (1 if fused else 0), "the step entry was not taken" if fused else "a fused launch"
        return l.detach(), o.grad
    finally:
        RL.FusedStep.enabled = old


@pytest.mark.parametrize("task", TASKS)
def test_task_step_against_its_standalone_kernels_on_long_lists(task):
    """rr_task_loss_step_f32 (task_step_kernel<LT, PT>: its own LDS opt-in per pair of terms) against the sum of the
    standalone kernels that the tests above hold to float64, under the module's measure per output column; and against
    itself over two launches, bit for bit.  The variant tests run on other second columns than the two-column task types
    here, so the standalone list term is also held to its float64 restatement on this test's own columns (float32 CPU error
    4.5e-8 for mledis, 1.2e-7 for listnet_gauss: bound 1e-5), which ties the step to float64 through it."""
    lp, gp = run_task(task, False)
    l1, g1 = run_task(task, True)
    l2, g2 = run_task(task, True)
    assert torch.equal(l1, l2) and torch.equal(g1, g2), "two launches differ"
    assert bool(torch.isfinite(g1).all())
    check(f"{task} step loss", loss_error(l1, float(lp.double().sum())))
    g1c, gpc = g1.reshape(g1.shape[0], -1), gp.reshape(gp.shape[0], -1)
    for c in range(g1c.shape[1]):
        check(f"{task} step d out[:, {c}]", grad_error(g1c[:, c], gpc[:, c].double().cpu().numpy()))
    if task in ("listnet_uq", "dirichlet_uq"):      # one term on the variant test's own inputs: the float64 restatement itself
        ref = variant_reference(task, "mixed")
        check(f"{task} step loss against float64", loss_error(l1, ref[0]))
        check(f"{task} step d out against float64", grad_error(g1, ref[1][0]))
    if task in LIST_TERM:
        ref = list_term_reference(task)
        _, bound = f32_error(f"{task} list term", ref, list_term_reference(task, torch.float32))
        l, gs = run_variant(LIST_TERM[task], "mixed", list_term_columns(task))
        check(f"{task} standalone list term loss", loss_error(l, ref[0]), bound)
        for name, g, r in zip(("mean", "variance"), gs, ref[1]):
            check(f"{task} standalone list term d {name}", grad_error(g, r), bound)


# ------------------------------------------------------------------------------------------------ 4. Beta losses, pairwise evaluation
def run_beta(kind):
    scope, d = WINDOWS["beta"], inputs("beta")
    x = dev(d["score"] if kind == "betanet" else d["pos"], True)
    fn = RL.betanet_loss if kind == "betanet" else RL.beta_evidential_loss
    loss_sum, pairs = fn(x, scope, torch.tensor(np.array(d["targets"])), BETA_PARAM[kind], 0)
    loss_sum.backward()
    return loss_sum.detach(), int(pairs), x.grad


@pytest.mark.parametrize("kind", ["betanet", "beta_evidential"])
def test_beta_losses_at_the_first_length_that_needs_the_opt_in(kind):
    """betanet_loss / beta_evidential_loss on [5462, 3] (12 bytes per candidate: 65,544 bytes of LDS) against the row-blocked
    float64 restatement.  The module's rule gives 1e-5 for beta_evidential (float32 CPU error 5.7e-7) and 8 x 8.3e-6 =
    6.6e-5 for betanet; both kernels compute in double precision and are held to 1e-5 (module docstring)"""
    scope = WINDOWS["beta"]
    ref_loss, ref_pairs, ref_g = beta_reference(kind)
    r32 = beta_reference(kind, torch.float32)
    _, rule = f32_error(f"{kind} beta", (ref_loss, [ref_g]), (r32[0], [r32[2]]))
    bound = min(rule, BOUND)                                               # a double-precision kernel: module docstring
    loss_sum, pairs, g = run_beta(kind)
    assert pairs == ref_pairs == RL.sq_pairs(scope)
    check(f"{kind} beta loss", loss_error(loss_sum, ref_loss), bound)
    check(f"{kind} beta d score", grad_error(g, ref_g), bound)


def test_pairwise_evaluation_at_8192():
    from reactranker_amd import eval as RE
    d = inputs("cap")
    sums, per_query = RE.pairwise_stats_from_scores(dev(d["score"]), WINDOWS["cap"], torch.tensor(np.array(d["targets"])), 1.0, 0)
    acc, ce, rows = PV.pairwise_stats(d["score"], WINDOWS["cap"], d["targets"], 1.0, block=1024)
    sums, per_query = sums.cpu().numpy(), per_query.cpu().numpy()
    assert np.array_equal(per_query[:, :2], rows[:, :2]), (per_query[:, :2], rows[:, :2])     # pair counts, mismatches: exactly
    assert sums[1] == 1.0 and sums[3] == 2 * rows[0, 0] == 67_100_672
    check("pairwise_acc 8192", abs(sums[0] / sums[1] - acc) / acc)
    check("eval_cross_entropy_loss 8192", abs(sums[2] / sums[3] - ce) / ce)


# ------------------------------------------------------------------------------------------------ 5. the LDS opt-in itself
def forward_only(kind, win):
    """the loss of `kind` on a window, its inputs wanting a gradient, nothing back-propagated yet"""
    scope, d = WINDOWS[win], inputs(win)
    tt = torch.tensor(np.array(d["targets"]))
    if kind == "mle":
        return RL.MLEloss()(dev(d["score"], True), scope, tt, 0)
    if kind == "evid":
        x = torch.stack([dev(d["score"]), dev(d["var"])], 1).requires_grad_(True)
        return RL.evidential_ranking()(x, scope, tt, None, None, None, 0)
    if kind == "ranknet":
        return RL.ranknet_loss(dev(d["score"], True), scope, tt, 1.0, 0)[0]
    if kind in BETA_PARAM:
        fn = RL.betanet_loss if kind == "betanet" else RL.beta_evidential_loss
        return fn(dev(d["score"] if kind == "betanet" else d["pos"], True), scope, tt, BETA_PARAM[kind], 0)[0]
    cls, names = VARIANTS[kind]
    return cls()(*[dev(d[c], True)[:, None] for c in names], scope, tt, 0)


# case -> (loss, window, fused step, opt-ins of its forward launches, of its backward launches).  A launch stages
# bytes per candidate x the window's longest list and opts in above 65,536 bytes (csrc/wave_util.h: set_lds, once per launch);
# forward and backward are counted apart, so neither kernel can stand in for the other.
OPT_IN = {
    "mle": ("mle", "mixed", False, 1, 1),                                  # 20 bytes: list_loss_kernel<kListMle> forward, backward
    "mle step": ("mle", "mixed", True, 1, 0),                              # ... and its one-launch form
    "mle 3277": ("mle", "at20", False, 1, 1),                              # 65,540 bytes: the first length of 20 bytes
    "mle 3276": ("mle", "below20", False, 0, 0),                           # 65,520
    "evid": ("evid", "mixed", False, 1, 1),                                # <kUcListwise>: 12 bytes x 5462 = 65,544: the first length
    "evid step": ("evid", "mixed", True, 1, 0),
    "evid 5461": ("evid", "below12", False, 0, 0),                         # 65,532
    "ranknet": ("ranknet", "mixed", False, 0, 1),                          # 8 bytes forward, 12 backward
    "mledis": ("mledis", "mixed", False, 1, 1),                            # list_loss_kernel<K> of the variants: 20,
    "listnet_gauss": ("listnet_gauss", "mixed", False, 1, 1),              # 12,
    "listnet_lognorm": ("listnet_lognorm", "mixed", False, 1, 1),          # 12,
    "listnet_evidential": ("listnet_evidential", "mixed", False, 1, 1),    # 16 bytes
    "listnet_evidential 4097": ("listnet_evidential", "at16", False, 1, 1),       # 65,552 bytes: the first length of 16 bytes
    "listnet_evidential 4096": ("listnet_evidential", "below16", False, 0, 0),    # 65,536
    "betanet": ("betanet", "beta", False, 1, 1),                           # 12 bytes: betanet_fwd_kernel, betanet_bwd_kernel
    "beta_evidential": ("beta_evidential", "beta", False, 1, 1),           # beta_evi_kernel<false>, <true>
}


@pytest.mark.parametrize("case", list(OPT_IN))
def test_every_launch_above_64_KiB_opts_in(case):
    """the library's count of opt-ins (rr_lds_opt_ins) around the forward and around the backward of each kernel family: one
    per launch that stages more than 64 KiB, none one candidate below the threshold.  The values are the other tests'
    business (module docstring)."""
    kind, win, fused, in_forward, in_backward = OPT_IN[case]
    count = _lib.lib().rr_lds_opt_ins
    old = RL.FusedStep.enabled
    RL.FusedStep.enabled = fused
    try:
        n0 = count()
        loss = forward_only(kind, win)
        n1 = count()
        RL.backward(loss) if fused else loss.sum().backward()
        n2 = count()
    finally:
        RL.FusedStep.enabled = old
    torch.cuda.synchronize()
    assert (n1 - n0, n2 - n1) == (in_forward, in_backward), (case, n1 - n0, n2 - n1)


@pytest.mark.parametrize("task", ["mledis_gaussian", "listnetdis_gauss", "mle_mse"])       # 20, 12, 20 bytes per candidate
def test_task_step_launch_opts_in(task):
    """task_step_kernel<LT, PT> has an opt-in per pair of terms: the one launch of a step on MIXED makes one"""
    before = _lib.lib().rr_lds_opt_ins()
    run_task(task, True)
    torch.cuda.synchronize()
    assert _lib.lib().rr_lds_opt_ins() - before == 1, task
