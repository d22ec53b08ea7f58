"""Inputs, float64 references and float32 yardsticks of the value-range tests of the loss kernels
(tests/test_loss_range_cpu.py, tests/test_gpu_loss_range.py).  Nothing here touches the device or the library.

Window.  SCOPE = [1, 2, 7, 64, 65, 130, 300], 569 candidates, fixed seed.  Base inputs: score = 2 z with z ~ N(0, 1),
targets a z-scored permutation per query (no ties; the one-candidate query's target is 0), var = softplus(N(0, 1)) + 1e-6,
and the positive columns pos, conc, nu, alpha, beta as tests/test_gpu_long_lists.py draws them.

A regime (REGIMES) changes one thing about the base inputs.  The score regimes also hand their scores to `pos`, the
positive score column of Listnetlognorm, Lognorm, Listnet_with_uq and Beta-evidential: where those scores are not all
positive the float64 reference is NaN (log of a non-positive number) and the pair is skipped.  PAIRS is every kernel x
regime in which the kernel reads a column the regime changes.

Skipped pairs (SKIPPED; tests/test_loss_range_cpu.py holds that these, and only these, have a non-finite float64
reference):
  listnet_lognorm, listnet_uq, beta_evidential  x  spread8, tiny   (scores of both signs: log of a negative ratio or share)
  lognorm  x  down20, spread8, tiny                                 (log of a non-positive score)
down20 is NOT skipped for the first three: with every score negative the ratios s_j / s_i and shares s_i / sum(s) are
positive, and the kernels keep the sign as the reference does.

Two pairs have a finite float64 reference while plain float32 arithmetic leaves its range (F32_OVERFLOW): exp_mse x
raw_targets and far_targets, (exp(t) - exp(o))^2 with t = 45 + 12 z and 200 + 12 z.  The kernel is float32 and keeps the
reference's arithmetic, so these two are compared as the documented non-finite cases are: the finite / non-finite pattern of
the float32 CPU evaluation (raw_targets: loss +inf, every gradient entry finite; far_targets: loss +inf, every entry -inf),
every finite element within the bound of float64.

Measure (tests/test_gpu_long_lists.py's).  Loss: |loss - ref| / |ref|.  Gradient: max |g - ref| / max |ref| per input column.
soft_rank has no scalar: its ranks are measured as max |r - ref| / ref (ranks are >= 1).  A NaN anywhere fails.

Reference.  float64 throughout: oracle/ref_cpu.py on .double() tensors, tests/listwise_variants_ref.py (the reference's own
pair-sum forms), pairwise_variants_ref.py, lambdarank_ref.py, approx_ndcg_ref.py, loss_variants_ref.nig_cross; the pointwise
means and the NIG loss are written below from train/loss.py:144-184, 402-437 and train_listwise.py:274-279 for any dtype (the
float64 NIG cross form is held to loss_variants_ref.nig_cross).

Yardstick and bound.  The float32 CPU evaluation of the same restatement against its float64 run, under the same measure;
at or below 1.25e-6 the bound is 1e-5, above it 8 x the measured number (4 for summation order, 2 for the device's
transcendentals).  For MLEDisLoss, Listnet_For_Gauss and Listnetlognorm the reference's pair form is useless in float32
outside the base range (MLEDis' float32 gradient error is 1.6e-2 in var_wide, its loss inf in var_over), so their yardstick is
the reference's formula with every log-sum-exp taken by torch.logsumexp (stable_variant below: the textbook form, not the
kernels' factorisation), which agrees with listwise_variants_ref in float64 to 1e-12.  The two Beta kernels compute in double
and are held to 1e-5 whatever the rule allows.  Measured on the CPU with the seed below, largest of loss and gradient
columns per pair (tests/test_loss_range_cpu.py recomputes every figure, prints it, and fails if one exceeds what is
recorded here, so a change of seed or regime cannot loosen a bound unseen):
  every pair of PAIRS and every +-120 case not named below: at most 1.25e-6, bound 1e-5.  The largest per kernel: mle 4.3e-7
  (up20), listnet 1.4e-7, evid 3.2e-7, ranknet 1.5e-7, listnet_gauss 8.4e-7 (var_wide), listnet_evidential 1.9e-7,
  listnet_uq 2.6e-7, dirichlet_uq 1.6e-7, gauss_nll 1.2e-7, mse 8.9e-8, lognorm 2.0e-7, exp_mse 1.2e-7, lambdarank 1.2e-7 /
  9.1e-8 (k = 0 / 10), approx_ndcg 1.5e-7 / 9.1e-8, soft_rank 2.8e-8, beta_evidential 1.9e-7
  mledis x var_over 1.36e-6 (bound 1.1e-5);  listnet_lognorm x var_over 1.71e-6 (1.4e-5)
  nig x evidence_small 1.32e-6 (1.1e-5), x evidence_large 1.67e-6 (1.3e-5)
  nig_cross x tiny 1.00e-5 (8.0e-5: d nu of v (t - mu)^2 + 2 beta (1 + v) summed over 569 targets with mu ~ 1e-4),
  x evidence_small 1.74e-6 (1.4e-5), x evidence_large 2.70e-6 (2.2e-5)
  betanet (a double-precision kernel, bound 1e-5 whatever the figure): 7.2e-6 .. 1.0e-5 in the score regimes, 1.33e-6 in the
  target regimes, and 1.0 in up20, where float32's sigmoid(20 + z) is exactly 1 and the float32 gradient exactly 0.
"""
import functools
import math

import numpy as np
import torch

from oracle import ref_cpu as O
from tests import approx_ndcg_ref as AR
from tests import lambdarank_ref as LR
from tests import listwise_variants_ref as LV
from tests import pairwise_variants_ref as PV
from tests.loss_variants_ref import PI_F32

SCOPE = [1, 2, 7, 64, 65, 130, 300]
M = sum(SCOPE)
SEED = 41
BOUND = 1e-5
UQ_COEF = 0.5 * (2 / 4) ** 3                # annealing_coef(0.5, 2, 5)
BETA_PARAM = {"betanet": 100.0, "beta_evidential": 0.01}
NIG_LAM, NIG_EPS = 0.1, 1e-4
VAR_FLOOR = np.float32(math.log1p(math.exp(-20.0)) + 1e-6)
# float32 exp: overflow above 88.7, subnormal below -87.3, zero below -103.3; the hand-built cases keep every exp argument
# MARGIN away from all three
EXP_OVERFLOW, EXP_SUBNORMAL, EXP_ZERO, MARGIN = 88.7, -87.3, -103.3, 15.0


def _softplus(x):
    return np.log1p(np.exp(x))


def _f32(a):
    a = np.asarray(a, np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def base():
    """the base columns (float32, read-only) plus the float64 draws the regimes are built from: z, zt"""
    rng = np.random.default_rng(SEED)
    z = rng.standard_normal(M)
    zt = []
    for c in SCOPE:
        p = rng.permutation(c).astype(np.float64)
        zt.append((p - p.mean()) / (p.std() + 1e-6))
    zt = np.concatenate(zt)
    d = dict(z=z, zt=zt, score=_f32(2 * z), targets=_f32(zt))
    d["var"] = _f32(_softplus(rng.standard_normal(M)) + 1e-6)
    d["pos"] = _f32(_softplus(rng.standard_normal(M)) + 0.1)
    d["conc"] = _f32(_softplus(rng.standard_normal(M)) + 1.0 + 1e-6)
    d["nu"] = _f32(_softplus(rng.standard_normal(M)) + 1e-6)
    d["alpha"] = _f32(_softplus(rng.standard_normal(M)) + 1.0 + 1e-6)
    d["beta"] = _f32(_softplus(rng.standard_normal(M)) + 1e-6)
    z.setflags(write=False)
    zt.setflags(write=False)
    return d


def _score(f):
    return lambda b: dict(score=_f32(f(b["z"])), pos=_f32(f(b["z"])))


def _var_floor(b):
    v = np.array(b["var"])
    v[::2] = VAR_FLOOR
    return dict(var=_f32(v))


def _evidence(k):
    return lambda b: dict(pos=_f32(b["pos"] * np.float32(k)), conc=_f32(b["conc"] * np.float32(k)), nu=_f32(b["nu"] * np.float32(k)),
                          alpha=_f32(np.float32(1.0) + (b["alpha"] - np.float32(1.0)) * np.float32(k)))


REGIMES = {      # name -> the columns it replaces
    "up20": _score(lambda z: z + 20.0),
    "down20": _score(lambda z: z - 20.0),
    "spread8": _score(lambda z: 8.0 * z),
    "tiny": _score(lambda z: 1e-4 * z),
    "raw_targets": lambda b: dict(targets=_f32(12.0 * b["zt"] + 45.0)),
    "far_targets": lambda b: dict(targets=_f32(12.0 * b["zt"] + 200.0)),
    "var_floor": _var_floor,
    "var_wide": lambda b: dict(var=_f32(b["var"] * np.float32(20.0))),
    "var_over": lambda b: dict(var=_f32(b["var"] * np.float32(60.0))),
    "evidence_small": _evidence(1e-3),
    "evidence_large": _evidence(1e3),
}
CASE_REGIMES = {  # the inputs of the documented non-finite cases (not part of PAIRS)
    "base": lambda b: {},
    "up120": _score(lambda z: z + 120.0),
    "down120": _score(lambda z: z - 120.0),
    "spread60": _score(lambda z: 60.0 * z),
    "spread15": _score(lambda z: 15.0 * z),
}


@functools.lru_cache(maxsize=None)
def inputs(regime):
    b = base()
    d = {k: v for k, v in b.items() if k not in ("z", "zt")}
    d.update((REGIMES.get(regime) or CASE_REGIMES[regime])(b))
    return d


@functools.lru_cache(maxsize=None)
def changed(regime):
    return frozenset((REGIMES.get(regime) or CASE_REGIMES[regime])(base()))


# kernel -> (input columns with a gradient, does it read the targets)
KINDS = {
    "mle": (("score",), True), "listnet": (("score",), True), "evid": (("score", "var"), True), "ranknet": (("score",), True),
    "mledis": (("score", "var"), True), "listnet_gauss": (("score", "var"), True), "listnet_lognorm": (("pos", "var"), True),
    "listnet_evidential": (("score", "nu", "alpha"), True), "listnet_uq": (("pos",), True), "dirichlet_uq": (("conc",), True),
    "gauss_nll": (("score", "var"), True), "mse": (("score",), True), "lognorm": (("pos", "var"), True), "exp_mse": (("score",), True),
    "nig": (("score", "nu", "alpha", "beta"), True), "nig_cross": (("score", "nu", "alpha", "beta"), True),
    "lambdarank_k0": (("score",), True), "lambdarank_k10": (("score",), True),
    "approx_ndcg_k0": (("score",), True), "approx_ndcg_k10": (("score",), True), "soft_rank": (("score",), False),
    "betanet": (("score",), True), "beta_evidential": (("pos",), True),
}
CORE = ("mle", "listnet", "evid", "ranknet")
FACTORISED = ("mledis", "listnet_gauss", "listnet_lognorm")
DOUBLE_KERNELS = ("betanet", "beta_evidential")
STEP_KINDS = ("mle", "listnet", "evid", "lambdarank_k0", "lambdarank_k10", "approx_ndcg_k0", "approx_ndcg_k10")
# ranknet's second "gradient" is ranknet_lambda / pairs (accelerate_grad's closed form), soft_rank's value is its rank vector
GRAD_NAMES = {"ranknet": ("d score", "lambda")}


def reads(kind):
    cols, t = KINDS[kind]
    return set(cols) | ({"targets"} if t else set())


PAIRS = [(k, r) for k in KINDS for r in REGIMES if reads(k) & changed(r)]
SKIPPED = frozenset([(k, r) for k in ("listnet_lognorm", "lognorm", "listnet_uq", "beta_evidential") for r in ("spread8", "tiny")]
                    + [("lognorm", "down20")])
F32_OVERFLOW = frozenset({("exp_mse", "raw_targets"), ("exp_mse", "far_targets")})
FINITE_PAIRS = [p for p in PAIRS if p not in SKIPPED and p not in F32_OVERFLOW]


# ------------------------------------------------------------------------------------------------ restatements for any dtype
def stable_variant(kind, cols, scope, targets, dtype=torch.float64):
    """(loss, [gradients]) of MLEDisLoss / Listnet_For_Gauss / Listnetlognorm as train/loss.py:102-141, 233-314 write them,
    every log of a sum of exponentials taken by torch.logsumexp: for MLEDis each column j of the i >= j pair matrix of
    s_i - s_j + (v_i + v_j) / 2 (sorted by target), for the two ListNet forms each row of x_j - x_i + (y_i + y_j) / 2
    (lognorm: x = log(score)).  Mean over the list, then over the queries."""
    leaves = [torch.tensor(np.asarray(c, np.float32)).to(dtype).requires_grad_(True) for c in cols]
    t = torch.tensor(np.asarray(targets, np.float32)).to(dtype)
    total = torch.zeros((), dtype=dtype)
    lo = 0
    for c in scope:
        x, y, tq = leaves[0][lo:lo + c], leaves[1][lo:lo + c], t[lo:lo + c]
        lo += c
        if kind == "mledis":
            idx = torch.argsort(tq, descending=True, stable=True)
            ss, sv = x[idx], y[idx]
            pair = ss[:, None] - ss[None, :] + (sv[:, None] + sv[None, :]) / 2
            rows = torch.arange(c)
            pair = pair.masked_fill(rows[:, None] < rows[None, :], float("-inf"))
            total = total + torch.logsumexp(pair, 0).mean()
        else:
            if kind == "listnet_lognorm":                                  # x_j / x_i of scores of one sign; mixed signs: NaN
                x = torch.log(x * torch.sign(x[0]))
            pair = x[None, :] - x[:, None] + (y[None, :] + y[:, None]) / 2
            total = total + (torch.softmax(tq, 0) * torch.logsumexp(pair, 1)).mean()
    total = total / len(scope)
    gs = torch.autograd.grad(total, leaves)
    return float(total.detach()), [g.double().numpy() for g in gs]


def pointwise(kind, cols, targets, dtype=torch.float64):
    """(loss, [gradients]) of the pointwise means: GaussDisLoss (through the oracle), nn.MSELoss, Lognorm (train/loss.py:180-181)
    and the regression_exploss expression (train_listwise.py:274-279)"""
    leaves = [torch.tensor(np.asarray(c, np.float32)).to(dtype).requires_grad_(True) for c in cols]
    t = torch.tensor(np.asarray(targets, np.float32)).to(dtype)
    if kind == "mse":
        loss = O.mse_loss(leaves[0], t)
    elif kind == "gauss_nll":
        loss = O.gauss_nll_loss(leaves[0], leaves[1], t)
    elif kind == "lognorm":
        s, v = leaves
        loss = torch.mean(0.5 * math.log(2 * PI_F32) + 0.5 * torch.log(v * (s ** 2)) + torch.pow(torch.log(s) - t, 2) / (2 * v))
    else:
        loss = torch.mean((torch.exp(t) - torch.exp(leaves[0])) ** 2)
    gs = torch.autograd.grad(loss.sum(), leaves)
    return float(loss.detach().sum()), [g.double().numpy() for g in gs]


def nig(cols, targets, cross, dtype=torch.float64):
    """evidential_loss_new (train/loss.py:402-437): parameters [M] against targets [M], or - cross - [M, 1] against [M], the
    M x M grid the trainer's broadcast makes; pi = float32(np.pi) as the kernels have it"""
    leaves = [torch.tensor(np.asarray(c, np.float32)).to(dtype).requires_grad_(True) for c in cols]
    t = torch.tensor(np.asarray(targets, np.float32)).to(dtype)
    mu, v, a, b = [x[:, None] for x in leaves] if cross else leaves
    om = 2 * b * (1 + v)
    nll = 0.5 * torch.log(PI_F32 / v) - a * torch.log(om) + (a + 0.5) * torch.log(v * (t - mu) ** 2 + om) + torch.lgamma(a) \
        - torch.lgamma(a + 0.5)
    loss = torch.mean(nll + NIG_LAM * (torch.abs(t - mu) * (2 * v + a) - NIG_EPS))
    gs = torch.autograd.grad(loss, leaves)
    return float(loss.detach()), [g.double().numpy() for g in gs]


def _core(kind, d, dtype):
    ts = torch.tensor(np.array(d["score"])).to(dtype).requires_grad_(True)
    tv = torch.tensor(np.array(d["var"])).to(dtype).requires_grad_(True)
    tt = torch.tensor(np.array(d["targets"])).to(dtype)
    if kind == "mle":
        ref = O.listmle_loss(ts, SCOPE, tt).sum()
        return float(ref.detach()), [torch.autograd.grad(ref, ts)[0].double().numpy()]
    if kind == "listnet":
        ref = O.listnet_loss(ts, SCOPE, tt)
        return float(ref.detach()), [torch.autograd.grad(ref, ts)[0].double().numpy()]
    if kind == "evid":
        ref = O.evidential_ranking_loss(torch.stack([ts, tv], 1), SCOPE, tt).sum()
        return float(ref.detach()), [g.double().numpy() for g in torch.autograd.grad(ref, [ts, tv])]
    ref, pairs = O.ranknet_sum_session(ts, SCOPE, tt, 1.0)
    assert pairs == ranknet_pairs()
    g, = torch.autograd.grad(ref / pairs, ts)
    with torch.no_grad():
        lam = O.ranknet_lambda(ts.detach(), SCOPE, tt, 1.0) / pairs
    return float(ref.detach()) / pairs, [g.double().numpy(), lam.double().numpy()]


def ranknet_pairs():
    return sum(c * c - c for c in SCOPE)           # the targets have no ties


def evaluate(kind, d, dtype=torch.float64, stable=False):
    """(value, [gradient per input column]) of `kind` on the columns d, evaluated in `dtype` on the CPU.  value is the loss
    (loss_sum for the window losses, loss_sum / pairs for RankNet) or, for soft_rank, the rank vector.  stable: the
    logsumexp restatement of the three factorised variants in place of the reference's pair form."""
    cols = [d[c] for c in KINDS[kind][0]]
    t = d["targets"]
    with np.errstate(all="ignore"):
        if kind in CORE:
            return _core(kind, d, dtype)
        if kind in LV.KINDS:
            if stable:
                return stable_variant(kind, cols, SCOPE, t, dtype)
            return LV.variant_loss(kind, cols, SCOPE, t, UQ_COEF, dtype=dtype)
        if kind in ("gauss_nll", "mse", "lognorm", "exp_mse"):
            return pointwise(kind, cols, t, dtype)
        if kind in ("nig", "nig_cross"):
            return nig(cols, t, kind == "nig_cross", dtype)
        if kind.startswith("lambdarank"):
            loss, pairs, g = LR.lambdarank(cols[0], SCOPE, t, 1.0, int(kind.split("_k")[1]), dtype=dtype)
            assert pairs == ranknet_pairs()
            return loss, [g]
        if kind.startswith("approx_ndcg"):
            loss, ranked, g = AR.approx_ndcg(cols[0], SCOPE, t, 1.0, int(kind.split("_k")[1]), dtype=dtype)
            assert ranked == len(SCOPE) - 1        # the one-candidate query is unranked
            return loss, [g]
        if kind == "soft_rank":
            r, g = AR.soft_rank(cols[0], SCOPE, 1.0, soft_rank_upstream(), dtype=dtype)
            return r, [g]
        loss, pairs, g = PV.sq_loss(kind, cols[0], SCOPE, t, BETA_PARAM[kind], dtype=dtype)
        assert pairs == ranknet_pairs()
        return loss, [g]


@functools.lru_cache(maxsize=None)
def soft_rank_upstream():
    return _f32(np.random.default_rng(SEED + 1).standard_normal(M))


def _freeze(out):
    value, grads = out
    for a in grads + ([value] if isinstance(value, np.ndarray) else []):
        a.setflags(write=False)
    return value, tuple(grads)


@functools.lru_cache(maxsize=None)
def reference(kind, regime):
    """the float64 reference of a pair (computed once, read-only)"""
    return _freeze(evaluate(kind, inputs(regime), torch.float64))


@functools.lru_cache(maxsize=None)
def float32_run(kind, regime):
    """the float32 CPU evaluation that serves as yardstick: the stable restatement for the three factorised variants"""
    return _freeze(evaluate(kind, inputs(regime), torch.float32, stable=kind in FACTORISED))


def is_finite(out):
    value, grads = out
    return bool(np.isfinite(np.asarray(value, np.float64)).all() and all(np.isfinite(g).all() for g in grads))


# ------------------------------------------------------------------------------------------------ the measure
def value_error(kind, got, ref):
    if kind == "soft_rank":
        got = np.asarray(got, np.float64).reshape(-1)
        return float(np.max(np.abs(got - ref) / ref))
    return abs(float(got) - ref) / abs(ref)


def grad_error(got, ref):
    g = np.asarray(got, np.float64).reshape(-1)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    return float(np.max(np.abs(g - ref)) / np.max(np.abs(ref)))          # (a NaN anywhere makes this NaN, which fails)


def errors(kind, got, ref):
    """[value error, gradient error per column] of an evaluation against the reference"""
    return [value_error(kind, got[0], ref[0])] + [grad_error(a, b) for a, b in zip(got[1], ref[1])]


def labels(kind):
    names = GRAD_NAMES.get(kind) or tuple("d " + c for c in KINDS[kind][0])
    return ("ranks" if kind == "soft_rank" else "loss",) + names


def rule(e):
    return BOUND if e <= 1.25e-6 else 8 * e


@functools.lru_cache(maxsize=None)
def yardstick(kind, regime):
    """(the float32 CPU figure of a pair: the largest of its value and gradient errors, the bound the rule derives from it).
    The two double-precision Beta kernels are held to 1e-5 at most."""
    e = max(errors(kind, float32_run(kind, regime), reference(kind, regime)))
    return e, (min(rule(e), BOUND) if kind in DOUBLE_KERNELS else rule(e))


# the pairs whose float32 CPU figure is above 1.25e-6, with that figure rounded up in the second digit (module docstring);
# every other pair is at or below 1.25e-6 (tests/test_loss_range_cpu.py::test_every_yardstick_is_within_its_recorded_figure)
YARDSTICK_ABOVE = {
    ("mledis", "var_over"): 1.4e-6, ("listnet_lognorm", "var_over"): 1.8e-6,
    ("nig", "evidence_small"): 1.4e-6, ("nig", "evidence_large"): 1.7e-6,
    ("nig_cross", "tiny"): 1.01e-5, ("nig_cross", "evidence_small"): 1.8e-6, ("nig_cross", "evidence_large"): 2.8e-6,
    ("betanet", "up20"): 1.0, ("betanet", "down20"): 1.02e-5, ("betanet", "spread8"): 1.0e-5, ("betanet", "tiny"): 9.4e-6,
    ("betanet", "raw_targets"): 1.4e-6, ("betanet", "far_targets"): 1.4e-6,
}
# case 2: the kernels whose reference forms see only score differences, or shift, at score +- 120
SHIFTED_KINDS = ("listnet", "evid", "ranknet", "mledis", "listnet_gauss", "listnet_evidential", "lambdarank_k0", "approx_ndcg_k0",
                 "soft_rank")
CASE2_PAIRS = [(k, r) for k in SHIFTED_KINDS for r in ("up120", "down120")]


# ------------------------------------------------------------------------------------------------ the hand-built cases
def ranknet_overflow_case():
    """(scope, score, targets) of one 70-candidate list with ONE overflowing pair.  RankNet's cost of the pair {a, b} with
    t_a > t_b is log(1 + exp(s_b - s_a)) for both of its orders, so a pair overflows when the candidate with the lower target
    scores 150 higher.  Scores N(0, 1) except candidate 11 at 150; candidate 40 has the highest target, candidate 11 the
    second highest: {40, 11} has the argument 150 - s_40, every other pair of 11 has s - 150, the rest |s_a - s_b| < 10."""
    rng = np.random.default_rng(SEED + 2)
    score = rng.standard_normal(70)
    score[11] = 150.0
    rank = rng.permutation(70).astype(np.float64)          # a target order without ties
    order = [40, 11] + [i for i in np.argsort(-rank, kind="stable") if i not in (40, 11)]
    t = np.empty(70)
    t[order] = np.arange(70, 0, -1)
    t = (t - t.mean()) / (t.std() + 1e-6)
    return [70], _f32(score), _f32(t)


def ranknet_case_arguments():
    """every exp argument of RankNet's loss on that list: s_(lower target) - s_(higher target) per pair"""
    _, s, t = ranknet_overflow_case()
    s, t = s.astype(np.float64), t.astype(np.float64)
    hi = t[:, None] > t[None, :]
    return (s[None, :] - s[:, None])[hi]


KL_QUERY, KL_AT, KL_SCORE = 3, 10 + 5, 120.0               # a score of 120 inside the 64-candidate query


def kl_case():
    """the base scores with one score of 120 in query KL_QUERY: calculate_ndcg's exp(120) is inf in float32, its softmax
    inf / inf"""
    s = np.array(base()["score"])
    s[KL_AT] = KL_SCORE
    return _f32(s)


HEAD_RAWS = (50.0, -50.0, 110.0, -110.0)
HEADS = ((0, 1), (1, 1), (2, 1), (3, 2), (4, 2), (5, 2), (6, 4), (3, 4), (6, 8))     # test_relu_bwd_axpby_head_segment's


def head_reference(raw, head):
    """(out, d out / d raw as a per-entry factor) of a head in float64, laid out like the kernel's output:
    out[m, j * G + g] = act_g(raw[m, g * (N / G) + j]); softplus and sigmoid in float64, the variance floor 1e-6"""
    raw = np.asarray(raw, np.float64)
    n = raw.shape[1]
    G = {0: 1, 1: 1, 2: 1, 3: 2, 4: 2, 5: 2, 6: 4}[head]
    mv = 1e-6
    acts = {0: [None], 1: [0.0], 2: [1.0], 3: [None, mv], 4: [None, 0.0], 5: [mv, mv], 6: [None, mv, mv + 1.0, mv]}[head]
    out, slope, col_in = np.empty_like(raw), np.empty_like(raw), np.empty(n, np.int64)
    for c in range(n):
        j, g = c // G, c % G
        ci = g * (n // G) + j
        col_in[c] = ci
        x = raw[:, ci]
        if acts[g] is None:
            out[:, c], slope[:, c] = x, 1.0
        else:
            out[:, c] = np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x))) + acts[g]
            slope[:, c] = np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))
    return out, slope, col_in, [a is not None for a in acts]
