"""Single-forward (analytic) uncertainty without a GPU: the C-ABI export, the quadrature, the float64 restatement
(tests/analytic_uq_ref.py) against closed forms and against sampling, and the argument checks that come before any launch
or model use.  The kernel itself is held to the restatement in tests/test_gpu_analytic_uq.py."""
import math
import os
import re

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from reactranker_amd import uncertainty as U
from tests.analytic_uq_ref import analytic_ref, list_ref, sampled_p_top1

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "rr_analytic_rank_stats_f32"


def _phi(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def _list(rng, c):
    """Means N(0, 1), variances in [0.05, 0.55]: the header's 'comparable variances'."""
    return rng.standard_normal(c), 0.05 + 0.5 * rng.random(c)


# ---------------------------------------------------------------------------------------------- the C-ABI
def test_the_symbol_is_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "reactranker_hip.h")).read()
    assert SYMBOL in set(re.findall(r"\b(rr_[a-z0-9_]+)\s*\(", hdr))
    assert "#define RR_UQ_NQSTATS 4" in hdr
    assert re.search(r"#define RR_UQ_MAX_NODES (\d+)", hdr).group(1) == str(U.MAX_NODES) == "128"
    for name, value in U.MOMENT_KINDS.items():
        assert re.search(rf"RR_MOMENT_{name.upper()} = {value}\b", hdr), name
    assert SYMBOL in _lib.EXPORTED_SYMBOLS
    lib = _lib.lib()
    assert len(getattr(lib, SYMBOL).argtypes) == 19
    assert lib.rr_version() == 8 == _lib.ABI_VERSION


def test_head_to_kind_map():
    assert U.MOMENT_KIND_OF_HEAD == {3: "gaussian", 4: "gaussian", 6: "nig"}


# ---------------------------------------------------------------------------------------------- quadrature
@pytest.mark.parametrize("n", [1, 2, 8, 32, 127, 128])
def test_quadrature_is_normalised_hermegauss(n):
    x, w = U.quadrature(n)
    hx, hw = np.polynomial.hermite_e.hermegauss(n)
    assert x.dtype == np.float64 and w.dtype == np.float64 and x.shape == w.shape == (n,)
    assert np.array_equal(x, hx) and np.array_equal(w, hw / hw.sum())
    assert np.allclose(x, -x[::-1], rtol=0, atol=1e-12) and np.allclose(w, w[::-1], rtol=1e-9, atol=0)
    assert abs(w.sum() - 1.0) <= 1e-15
    if n >= 2:                                                    # the rule integrates x^2 under N(0, 1) exactly
        assert abs(float((w * x * x).sum()) - 1.0) <= 1e-12


@pytest.mark.parametrize("n", [0, 129, -1, 2.5])
def test_quadrature_refuses_node_counts_outside_1_to_128(n):
    with pytest.raises(ValueError, match="n_nodes"):
        U.quadrature(n)


# ---------------------------------------------------------------------------------------------- the restatement
def test_two_candidates_match_the_closed_form():
    """P(X1 > X2) = Phi((mu1 - mu2) / sqrt(s1^2 + s2^2)); at equal variances the 32-node rule gives it within 1e-9."""
    worst = 0.0
    for mu1, mu2, var in ((0.3, -0.2, 0.25), (0.0, 0.0, 0.05), (-1.0, 1.5, 0.55), (2.0, 1.9, 0.1)):
        p, rank = list_ref([mu1, mu2], [var, var], 32)
        want = _phi((mu1 - mu2) / math.sqrt(2 * var))
        worst = max(worst, abs(p[0] - want), abs(p[1] - (1 - want)))
        assert abs(rank[0] - (2 - want)) <= 1e-12 and abs(rank[1] - (1 + want)) <= 1e-12     # the rank IS the closed form
    print(f"two candidates, equal variances, 32 nodes: worst |p - closed form| = {worst:.3e}")
    assert worst <= 1e-9


def test_a_list_of_one_and_the_rank_sum():
    p, rank = list_ref([0.7], [0.3], 32)
    assert abs(p[0] - 1.0) <= 1e-15 and np.float32(p[0]) == 1.0 and rank.tolist() == [1.0]   # (the weights sum to 1 within 1e-15)
    rng = np.random.default_rng(5)
    for c in (2, 5, 64, 300):
        mu, var = _list(rng, c)
        _, rank = list_ref(mu, var, 8)
        assert abs(rank.sum() - c * (c + 1) / 2) <= 1e-9, c
        assert np.all(rank >= 1) and np.all(rank <= c)


@pytest.mark.parametrize("c", [5, 64, 300])
def test_mass_is_one_for_comparable_variances(c):
    rng = np.random.default_rng(40 + c)
    mu, var = _list(rng, c)
    p32, _ = list_ref(mu, var, 32)
    p128, _ = list_ref(mu, var, 128)
    print(f"C={c}: |mass - 1| = {abs(p32.sum() - 1):.3e} (32 nodes), max |p32 - p128| = {np.abs(p32 - p128).max():.3e}")
    assert abs(p32.sum() - 1.0) <= 1e-3


def test_the_quadrature_limit_for_unequal_variances():
    """The documented limit (include/reactranker_hip.h): under candidate i's own Gaussian a rival with 1/k of
    its variance is a step of relative width 1/sqrt(k), which the rule resolves only while its nodes are closer than that.
    Two candidates, where the closed form is the truth; the bounds are the header's figures for the same variance ratios."""
    documented = {(10.0, 32): 1.7e-4, (100.0, 32): 9e-3, (100.0, 128): 1.1e-3}
    for (k, n), bound in documented.items():
        p, _ = list_ref([0.1, 0.0], [0.5 * k, 0.5], n)
        err = abs(p[0] - _phi(0.1 / math.sqrt(0.5 * k + 0.5)))
        print(f"variance ratio {k:g}, {n} nodes: |p - closed form| = {err:.3e} (documented {bound:g})")
        assert err <= bound, (k, n)


def test_p_top1_against_400000_samples():
    rng = np.random.default_rng(64)
    mu, var = _list(rng, 64)
    p, _ = list_ref(mu, var, 32)
    T = 400_000
    s = sampled_p_top1(mu, var, T, seed=1)
    excess = np.abs(p - s) - 4 * np.sqrt(p * (1 - p) / T)
    print(f"C=64, T={T}: worst |p - sampled| = {np.abs(p - s).max():.3e}, worst excess over 4 sigma = {excess.max():.3e}")
    assert np.all(excess <= 1e-3)


def test_kinds_decode_to_the_same_list():
    """The three kinds of one (mu, var) list give the same p_top1 and ranks; NIG splits the variance as documented."""
    rng = np.random.default_rng(9)
    mu, var = _list(rng, 7)
    mu, var = mu.astype(np.float32), var.astype(np.float32)
    tg = rng.standard_normal(7).astype(np.float32)
    g = analytic_ref(np.stack([mu, var], 1), [3, 0, 4], tg, "gaussian", 8)
    lv = analytic_ref(np.stack([mu, np.log(var.astype(np.float64)).astype(np.float32)], 1), [3, 0, 4], tg, "log_variance", 8)
    assert np.allclose(g["p_top1"], lv["p_top1"], rtol=0, atol=1e-6) and np.array_equal(g["mean"], lv["mean"])
    v, alpha, beta = np.float32(2.0), np.float32(3.0), var          # aleatoric = beta / 2, epistemic = beta / 4
    nig = analytic_ref(np.stack([mu, np.full(7, v), np.full(7, alpha), beta], 1), [3, 0, 4], tg, "nig", 8)
    assert np.allclose(nig["std"] ** 2, 0.75 * var.astype(np.float64), rtol=1e-12)
    assert np.allclose(nig["aleatoric_std"] ** 2, 0.5 * var.astype(np.float64), rtol=1e-12)
    assert np.allclose(nig["epistemic_std"] ** 2, 0.25 * var.astype(np.float64), rtol=1e-12)
    assert np.all(g["qstats"][1] == 0) and g["mass"][1] == 0        # the empty list
    assert g["qstats"][0, 1] == np.float32(g["p_top1"][int(np.argmax(tg[:3]))])
    assert abs(g["qstats"][2, 3] - np.sqrt(var[3:].astype(np.float64)).astype(np.float32).astype(np.float64).mean()) <= 1e-15


# ---------------------------------------------------------------------------------------------- refusals before any launch
@pytest.mark.parametrize("n", [0, 129])
def test_bad_node_counts_are_refused_before_any_launch(n):
    out = torch.zeros(5, 2)                                        # CPU tensors: any launch attempt would fail differently
    with pytest.raises(ValueError, match="n_nodes"):
        U.analytic_stats(out, [5], torch.zeros(5), "gaussian", n_nodes=n)
    with pytest.raises(ValueError, match="n_nodes"):
        U.distribution_predict(object(), [], kind="gaussian", n_nodes=n)   # not even a model: nothing may be touched
    with pytest.raises(ValueError, match="n_nodes"):
        U.evaluate_uncertainty(object(), [], "x.pt", 0, method="distribution", n_nodes=n)


def test_an_unknown_kind_is_refused_before_any_launch():
    with pytest.raises(ValueError, match="kind"):
        U.analytic_stats(torch.zeros(5, 2), [5], torch.zeros(5), "lognormal")
    with pytest.raises(ValueError, match="kind"):
        U.distribution_predict(object(), [], kind="student")
    with pytest.raises(ValueError, match="kind"):
        U.evaluate_uncertainty(object(), [], "x.pt", 0, method="distribution", kind="student")


@pytest.mark.parametrize("kind,shape", [("gaussian", (5, 1)), ("log_variance", (5, 1)), ("nig", (5, 3)), ("gaussian", (5,))])
def test_too_few_columns_are_refused_before_any_launch(kind, shape):
    with pytest.raises(ValueError, match="columns"):
        U.analytic_stats(torch.zeros(*shape), [5], torch.zeros(5), kind)


def test_distribution_takes_one_checkpoint_and_the_method_message_lists_all_three():
    with pytest.raises(ValueError, match="one checkpoint"):
        U.evaluate_uncertainty(object(), [], ["a.pt", "b.pt"], 0, method="distribution")
    with pytest.raises(ValueError) as e:
        U.evaluate_uncertainty(object(), [], "x.pt", 0, method="bootstrap")
    for m in ("MC_dropout", "ensemble", "distribution"):
        assert m in str(e.value)
