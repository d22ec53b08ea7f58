"""CPU-side checks of the soft ranks, the ApproxNDCG loss and its strategy: the eight entry points are declared, exported,
bound and reject bad arguments before any launch; run_train's selector and Config; and the float64 restatement of
tests/approx_ndcg_ref.py - its closed-form gradient against autograd, the identities of the soft ranks, a three-candidate query
by hand, the hard-NDCG limit, and what plain float32 pair terms do to the same formulas."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import approx_ndcg_ref as AR

from reactranker_amd import _lib
from reactranker_amd import loss as RL
from reactranker_amd import run_train_pairwise as RT
from reactranker_amd.main import Config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rr_soft_rank_fwd_f32", "rr_soft_rank_bwd_f32", "rr_approx_ndcg_fwd_f32", "rr_approx_ndcg_bwd_f32",
               "rr_approx_ndcg_step_f32", "rr_approx_ndcg_ranks_f32", "rr_approx_ndcg_waves", "rr_approx_ndcg_set_waves"]
SETTINGS = [(1.0, 0), (0.1, 0), (1.0, 10), (0.01, 5)]
BAD_T = (0.0, -1.0, float("nan"), float("inf"), 2.9e-39)   # the last: a positive subnormal whose float32 reciprocal is inf


def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(REPO, "include", "reactranker_hip.h")) as f:
        declared = set(re.findall(r"\b(rr_\w+)\s*\(", f.read()))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert getattr(_lib.lib(), s).argtypes is not None
    assert _lib.lib().rr_version() == _lib.ABI_VERSION == 8          # additive: new symbols only


def test_soft_rank_entry_points_reject_bad_arguments_before_any_launch():
    l = _lib.lib()
    one = ctypes.c_void_p(256)
    fwd, bwd = l.rr_soft_rank_fwd_f32, l.rr_soft_rank_bwd_f32
    #   score, stride, seg_off, Q, max_len, temperature, rank, rank_stride
    assert fwd(None, 1, one, 1, 4, 1.0, one, 1, None) == -1                           # null scores
    assert fwd(one, 1, None, 1, 4, 1.0, one, 1, None) == -1                           # null seg_off
    assert fwd(one, 1, one, 1, 4, 1.0, None, 1, None) == -1                           # null ranks
    assert fwd(one, 0, one, 1, 4, 1.0, one, 1, None) == -1                            # stride < 1
    assert fwd(one, 1, one, 1, 4, 1.0, one, 0, None) == -1
    assert fwd(one, 1, one, -1, 4, 1.0, one, 1, None) == -1                           # Q < 0
    for bad in BAD_T:
        assert fwd(one, 1, one, 1, 4, bad, one, 1, None) == -1, bad                   # temperature
    assert fwd(one, 1, one, 1, 8193, 1.0, one, 1, None) == -4                         # list too long: nothing launched
    assert fwd(one, 1, one, 0, 4, 1.0, one, 1, None) == 0                             # no queries: nothing launched
    assert fwd(one, 1, one, 0, 4, 3.0e-39, one, 1, None) == 0                         # a subnormal with a finite reciprocal is fine
    #   ..., drank, drank_stride, dscore, dscore_stride
    assert bwd(None, 1, one, 1, 4, 1.0, one, 1, one, 1, None) == -1
    assert bwd(one, 1, None, 1, 4, 1.0, one, 1, one, 1, None) == -1
    assert bwd(one, 1, one, 1, 4, 1.0, None, 1, one, 1, None) == -1                   # null upstream gradient
    assert bwd(one, 1, one, 1, 4, 1.0, one, 1, None, 1, None) == -1                   # null gradient
    assert bwd(one, 0, one, 1, 4, 1.0, one, 1, one, 1, None) == -1
    assert bwd(one, 1, one, 1, 4, 1.0, one, 0, one, 1, None) == -1
    assert bwd(one, 1, one, 1, 4, 1.0, one, 1, one, 0, None) == -1
    assert bwd(one, 1, one, -1, 4, 1.0, one, 1, one, 1, None) == -1
    for bad in BAD_T:
        assert bwd(one, 1, one, 1, 4, bad, one, 1, one, 1, None) == -1, bad
    assert bwd(one, 1, one, 1, 8193, 1.0, one, 1, one, 1, None) == -4
    assert bwd(one, 1, one, 0, 4, 1.0, one, 1, one, 1, None) == 0


def test_approx_ndcg_entry_points_reject_bad_arguments_before_any_launch():
    l = _lib.lib()
    one = ctypes.c_void_p(256)
    fwd, bwd, step, ranks = l.rr_approx_ndcg_fwd_f32, l.rr_approx_ndcg_bwd_f32, l.rr_approx_ndcg_step_f32, l.rr_approx_ndcg_ranks_f32
    #   score, stride, targets, seg_off, Q, max_len, temperature, ndcg_k, ...
    tails = [(fwd, (one, one, one)), (bwd, (one, one, 1)), (step, (1.0, one, one, one, one, one, 1)), (ranks, (one, 1))]
    for fn, tail in tails:
        assert fn(None, 1, one, one, 1, 4, 1.0, 0, *tail, None) == -1                 # null scores
        assert fn(one, 1, None, one, 1, 4, 1.0, 0, *tail, None) == -1                 # null targets
        assert fn(one, 1, one, None, 1, 4, 1.0, 0, *tail, None) == -1                 # null seg_off
        assert fn(one, 0, one, one, 1, 4, 1.0, 0, *tail, None) == -1                  # stride < 1
        assert fn(one, 1, one, one, -1, 4, 1.0, 0, *tail, None) == -1                 # Q < 0
        for bad in BAD_T:
            assert fn(one, 1, one, one, 1, 4, bad, 0, *tail, None) == -1, bad         # temperature
        assert fn(one, 1, one, one, 1, 4, 1.0, -1, *tail, None) == -1                 # ndcg_k < 0
        assert fn(one, 1, one, one, 1, 8193, 1.0, 0, *tail, None) == -4               # list too long: nothing launched
        for n, v in enumerate(tail):                                                  # every pointer and stride of the tail
            if fn is step and n == 0:
                continue                                                              # (the scale is any float)
            broken = list(tail)
            broken[n] = None if not isinstance(v, int) else 0
            assert fn(one, 1, one, one, 1, 4, 1.0, 0, *broken, None) == -1, (fn.__name__, n)
    assert bwd(one, 1, one, one, 0, 4, 1.0, 0, one, one, 1, None) == 0                # no queries: nothing launched
    assert ranks(one, 1, one, one, 0, 4, 1.0, 0, one, 1, None) == 0


def test_wave_count_setter():
    l = _lib.lib()
    assert l.rr_approx_ndcg_waves() == 0                                              # by max_len
    try:
        for w in (1, 4, 0):
            assert l.rr_approx_ndcg_set_waves(w) == 0 and l.rr_approx_ndcg_waves() == w
        for w in (-1, 2, 3, 8):
            assert l.rr_approx_ndcg_set_waves(w) == -1 and l.rr_approx_ndcg_waves() == 0
    finally:
        l.rr_approx_ndcg_set_waves(0)


def test_selector_config_and_python_argument_checks():
    assert RT.select_loop("approx_ndcg", "baseline") == "approx_ndcg"
    assert RT.select_loop("approx_ndcg", "BetaNet") == "BetaNet"                      # task_type still decides first
    assert RT.select_loop("lambdarank", "baseline") == "lambdarank"
    with pytest.raises(ValueError, match="pairwise selectors") as e:
        RT.select_loop("approx_ndcg", "listnet")
    assert "approx_ndcg" in str(e.value)
    with pytest.raises(ValueError, match="pairwise selectors"):                       # refused before anything touches a device
        RT.run_train(None, None, [], [], None, None, 1, 0, 0, train_strategy="approxndcg", task_type="baseline", temperature=0.5)
    cfg = Config(path="unused", task_type="ranknet", train_strategy="approx_ndcg", ndcg_k=10, temperature=0.5)
    assert cfg.temperature == 0.5 and Config(path="unused").temperature == 1.0
    s = torch.zeros(3)
    for bad in BAD_T:
        with pytest.raises(ValueError, match="temperature"):
            RL.approx_ndcg_loss(s, [3], s, temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            RL.soft_rank(s, [3], temperature=bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="ndcg_k"):
            RL.approx_ndcg_loss(s, [3], s, ndcg_k=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="queries"):
            RL.approx_ndcg_loss(s, [3], s, queries=bad)


@pytest.mark.parametrize("T,k", SETTINGS)
def test_closed_form_gradient_equals_autograd_and_the_rank_identities_hold(T, k):
    scope = [1, 2, 3, 12, 64, 65, 0, 130]
    score, targets = AR.window(0, scope)
    targets[:1 + 2] = targets[0]                                                      # queries 0 and 1 are unranked
    loss, ranked, grad, a = AR.approx_ndcg(score, scope, targets, T, k, block=50, terms=True)
    loss_c, ranked_c, grad_c, a_c = AR.approx_ndcg(score, scope, targets, T, k, block=4096, closed=True, terms=True)
    assert ranked == ranked_c == 5
    assert abs(loss - loss_c) <= 1e-12 * abs(loss)
    assert np.max(np.abs(grad - grad_c)) <= 1e-12 * np.abs(grad).max()
    assert np.max(np.abs(a - a_c)) <= 1e-12 * np.abs(a).max()
    assert 0.0 < loss < ranked and np.all(grad[:3] == 0)
    up = np.random.default_rng(1).standard_normal(len(score))
    r, g = AR.soft_rank(score, scope, T, up, block=50)
    r_c, g_c = AR.soft_rank(score, scope, T, up, block=4096, closed=True)
    assert np.max(np.abs(r - r_c)) <= 1e-12 * r.max() and np.max(np.abs(g - g_c)) <= 1e-12 * np.abs(g).max()
    off = 0
    for c in scope:
        assert abs(r[off:off + c].sum() - c * (c + 1) / 2) <= 1e-12 * max(1, c * c), c
        for v in (grad, g):
            assert abs(v[off:off + c].sum()) <= 1e-12 * max(1.0, np.abs(v[off:off + c]).sum()), c
        off += c


def test_three_candidate_query_by_hand():
    """scores 3, 1, 2 and targets 0, 1, 2 at T = 0.7, every term written out; k = 2 gates at rank 2.5"""
    s = np.array([3.0, 1.0, 2.0], np.float32)
    t = np.array([0.0, 1.0, 2.0], np.float32)
    T = 0.7
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    dsig = lambda x: sig(x) * (1.0 - sig(x))
    r = np.array([1 + sig(-2 / T) + sig(-1 / T), 1 + sig(2 / T) + sig(1 / T), 1 + sig(1 / T) + sig(-1 / T)])
    ranks, _ = AR.soft_rank(s, [3], T)
    assert np.max(np.abs(ranks - r)) <= 1e-15
    g = np.exp(t.astype(np.float64) - 2.0)
    l2 = np.log2(1.0 + r)
    dl2 = 1.0 / ((1.0 + r) * np.log(2.0))
    for k in (0, 2):
        max_dcg = g[2] + g[1] / np.log2(3.0) + (g[0] / 2.0 if k == 0 else 0.0)
        gate = sig(2.5 - r) if k == 2 else np.ones(3)
        dgate = -dsig(2.5 - r) if k == 2 else np.zeros(3)
        want = 1.0 - np.sum(g / max_dcg * gate / l2)
        a = -(g / max_dcg) * (dgate / l2 - gate * dl2 / l2 ** 2)
        wgrad = np.array([sum(dsig((float(s[j]) - float(s[i])) / T) * (a[j] - a[i]) for j in range(3) if j != i) / T for i in range(3)])
        loss, ranked, grad, a_ref = AR.approx_ndcg(s, [3], t, T, k, terms=True)
        assert ranked == 1 and abs(loss - want) <= 1e-15
        assert np.max(np.abs(a_ref - a)) <= 1e-15 and np.max(np.abs(grad - wgrad)) <= 1e-15


def test_all_tied_scores_give_the_middle_rank():
    for c in (1, 2, 5, 64, 65):
        r, _ = AR.soft_rank(np.full(c, 0.25, np.float32), [c], 0.3)
        assert np.all(r == (c + 1) / 2), c


def test_small_temperature_on_integer_spaced_scores_is_one_minus_the_hard_ndcg():
    rng = np.random.default_rng(3)
    for c in (2, 7, 40):
        s = rng.permutation(c).astype(np.float32)                                     # spacing 1 = 100 T: sigmoid(+-100) is 0 or 1
        _, t = AR.window(c, [c])
        order = np.argsort(-s)
        g = np.exp(t.astype(np.float64) - t.max())
        disc = 1.0 / np.log2(np.arange(1, c + 1) + 1.0)
        ndcg = np.sum(g[order] * disc) / np.sum(np.sort(g)[::-1] * disc)
        loss, ranked, _ = AR.approx_ndcg(s, [c], t, 0.01, 0)
        assert ranked == 1 and abs(loss - (1.0 - ndcg)) <= 1e-12


def test_ndcg_k_at_or_beyond_the_list_length_is_ndcg_k_zero():
    scope = [5, 12]
    score, targets = AR.window(4, scope)
    base = AR.approx_ndcg(score, scope, targets, 0.5, 0)
    for k in (12, 13, 1000):
        got = AR.approx_ndcg(score, scope, targets, 0.5, k)
        assert got[0] == base[0] and np.array_equal(got[2], base[2]), k
    assert AR.approx_ndcg(score, scope, targets, 0.5, 11)[0] != base[0]               # (11 gates the list of 12)


@pytest.mark.parametrize("T,k", SETTINGS)
def test_float32_pair_terms_stay_far_below_the_parity_bound(T, k):
    """What the GPU parity bound of 1e-5 leaves room for: the closed form with float32 pair terms in the e form and float64
    sums, as the kernels evaluate it.  Measured on these lists: loss <= 3.7e-9, gradient <= 1.4e-7 of the list's largest entry.
    The bounds come from the format, not from those figures.  Gradient 5e-7: a pair term is about eight rounded float32
    operations from the margin to the product with a_j - a_k, half an ulp (2^-24 = 6e-8) each, and 8 * 2^-24 = 4.8e-7 is all
    of them falling the same way on the terms that make the largest entry; the float64 sums add nothing.  Loss 2e-8: the loss
    is at most 1 and sees the pair terms only through the ranks, each a float64 sum of C - 1 independently rounded sigmoids,
    so their half-ulps average out instead of adding up - a third of one half-ulp is left as the bound.  sigmoid (1 - sigmoid)
    in place of e / (1 + e)^2 loses the gradient bound by two orders of magnitude at T = 0.01 (2.9e-5)."""
    for seed, c in enumerate((5, 64, 300, 1000, 4096)):
        score, targets = AR.window(20 + seed, [c])
        loss, _, grad = AR.approx_ndcg(score, [c], targets, T, k, closed=True)
        l32, _, g32 = AR.approx_ndcg(score, [c], targets, T, k, dtype=torch.float32)
        assert abs(l32 - loss) <= 2e-8, (c, abs(l32 - loss))
        assert np.max(np.abs(g32 - grad)) <= 5e-7 * np.abs(grad).max(), (c, np.max(np.abs(g32 - grad)) / np.abs(grad).max())
