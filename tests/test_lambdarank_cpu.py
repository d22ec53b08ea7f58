"""CPU-side checks of the LambdaRank loss and strategy: the three entry points are declared, exported, bound and reject bad
arguments before any launch; run_train's selector; and the float64 restatement of tests/lambdarank_ref.py counts RankNet's
pairs, has a gradient that sums to zero inside every query (the loss depends on score differences only) and gives the terms
written out by hand on a three-candidate query."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import lambdarank_ref as LR

from oracle import ref_cpu as O
from reactranker_amd import _lib
from reactranker_amd import run_train_pairwise as RT
from reactranker_amd.main import Config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rr_lambdarank_fwd_f32", "rr_lambdarank_bwd_f32", "rr_lambdarank_step_f32"]


window = LR.window


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


def test_entry_points_reject_bad_arguments_before_any_launch():
    l = _lib.lib()
    one = ctypes.c_void_p(256)
    fwd, bwd, step = l.rr_lambdarank_fwd_f32, l.rr_lambdarank_bwd_f32, l.rr_lambdarank_step_f32
    #   score, stride, targets, seg_off, Q, max_len, sigma, ndcg_k, ...
    assert fwd(None, 1, one, one, 1, 4, 1.0, 0, one, one, one, None) == -1            # null scores
    assert fwd(one, 1, None, one, 1, 4, 1.0, 0, one, one, one, None) == -1            # null targets
    assert fwd(one, 1, one, None, 1, 4, 1.0, 0, one, one, one, None) == -1            # null seg_off
    assert fwd(one, 1, one, one, 1, 4, 1.0, 0, None, one, one, None) == -1            # null loss
    assert fwd(one, 1, one, one, 1, 4, 1.0, 0, one, None, one, None) == -1            # null pairs
    assert fwd(one, 1, one, one, 1, 4, 1.0, 0, one, one, None, None) == -1            # null partials
    assert fwd(one, 0, one, one, 1, 4, 1.0, 0, one, one, one, None) == -1             # stride < 1
    assert fwd(one, 1, one, one, -1, 4, 1.0, 0, one, one, one, None) == -1            # Q < 0
    assert fwd(one, 1, one, one, 1, 4, 0.0, 0, one, one, one, None) == -1             # sigma <= 0
    assert fwd(one, 1, one, one, 1, 4, -1.0, 0, one, one, one, None) == -1
    assert fwd(one, 1, one, one, 1, 4, float("nan"), 0, one, one, one, None) == -1
    assert fwd(one, 1, one, one, 1, 4, 1.0, -1, one, one, one, None) == -1            # ndcg_k < 0
    assert fwd(one, 1, one, one, 1, 8193, 1.0, 0, one, one, one, None) == -4          # list too long: nothing launched
    #   ..., gloss, dscore, dscore_stride
    assert bwd(None, 1, one, one, 1, 4, 1.0, 0, one, one, 1, None) == -1
    assert bwd(one, 1, one, one, 1, 4, 1.0, 0, None, one, 1, None) == -1              # null upstream gradient
    assert bwd(one, 1, one, one, 1, 4, 1.0, 0, one, None, 1, None) == -1              # null gradient
    assert bwd(one, 1, one, one, 1, 4, 1.0, 0, one, one, 0, None) == -1               # gradient stride < 1
    assert bwd(one, 0, one, one, 1, 4, 1.0, 0, one, one, 1, None) == -1
    assert bwd(one, 1, one, one, -1, 4, 1.0, 0, one, one, 1, None) == -1
    assert bwd(one, 1, one, one, 1, 4, 0.0, 0, one, one, 1, None) == -1
    assert bwd(one, 1, one, one, 1, 4, 1.0, -2, one, one, 1, None) == -1
    assert bwd(one, 1, one, one, 1, 8193, 1.0, 0, one, one, 1, None) == -4
    assert bwd(one, 1, one, one, 0, 4, 1.0, 0, one, one, 1, None) == 0                # no queries: nothing launched
    #   ..., scale, loss, pairs, partial, counter, dscore, dscore_stride
    assert step(None, 1, one, one, 1, 4, 1.0, 0, 1.0, one, one, one, one, one, 1, None) == -1
    assert step(one, 1, one, one, 1, 4, 1.0, 0, 1.0, None, one, one, one, one, 1, None) == -1     # null loss
    assert step(one, 1, one, one, 1, 4, 1.0, 0, 1.0, one, None, one, one, one, 1, None) == -1     # null pairs
    assert step(one, 1, one, one, 1, 4, 1.0, 0, 1.0, one, one, None, one, one, 1, None) == -1     # null partials
    assert step(one, 1, one, one, 1, 4, 1.0, 0, 1.0, one, one, one, None, one, 1, None) == -1     # null counter
    assert step(one, 1, one, one, 1, 4, 1.0, 0, 1.0, one, one, one, one, None, 1, None) == -1     # null gradient
    assert step(one, 1, one, one, 1, 4, 1.0, 0, 1.0, one, one, one, one, one, 0, None) == -1      # gradient stride < 1
    assert step(one, 0, one, one, 1, 4, 1.0, 0, 1.0, one, one, one, one, one, 1, None) == -1
    assert step(one, 1, one, one, -1, 4, 1.0, 0, 1.0, one, one, one, one, one, 1, None) == -1
    assert step(one, 1, one, one, 1, 4, 0.0, 0, 1.0, one, one, one, one, one, 1, None) == -1
    assert step(one, 1, one, one, 1, 4, 1.0, -1, 1.0, one, one, one, one, one, 1, None) == -1
    assert step(one, 1, one, one, 1, 8193, 1.0, 0, 1.0, one, one, one, one, one, 1, None) == -4


def test_selector_and_config():
    assert RT.select_loop("lambdarank", "baseline") == "lambdarank"
    assert RT.select_loop("lambdarank", "BetaNet") == "BetaNet"                      # task_type still decides first
    assert RT.select_loop("sum_session", "baseline") == "sum_session"
    with pytest.raises(ValueError, match="pairwise selectors") as e:
        RT.select_loop("lambdarank", "listnet")
    assert "lambdarank" in str(e.value)
    with pytest.raises(ValueError, match="pairwise selectors"):                      # refused before anything touches a device
        RT.run_train(None, None, [], [], None, None, 1, 0, 0, train_strategy="lambda_rank", task_type="baseline", ndcg_k=3)
    cfg = Config(path="unused", task_type="ranknet", train_strategy="lambdarank", ndcg_k=10)
    assert cfg.ndcg_k == 10 and Config(path="unused").ndcg_k == 0


@pytest.mark.parametrize("seed,scope", [(0, [1, 2, 3, 32, 64, 65, 129, 300]), (2, [5, 1, 1, 7]), (5, [4, 3, 1, 0, 5])])
@pytest.mark.parametrize("sigma,ndcg_k", [(1.0, 0), (0.5, 1), (1.0, 10)])
def test_restatement_counts_ranknets_pairs_and_its_gradient_sums_to_zero_per_query(seed, scope, sigma, ndcg_k):
    score, targets = window(seed, scope)
    if seed == 2:
        score[:] = 0.5                                                               # the tie rule decides every rank
    if seed == 5:                                                                    # pair-less queries: all targets equal
        targets[:4] = targets[0]
    loss, pairs, grad = LR.lambdarank(score, scope, targets, sigma, ndcg_k, block=50)
    _, pairs_ref = O.ranknet_sum_session(torch.tensor(score), scope, torch.tensor(targets), sigma)
    assert pairs == int(pairs_ref)
    assert np.isfinite(loss) and loss > 0 and np.all(np.isfinite(grad))
    off = 0
    for c in scope:
        g = grad[off:off + c]
        assert abs(g.sum()) <= 1e-12 * max(1.0, np.abs(g).sum()), (c, g.sum())
        off += c
    if seed == 5:
        assert np.all(grad[:4] == 0) and np.all(grad[7:8] == 0)
    # the row blocks are a way to bound memory, not part of the definition
    loss1, pairs1, grad1 = LR.lambdarank(score, scope, targets, sigma, ndcg_k, block=4096)
    assert pairs1 == pairs and abs(loss1 - loss) <= 1e-12 * loss and np.max(np.abs(grad1 - grad)) <= 1e-12 * np.abs(grad).max()


def test_restatement_weights_by_hand_on_a_three_candidate_query():
    """scores 3 > 1 > 2 put the candidates at ranks 1, 3, 2; targets 0 < 1 < 2.  Every term written out."""
    s = np.array([3.0, 1.0, 2.0], np.float32)
    t = np.array([0.0, 1.0, 2.0], np.float32)
    for k in (0, 2):
        D = np.array([1.0, 1 / np.log2(4.0) if k == 0 else 0.0, 1 / np.log2(3.0)])
        g = np.exp(t.astype(np.float64) - 2.0)
        ideal = np.sort(g)[::-1]
        max_dcg = ideal[0] + ideal[1] / np.log2(3.0) + (ideal[2] / 2.0 if k == 0 else 0.0)
        want, wgrad = 0.0, np.zeros(3)
        for i in range(3):
            for j in range(3):
                if t[i] == t[j]:
                    continue
                w = abs(g[i] - g[j]) * abs(D[i] - D[j]) / max_dcg
                x = 0.7 * (float(s[i]) - float(s[j]))
                y = x if t[i] > t[j] else -x
                want += w * np.log1p(np.exp(-y))
                d = -0.7 / (1 + np.exp(y)) * (1.0 if t[i] > t[j] else -1.0)
                wgrad[i] += w * d
                wgrad[j] -= w * d
        loss, pairs, grad = LR.lambdarank(s, [3], t, 0.7, k)
        assert pairs == 6
        assert abs(loss - want) <= 1e-14 * want
        assert np.max(np.abs(grad - wgrad)) <= 1e-14


def test_restatement_gradient_at_tied_scores_is_half_sigma_per_pair():
    """Two candidates with the same score: softplus'(0) = 1 / 2, so d loss_sum / d s = -/+ 2 w sigma / 2; ranks by position."""
    t = np.array([0.0, 1.0], np.float32)
    g = np.exp(t.astype(np.float64) - 1.0)
    w = abs(g[0] - g[1]) * abs(1.0 - 1.0 / np.log2(3.0)) / (g[1] + g[0] / np.log2(3.0))
    loss, pairs, grad = LR.lambdarank(np.array([0.5, 0.5], np.float32), [2], t, 0.8, 0)
    assert pairs == 2 and abs(loss - 2 * w * np.log(2.0)) <= 1e-15
    assert np.max(np.abs(grad - np.array([w * 0.8, -w * 0.8]))) <= 1e-15


def test_float32_evaluation_of_the_restatement_stays_far_below_the_parity_bound():
    """What the GPU parity bound of 1e-5 leaves room for: the same formulas in plain float32 torch arithmetic."""
    for seed, scope in ((0, [1, 2, 3, 32, 64, 65, 129, 300]), (1, [64] * 8)):
        score, targets = window(seed, scope)
        loss, pairs, grad = LR.lambdarank(score, scope, targets, 1.0, 0)
        l32, p32, g32 = LR.lambdarank(score, scope, targets, 1.0, 0, dtype=torch.float32)
        assert p32 == pairs
        assert abs(l32 - loss) / loss <= 1e-6
        assert np.max(np.abs(g32 - grad)) / np.abs(grad).max() <= 1e-6
