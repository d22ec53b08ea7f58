"""Every entry point ranks the same tied list the same way: the stable descending order (csrc/rr_common.h, rr_precedes and the
first maximum built on it) - candidate j comes before i iff x[j] > x[i], or x[j] == x[i] and j < i.

Lists of finite values drawn from {0, 0.5, 1}, so nearly every comparison is a tie, of 1, 2, 63, 64, 65, 129 and 257 candidates
and one all-equal list of 257; positions 63|64, 127|128 and 255|256 hold equal values wherever both exist, so a tie group
crosses a lane, a wave and a workgroup boundary of the four-wave kernels.  The reference is numpy's stable descending order,
np.argsort(-x, kind="stable"), and its inverse; every result below is compared with it as exact integers:
  eval.ranking_stats                 `order`
  rr_rank_correlation_f32            the reciprocal rank 1 / (1 + rank), waves 0, 1 and 4 - it ranks the target's first maximum
                                     only, so every list is repeated once per candidate with that candidate as the one maximum
                                     of the targets (which also checks the first maximum of a one-hot key)
  rr_top1_sets_f32                   `rank` (1-based), waves 0, 1 and 4
  rr_mc_sample_stats_f32             `mean_rank` of T = 2 identical samples: (2 rank + 2) / 2 = rank + 1 exactly
ApproxNDCG and LambdaRank count their target rank by the same rule, but no public function returns it (rr_approx_ndcg_ranks_f32
gives the gradient weights): they are not compared here.  No NaNs: the kernels that scatter by rank leave their output
undefined for them, and the NaN contracts are tested with each entry point."""
import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from reactranker_amd import eval as RE
from reactranker_amd import uncertainty as UQ

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 63, 64, 65, 129, 257)
BOUNDARIES = (63, 127, 255)          # positions b and b + 1 hold equal values
WAVES = (0, 1, 4)


def _lists():
    rng = np.random.default_rng(7)
    out = []
    for C in LENGTHS:
        x = rng.integers(0, 3, C).astype(np.float32) * 0.5
        for b in BOUNDARIES:
            if b + 1 < C:
                x[b + 1] = x[b]
        out.append(x)
    out.append(np.full(257, 0.5, np.float32))
    return out


LISTS = _lists()
SCOPE = [len(x) for x in LISTS]
X = np.concatenate(LISTS)
ORDER = [np.argsort(-x, kind="stable") for x in LISTS]             # ORDER[q][r] = the candidate at rank r
RANK = []                                                          # RANK[q][i] = the 0-based rank of candidate i
for o in ORDER:
    r = np.empty(len(o), np.int64)
    r[o] = np.arange(len(o))
    RANK.append(r)
for a in (X, *ORDER, *RANK):
    a.setflags(write=False)


def _pinned(setter, waves, fn):
    assert setter(waves) == 0
    try:
        return fn()
    finally:
        setter(0)


def test_the_lists_are_what_the_docstring_says():
    assert SCOPE == list(LENGTHS) + [257] and np.isfinite(X).all() and set(np.unique(X)) <= {0.0, 0.5, 1.0}
    for x in LISTS:
        for b in BOUNDARIES:
            assert b + 1 >= len(x) or x[b] == x[b + 1]
    assert len(np.unique(LISTS[-1])) == 1 and any(len(np.unique(x)) == 3 for x in LISTS)


def test_ranking_stats_order():
    _, order = RE.ranking_stats(torch.tensor(X).cuda(), SCOPE, torch.zeros(len(X)), 0)
    got = order.cpu().numpy()
    assert got.dtype == np.int32
    assert np.array_equal(got, np.concatenate(ORDER))


@pytest.mark.parametrize("waves", WAVES)
def test_rank_correlation_reciprocal_rank(waves):
    # list q once per candidate i, the targets one-hot at i: the reciprocal rank is that of candidate i
    scope = [C for C in SCOPE for _ in range(C)]
    score = np.concatenate([x for x in LISTS for _ in range(len(x))])
    targets = np.concatenate([np.eye(len(x), dtype=np.float32).reshape(-1) for x in LISTS])
    stats = _pinned(_lib.lib().rr_rank_correlation_set_waves, waves,
                    lambda: RE.rank_correlation_stats(torch.tensor(score).cuda(), scope, torch.tensor(targets), 0).cpu().numpy())
    want = 1.0 / (1.0 + np.concatenate(RANK).astype(np.float64))
    assert np.array_equal(stats[:, 2], want)                       # one IEEE division of exact integers on both sides


@pytest.mark.parametrize("waves", WAVES)
def test_top1_sets_rank(waves):
    out = _pinned(_lib.lib().rr_top1_sets_set_waves, waves,
                  lambda: UQ.top1_sets(torch.tensor(X).cuda(), SCOPE, torch.zeros(len(X)), 0.5, 0)["rank"].cpu().numpy())
    assert out.dtype == np.int32
    assert np.array_equal(out.astype(np.int64) - 1, np.concatenate(RANK))


def test_mc_sample_stats_mean_rank():
    samples = torch.tensor(np.stack([X, X])).cuda()
    got = UQ.sample_stats(samples, SCOPE, torch.zeros(len(X)), 0)["mean_rank"].cpu().numpy()
    assert got.dtype == np.float32
    assert np.array_equal(got.astype(np.int64) - 1, np.concatenate(RANK)) and np.array_equal(got, np.rint(got))
