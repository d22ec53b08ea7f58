"""The per-term normalisers of the listwise task types (reactranker_amd.dp.TASK_TERMS), without a GPU.

A task type that sums a per-query mean and a per-candidate mean cannot be weighted by one factor per rank.  The table names
what each term is averaged over; dividing every term by the WHOLE step's count of its own normaliser makes the shards'
losses add up to the unsharded loss and their gradients concatenate to the unsharded gradient.  For the four older
composites the terms are restated in oracle/ref_cpu.py, so that identity is checked here in float64 on the ragged scope of
tests/test_dp_gloo.py split 3 + 2; 1e-12 relative only absorbs the order of summation."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from reactranker_amd import dp
from reactranker_amd import train_listwise as TL

SCOPE = [5, 3, 7, 2, 6]          # ragged lists; shards get 3 and 2 queries
NIG = ["evidential", "mle_evidential", "mledis_evidential", "listnet_evidential"]
OLD_COMPOSITES = ["mle_gaussian", "listnet_gauss", "mle_regression", "listnet_regression"]

# term name of dp.TASK_TERMS -> its restatement in the oracle, on (output [M, k], scope, targets)
ORACLE_TERMS = {
    "ListMLE": lambda o, scope, t: O.listmle_loss(o[:, 0], scope, t),
    "ListNet top-1": lambda o, scope, t: O.listnet_loss(o[:, 0], scope, t),
    "MSE": lambda o, scope, t: O.mse_loss(o[:, 0], t),
    "Gaussian NLL": lambda o, scope, t: O.gauss_nll_loss(o[:, 0], o[:, 1], t),
}


def test_table_covers_exactly_the_supported_task_types():
    assert set(dp.TASK_TERMS) == set(TL.SUPPORTED_TASKS)
    assert len(dp.TASK_TERMS) == len(TL.SUPPORTED_TASKS) == 19
    for task in TL.SUPPORTED_TASKS:
        terms = dp.task_terms(task)
        assert 1 <= len(terms) <= 2, task
        for name, normaliser in terms:
            assert isinstance(name, str) and name
            assert normaliser in ("queries", "cands"), (task, name, normaliser)
    with pytest.raises(ValueError, match="mle_dirichlet"):
        dp.task_terms("mle_dirichlet")


def test_single_normaliser_task_types_agree_with_the_weight_table():
    # the five task types the one-weight path serves: their only term's normaliser is the one loss_weight uses
    for task in ("mle", "evidential_ranking", "listnet", "regression", "gauss_regression"):
        (_, normaliser), = dp.task_terms(task)
        assert normaliser == {"mle": "queries", "listnet": "cands"}[dp._KIND[task]], task
        w = dp.loss_weight(dp._KIND[task], 3, 5, 15, 23)
        assert dp.term_scales(task, SCOPE[:3], dict(queries=5, cands=23)) == [w]


@pytest.mark.parametrize("task", NIG)
def test_cross_step_task_types_are_refused_with_a_reason(task):
    with pytest.raises(ValueError, match=task) as e:
        dp.require_shardable(task)
    assert "target" in str(e.value) and "one process" in str(e.value)
    # batch_loss refuses a shard's norm for them before it touches the output (no GPU needed to get here)
    with pytest.raises(ValueError, match=task):
        TL.batch_loss(task, None, SCOPE, None, None, norm=dict(queries=5, cands=23))


def test_every_other_task_type_is_shardable():
    for task in TL.SUPPORTED_TASKS:
        if task not in NIG:
            dp.require_shardable(task)


def _loss(task, out, scope, targets, norm):
    scales = dp.term_scales(task, scope, norm)
    total = 0.0
    for (name, _), f in zip(dp.task_terms(task), scales):
        total = total + ORACLE_TERMS[name](out, scope, targets).sum() * f
    return total


@pytest.mark.parametrize("task", OLD_COMPOSITES)
def test_shards_under_global_normalisers_add_up_to_the_unsharded_step(task):
    rng = np.random.default_rng(17)
    M = sum(SCOPE)
    out_np = rng.standard_normal((M, 2))
    out_np[:, 1] = np.log1p(np.exp(out_np[:, 1])) + 0.1          # a positive variance column
    t = torch.tensor(rng.standard_normal(M), dtype=torch.float64)
    norm = dict(queries=len(SCOPE), cands=M)
    assert dp.term_scales(task, SCOPE, norm) == [1.0] * len(dp.task_terms(task))

    full_out = torch.tensor(out_np, dtype=torch.float64, requires_grad=True)
    full = _loss(task, full_out, SCOPE, t, norm)
    full_grad, = torch.autograd.grad(full, full_out)
    full = full.detach()

    losses, grads = [], []
    for rank in range(2):
        lo, hi = dp.shard_queries(len(SCOPE), rank, 2)
        assert hi - lo == (3, 2)[rank]
        m0, m1 = sum(SCOPE[:lo]), sum(SCOPE[:hi])
        o = torch.tensor(out_np[m0:m1], dtype=torch.float64, requires_grad=True)
        l = _loss(task, o, SCOPE[lo:hi], t[m0:m1], norm)
        losses.append(l.detach())
        grads.append(torch.autograd.grad(l, o)[0])
    got, got_grad = sum(losses), torch.cat(grads, 0)
    assert abs(float(got - full)) <= 1e-12 * abs(float(full)), (task, float(got), float(full))
    rel = float((got_grad - full_grad).abs().max() / full_grad.abs().max())
    assert rel <= 1e-12, (task, rel)
    # the local normalisers do NOT add up on ragged shards: the identity above is the table's doing
    local = sum(_loss(task, torch.tensor(out_np[a:b], dtype=torch.float64), s, t[a:b], dict(queries=len(s), cands=b - a))
                for s, a, b in ((SCOPE[:3], 0, 15), (SCOPE[3:], 15, 23)))
    assert abs(float(local / 2 - full)) > 1e-6 * abs(float(full))
