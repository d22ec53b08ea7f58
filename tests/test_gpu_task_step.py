"""Composite task types: per-term normalisers on shards, and rr_task_loss_step_f32 (loss + gradient in one launch).

Reference numbers: tests/golden/loss_variants.npz (`train.<task>.*`, the six newer non-NIG task types on scope
[7, 12, 1, 30], written by tools/make_golden_loss_variants.py) and tests/golden/task_steps.npz (the four older composites
on five scopes, written by tools/make_golden_task_steps.py) - both produced by the reference itself.  Bound everywhere:
1e-5 * (1 + |ref|), the bound tests/test_gpu_loss_variants.py uses for the same vectors."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as Hh

from reactranker_amd import _lib
from reactranker_amd import loss as RL
from reactranker_amd import train_listwise as TL

pytestmark = pytest.mark.gpu

OLD_TASKS = ["mle_gaussian", "listnet_gauss", "mle_regression", "listnet_regression"]
NEW_TASKS = ["mledis_gaussian", "listnetdis_gauss", "listnetdis_lognorm", "listnet_uq", "dirichlet_uq", "regression_exploss"]
FUSED = ["mle_gaussian", "listnet_gauss", "mle_regression", "listnet_regression", "mledis_gaussian", "listnetdis_gauss",
         "listnet_uq", "dirichlet_uq"]
OLD_CASES = ["single", "tiny", "c64", "ragged", "list300"]
# (task, case) of every reference vector; "train" = the loss_variants.npz trainer case
VECTORS = [(t, c) for t in OLD_TASKS for c in OLD_CASES] + [(t, "train") for t in NEW_TASKS]
FUSED_VECTORS = [(t, c) for t, c in VECTORS if t in FUSED]


def close(got, ref, tol=1e-5, what=""):
    got = got.detach().cpu().double().numpy().reshape(-1) if torch.is_tensor(got) else np.asarray(got, np.float64).reshape(-1)
    ref = ref.detach().cpu().double().numpy().reshape(-1) if torch.is_tensor(ref) else np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.max(np.abs(got - ref) / (1 + np.abs(ref))) if got.size else 0
    Hh.record(what, err, tol)
    print(f"{what}: err {err:.3e} (bound {tol:.0e})")
    assert err <= tol, f"{what}: err {err:.3e}"


@pytest.fixture(scope="module")
def G(golden_dir):
    return (np.load(os.path.join(golden_dir, "loss_variants.npz")), np.load(os.path.join(golden_dir, "task_steps.npz")))


def vector(G, task, case):
    """(scope, output, targets, loss, grad, (epoch, epochs, max_coeff)) of one reference vector"""
    V, S = G
    if case == "train":
        epoch, epochs, max_coeff = V["train.args"].tolist()
        P = f"train.{task}."
        return V["train.scope"].tolist(), V[P + "output"], V[P + "targets"], V[P + "loss"], V[P + "grad"], (int(epoch), int(epochs), max_coeff)
    P = f"{case}.{task}."
    return S[f"{case}.scope"].tolist(), S[P + "output"], S[P + "targets"], S[P + "loss"], S[P + "grad"], (0, 1, 1e-4)


def leaf(a):
    return torch.tensor(np.asarray(a, np.float32)).cuda().requires_grad_(True)


@pytest.fixture
def fused_on():
    old = RL.FusedStep.enabled
    RL.FusedStep.enabled = True
    yield
    RL.FusedStep.enabled = old


def run(task, o_np, scope, t_np, args, norm=None, unit=True):
    o = leaf(o_np)
    l = TL.batch_loss(task, o, scope, torch.tensor(t_np), 0, *args, norm=norm)
    if unit:
        RL.backward(l)
    else:
        l.sum().backward()
    return l.detach(), o.grad


# ------------------------------------------------------------------------------------------------ shard identity (check 2)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_term"])
@pytest.mark.parametrize("task,case", VECTORS)
def test_shards_under_global_normalisers_add_up_to_the_reference(task, case, fused, G):
    scope, o, t, ref_loss, ref_grad, args = vector(G, task, case)
    norm = dict(queries=len(scope), cands=int(sum(scope)))
    old = RL.FusedStep.enabled
    RL.FusedStep.enabled = fused
    try:
        for k in range(len(scope) + 1):                     # every split into a prefix and a suffix
            total, grads = 0.0, []
            for lo, hi in ((0, k), (k, len(scope))):
                if hi == lo:                                # an empty part adds nothing and is not evaluated (as in _train)
                    continue
                m0, m1 = int(sum(scope[:lo])), int(sum(scope[:hi]))
                l, g = run(task, o[m0:m1], scope[lo:hi], t[m0:m1], args, norm=norm)
                total = total + float(l.double().sum())
                grads.append(g)
            close(np.float64(total), ref_loss, what=f"{task}.{case}.split{k}.loss")
            close(torch.cat(grads, 0), ref_grad, what=f"{task}.{case}.split{k}.grad")
    finally:
        RL.FusedStep.enabled = old


# ------------------------------------------------------------------------------------------------ the step entry (check 3)
@pytest.mark.parametrize("task,case", FUSED_VECTORS)
def test_step_entry_against_reference_vectors(task, case, G, fused_on):
    scope, o, t, ref_loss, ref_grad, args = vector(G, task, case)
    hits = RL.FusedStep.hits
    l, g = run(task, o, scope, t, args)
    assert RL.FusedStep.hits == hits + 1, "loss.backward(loss) did not take the gradient of the forward launch"
    assert tuple(l.shape) == tuple(np.shape(ref_loss)), (tuple(l.shape), np.shape(ref_loss))
    close(l, ref_loss, what=f"{task}.{case}.loss")
    close(g, ref_grad, what=f"{task}.{case}.grad")
    l2, g2 = run(task, o, scope, t, args)
    assert torch.equal(l, l2) and torch.equal(g, g2), "two runs differ"
    # the per-term path agrees at the same bound, and keeps its shapes
    RL.FusedStep.enabled = False
    hits = RL.FusedStep.hits
    lp, gp = run(task, o, scope, t, args)
    RL.FusedStep.enabled = True
    assert RL.FusedStep.hits == hits, "FusedStep.enabled = False still took a fused launch"
    assert lp.shape == l.shape and gp.shape == g.shape
    close(lp, ref_loss, what=f"{task}.{case}.per_term.loss")
    close(l, lp, what=f"{task}.{case}.fused_vs_per_term.loss")
    close(g, gp, what=f"{task}.{case}.fused_vs_per_term.grad")
    # a non-unit upstream gradient multiplies the stored gradient
    o3 = leaf(o)
    l3 = TL.batch_loss(task, o3, scope, torch.tensor(t), 0, *args)
    hits = RL.FusedStep.hits
    l3.backward(gradient=torch.full_like(l3, 2.5))
    assert RL.FusedStep.hits == hits
    assert torch.equal(o3.grad, g * 2.5)
    # a plain loss.backward() (autograd's own ones) is such a gradient too
    o4 = leaf(o)
    TL.batch_loss(task, o4, scope, torch.tensor(t), 0, *args).sum().backward()
    assert torch.equal(o4.grad, g)


def _output(task, M, seed, cols=None):
    """A well-formed head output for a fused task type: positive variance column / positive scores where the loss needs them."""
    rng = np.random.default_rng(seed)
    sp = lambda x: np.log1p(np.exp(x))                                          # noqa: E731
    k = RL.TASK_STEPS[task][2]
    if task in ("listnet_uq", "dirichlet_uq"):
        return (sp(rng.standard_normal(M)) + 1.0).astype(np.float32)
    raw = rng.standard_normal((M, cols or k)).astype(np.float32)
    if k == 2:
        raw[:, 1] = sp(raw[:, 1]) + 1e-2
    return raw if raw.shape[1] > 1 else raw[:, 0]


def _targets(M, seed):
    return np.random.default_rng(seed).standard_normal(M).astype(np.float32)


@pytest.mark.parametrize("task", ["mle_gaussian", "listnet_gauss"])
def test_columns_the_task_does_not_read_get_exact_zeros(task, fused_on):
    scope = [33, 64, 1, 70, 0, 12]
    M = sum(scope)
    o, t = _output(task, M, 5, cols=4), _targets(M, 6)
    hits = RL.FusedStep.hits
    l, g = run(task, o, scope, t, (0, 1, 1e-4))
    assert RL.FusedStep.hits == hits + 1
    assert g.shape == (M, 4) and torch.count_nonzero(g[:, 2:]) == 0
    l2, g2 = run(task, o[:, :2], scope, t, (0, 1, 1e-4))
    assert torch.equal(l, l2) and torch.equal(g[:, :2], g2)
    assert torch.count_nonzero(g2) > 0


@pytest.mark.parametrize("task", FUSED)
def test_empty_and_one_candidate_queries(task, fused_on):
    args = (1, 3, 0.2)
    scope = [3, 0, 1, 2]
    o, t = _output(task, 6, 9), _targets(6, 10)
    hits = RL.FusedStep.hits
    l, g = run(task, o, scope, t, args)
    assert RL.FusedStep.hits == hits + 1
    assert torch.isfinite(l).all() and torch.isfinite(g).all()
    RL.FusedStep.enabled = False
    lp, gp = run(task, o, scope, t, args)
    RL.FusedStep.enabled = True
    close(l, lp, what=f"{task}.empty_query.loss")
    close(g, gp, what=f"{task}.empty_query.grad")
    # the empty query adds zero and still counts: with it as the step's norm, dropping it changes nothing
    l3, g3 = run(task, o, [3, 1, 2], t, args, norm=dict(queries=4, cands=6))
    close(l3, l, what=f"{task}.empty_query_counts.loss")
    close(g3, g, what=f"{task}.empty_query_counts.grad")
    l1, g1 = run(task, o[:1], [1], t[:1], args)
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all()
    RL.FusedStep.enabled = False
    l1p, g1p = run(task, o[:1], [1], t[:1], args)
    RL.FusedStep.enabled = True
    close(l1, l1p, what=f"{task}.one_candidate.loss")
    close(g1, g1p, what=f"{task}.one_candidate.grad")


@pytest.mark.parametrize("task", FUSED)
def test_strided_output_is_read_in_place(task, fused_on):
    scope = [33, 64, 1, 70, 0, 12]
    M = sum(scope)
    o, t = _output(task, M, 21), _targets(M, 22)
    args = (1, 3, 0.2)
    l, g = run(task, o, scope, t, args)
    wide = torch.zeros(M, 5).cuda()
    if o.ndim == 2:
        wide[:, 1:3] = torch.tensor(o).cuda()
    else:
        wide[:, 2] = torch.tensor(o).cuda()
    wide.requires_grad_(True)
    view = wide[:, 1:3] if o.ndim == 2 else wide[:, 2]
    assert not view.is_contiguous()
    hits = RL.FusedStep.hits
    lw = TL.batch_loss(task, view, scope, torch.tensor(t), 0, *args)
    RL.backward(lw)
    assert RL.FusedStep.hits == hits + 1, "a column slice of a wider tensor did not take the step entry"
    assert torch.equal(lw.detach(), l)
    gw = wide.grad[:, 1:3] if o.ndim == 2 else wide.grad[:, 2]
    assert torch.equal(gw, g)
    rest = wide.grad.clone()
    if o.ndim == 2:
        rest[:, 1:3] = 0
    else:
        rest[:, 2] = 0
    assert torch.count_nonzero(rest) == 0


@pytest.mark.parametrize("task", FUSED)
def test_lists_over_8192_are_unsupported(task, fused_on):
    n = 8193
    o = _output(task, n, 3)
    with pytest.raises(RuntimeError, match="status -4"):
        TL.batch_loss(task, leaf(o), [n], torch.zeros(n), 0, 1, 3, 0.2)
    torch.cuda.synchronize()


def test_an_output_layout_the_entry_does_not_know_takes_the_per_term_path(fused_on):
    scope = [4, 3]
    o = _output("mledis_gaussian", 7, 1)
    hits = RL.FusedStep.hits
    # no gradient wanted: nothing to fuse
    l0 = TL.batch_loss("mledis_gaussian", torch.tensor(o).cuda(), scope, torch.tensor(_targets(7, 2)), 0)
    # a transposed [2, M] storage: unit stride along the rows, not along the columns
    ot = torch.tensor(np.ascontiguousarray(o.T)).cuda().requires_grad_(True)
    l1 = TL.batch_loss("mledis_gaussian", ot.t(), scope, torch.tensor(_targets(7, 2)), 0)
    RL.backward(l1)
    assert RL.FusedStep.hits == hits
    close(l1, l0, what="layout_fallback")


# ------------------------------------------------------------------------------------------------ through the C-ABI
@pytest.mark.parametrize("task", FUSED)
def test_c_abi_terms_and_a_preset_ticket_word(task, G):
    case = "ragged" if task in OLD_TASKS else "train"
    scope, o, t, ref_loss, ref_grad, args = vector(G, task, case)
    list_term, point_term, cols, _ = RL.TASK_STEPS[task]
    coef = RL.annealing_coef(args[2], args[0], args[1]) if task in ("listnet_uq", "dirichlet_uq") else 0.0
    o2 = torch.tensor(o).cuda().reshape(len(t), -1)
    tt = torch.tensor(t).cuda()
    seg, total, max_len = RL._segments(tuple(int(c) for c in scope), str(o2.device))
    Q = len(scope)

    def call(counter):
        dout = torch.full_like(o2, float("nan"))
        terms = torch.full((2,), float("nan"), device="cuda")
        loss = RL.task_loss_step(list_term, point_term, o2, tt, seg, Q, max_len, coef, Q, total, dout, terms=terms,
                                 counter=counter)
        torch.cuda.synchronize()
        return loss, terms, dout

    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    loss, terms, dout = call(zero)
    assert int(zero) == 0, "the ticket word was not left at zero"
    assert float(terms[0] + terms[1]) == float(loss), (terms.tolist(), float(loss))
    if point_term == _lib.RR_POINT_NONE:
        assert float(terms[1]) == 0.0
    close(loss, ref_loss, what=f"{task}.abi.loss")
    close(dout, ref_grad, what=f"{task}.abi.grad")
    preset = torch.full((1,), Q, dtype=torch.int32, device="cuda")      # a word an earlier launch left at a multiple of Q
    loss2, terms2, dout2 = call(preset)
    assert int(preset) == 0
    assert torch.equal(loss2, loss) and torch.equal(terms2, terms) and torch.equal(dout2, dout)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    o2 = torch.ones(4, 1).cuda()
    tt = torch.zeros(4).cuda()
    seg = RL._segments((4,), str(o2.device))[0]
    dout = torch.empty_like(o2)
    with pytest.raises(RuntimeError, match="status -1"):                # both terms NONE
        RL.task_loss_step(_lib.RR_LIST_NONE, _lib.RR_POINT_NONE, o2, tt, seg, 1, 4, 0.0, 1, 4, dout)
    with pytest.raises(RuntimeError, match="status -1"):                # the Gaussian term needs two columns
        RL.task_loss_step(_lib.RR_LIST_MLE, _lib.RR_POINT_GAUSS, o2, tt, seg, 1, 4, 0.0, 1, 4, dout)
    with pytest.raises(RuntimeError, match="status -4"):
        RL.task_loss_step(_lib.RR_LIST_MLE, _lib.RR_POINT_MSE, o2, tt, seg, 1, 8193, 0.0, 1, 4, dout)
