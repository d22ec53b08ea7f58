"""GPU parity of the reference trainer's remaining losses (MLEDisLoss, Listnet_For_Gauss, Listnetlognorm,
Listnet_For_evidential, Listnet_with_uq, Dirichlet_uq, evidential_loss_new, Lognorm, the regression_exploss expression) and
of the task types built on them: against vectors produced by the reference itself (tests/golden/loss_variants.npz, written
by tools/make_golden_loss_variants.py), at 1e-5 * (1 + |ref|) like tests/test_gpu_losses.py."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import loss_variants_ref as R

from reactranker_amd import featurization, synth
from reactranker_amd import loss as RL
from reactranker_amd import train_listwise as TL
from reactranker_amd import train_utils as TU
from reactranker_amd.base_model import build_model

pytestmark = pytest.mark.gpu
CASES = ["single", "tiny", "c32", "c64", "ragged", "long"]
NEW_TASKS = ["mledis_gaussian", "listnetdis_gauss", "listnetdis_lognorm", "listnet_uq", "evidential", "mle_evidential",
             "mledis_evidential", "listnet_evidential", "dirichlet_uq", "regression_exploss"]


def close(got, ref, tol=1e-5, what=""):
    got = got.detach().cpu().double().numpy().reshape(-1) if torch.is_tensor(got) else np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.max(np.abs(got - ref) / (1 + np.abs(ref))) if got.size else 0
    Hh.record(what, err, tol)
    assert err <= tol, f"{what}: err {err:.3e}"


@pytest.fixture(scope="module")
def V(golden_dir):
    return np.load(os.path.join(golden_dir, "loss_variants.npz"))


def leaf(a):
    return torch.tensor(np.asarray(a, np.float32)).cuda().requires_grad_(True)


@pytest.mark.parametrize("name", CASES)
def test_losses_against_reference_vectors(name, V):
    P = name + "."
    scope = V[P + "scope"].tolist()
    t = torch.tensor(V[P + "targets"])
    uq = tuple(V["uq_args"].tolist())
    uq = (uq[0], int(uq[1]), int(uq[2]))

    def check(loss, shape, key, leaves, suffixes):
        assert tuple(loss.shape) == shape, (key, tuple(loss.shape))
        gs = torch.autograd.grad(loss.sum(), leaves)
        close(loss, V[P + key], what=key)
        for g, sfx in zip(gs, suffixes):
            close(g, V[P + key + sfx], what=key + sfx)

    for key, cls, a0 in (("mledis", RL.MLEDisLoss, "score"), ("lgauss", RL.Listnet_For_Gauss, "score"),
                         ("llognorm", RL.Listnetlognorm, "pos")):
        s, v = leaf(V[P + a0]), leaf(V[P + "var"])
        check(cls()(s[:, None], v[:, None], scope, t, 0), (1,), key, [s, v], ["_gs", "_gv"])

    s, v, a = leaf(V[P + "score"]), leaf(V[P + "nu"]), leaf(V[P + "alpha"])
    check(RL.Listnet_For_evidential()(s[:, None], v[:, None], a[:, None], scope, t, 0), (1,), "levid", [s, v, a],
          ["_gs", "_gv", "_ga"])

    s = leaf(V[P + "pos"])
    check(RL.Listnet_with_uq()(s, scope, t, *uq, 0), (1,), "uq", [s], ["_g"])
    a = leaf(V[P + "conc"])
    check(RL.Dirichlet_uq()(a, scope, t, *uq, 0), (1,), "dir", [a], ["_g"])

    lam = float(V["nig_lam"])
    for key, col in (("nig", False), ("nigx", True)):
        ps = [leaf(V[P + k]) for k in ("mu", "nu", "alpha", "beta")]
        args = [p[:, None] for p in ps] if col else ps
        check(RL.evidential_loss_new(*args, t, 0, lam=lam), (), key, ps, ["_gmu", "_gv", "_ga", "_gb"])

    s, v = leaf(V[P + "pos"]), leaf(V[P + "var"])
    check(RL.Lognorm()(s, v, t, 0), (), "lognorm", [s, v], ["_gs", "_gv"])
    s = leaf(V[P + "expmse_x"])
    check(RL.ExpMSELoss()(s, t), (), "expmse", [s], ["_g"])


def _nig_inputs(M, seed):
    rng = np.random.default_rng(seed)
    sp = lambda x: np.log1p(np.exp(x))                                          # noqa: E731
    mu = rng.standard_normal(M).astype(np.float32)
    v = (sp(rng.standard_normal(M)) + 1e-6).astype(np.float32)
    a = (sp(rng.standard_normal(M)) + 1 + 1e-6).astype(np.float32)
    b = (sp(rng.standard_normal(M)) + 1e-6).astype(np.float32)
    t = rng.standard_normal(M).astype(np.float32)
    return mu, v, a, b, t


def test_evidential_cross_form_at_4096_against_float64():
    M = 4096                                                  # 64 x 64: the size of a 64-query, 64-candidate step
    mu, v, a, b, t = _nig_inputs(M, 11)
    ps = [leaf(x[:, None]) for x in (mu, v, a, b)]
    l = RL.evidential_loss_new(*ps, torch.tensor(t), 0, lam=0.1)
    gs = torch.autograd.grad(l, ps)
    ref = R.nig_cross(mu, v, a, b, t, 0.1)
    close(l, ref[0], what="nigx4096")
    for g, r, nm in zip(gs, ref[1:], ("mu", "v", "alpha", "beta")):
        close(g, r, what="nigx4096_g" + nm)


def test_device_digamma_against_torch():
    x = torch.linspace(1.0, 50.0, 2001, device="cuda")
    got = RL.digamma(x)
    ref = torch.digamma(x.double())
    close(got, ref.cpu().numpy(), tol=2e-6, what="digamma")


def _task_output(task, M, seed):
    """A well-formed [M, task_num] output of each task type's head."""
    k = 4 if "evidential" in task else (2 if "dis_" in task else 1)
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((M, k)).astype(np.float32)
    sp = lambda x: np.log1p(np.exp(x))                                          # noqa: E731
    if k == 4:
        raw[:, 1] = sp(raw[:, 1]) + 1e-6
        raw[:, 2] = sp(raw[:, 2]) + 1 + 1e-6
        raw[:, 3] = sp(raw[:, 3]) + 1e-6
        return raw
    if k == 2:
        return sp(raw) + 1e-6
    if task == "regression_exploss":
        return raw[:, 0] * 0.5
    return sp(raw[:, 0]) + 1.0


@pytest.mark.parametrize("task", NEW_TASKS)
def test_strided_columns_and_repeat_runs_give_identical_bits(task):
    scope = [33, 64, 1, 70, 0, 12]
    M = sum(scope)
    o_np = _task_output(task, M, 5)
    t = torch.tensor(np.random.default_rng(6).standard_normal(M).astype(np.float32))

    def run():
        o = torch.tensor(o_np).cuda().requires_grad_(True)
        l = TL.batch_loss(task, o, scope, t, 0, 1, 3, 0.2)
        g, = torch.autograd.grad(l.sum(), o)
        return l.detach(), g

    l1, g1 = run()
    l2, g2 = run()
    assert torch.equal(l1, l2) and torch.equal(g1, g2), "two runs differ"
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all()
    if o_np.ndim == 2:
        # the kernels read the [M, k] output's columns in place: the same bits as from contiguous copies
        o = torch.tensor(o_np).cuda()
        cols = [o[:, k] for k in range(o.shape[1])]
        copies = [c.contiguous() for c in cols]
        for kind, n in (("mledis", 2), ("listnet_gauss", 2), ("listnet_lognorm", 2), ("listnet_evidential", 3)):
            if n > o.shape[1]:
                continue
            seg = RL._segments(tuple(scope), str(o.device))[0]
            a = RL._ListwiseVariantFn.apply(kind, 0.0, t.cuda(), seg, len(scope), max(scope), *cols[:n])
            b = RL._ListwiseVariantFn.apply(kind, 0.0, t.cuda(), seg, len(scope), max(scope), *copies[:n])
            torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True, msg=kind)
        if o.shape[1] == 4:
            a = RL.evidential_loss_new(*[c[:, None] for c in cols], t, 0)
            b = RL.evidential_loss_new(*[c[:, None] for c in copies], t, 0)
            torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def test_empty_and_one_candidate_queries():
    rng = np.random.default_rng(9)
    s_np = (np.log1p(np.exp(rng.standard_normal(6))) + 1.0).astype(np.float32)
    v_np = (np.log1p(np.exp(rng.standard_normal(6))) + 0.1).astype(np.float32)
    t = torch.tensor(rng.standard_normal(6).astype(np.float32))
    losses = [lambda s, v, sc, tt: RL.MLEDisLoss()(s, v, sc, tt, 0), lambda s, v, sc, tt: RL.Listnet_For_Gauss()(s, v, sc, tt, 0),
              lambda s, v, sc, tt: RL.Listnetlognorm()(s, v, sc, tt, 0),
              lambda s, v, sc, tt: RL.Listnet_For_evidential()(s, v, v, sc, tt, 0),
              lambda s, v, sc, tt: RL.Listnet_with_uq()(s, sc, tt, 0.5, 1, 3, 0),
              lambda s, v, sc, tt: RL.Dirichlet_uq()(s, sc, tt, 0.5, 1, 3, 0)]
    for f in losses:
        s, v = leaf(s_np), leaf(v_np)
        with_empty = f(s, v, [3, 0, 1, 2], t)          # an empty query adds 0 and counts in Q
        g1 = torch.autograd.grad(with_empty.sum(), [s])[0]
        s2, v2 = leaf(s_np), leaf(v_np)
        without = f(s2, v2, [3, 1, 2], t)
        g2 = torch.autograd.grad(without.sum(), [s2])[0]
        assert torch.isfinite(with_empty).all() and torch.isfinite(g1).all()
        close(with_empty * 4, without.detach().cpu().numpy() * 3, what="empty_query")
        close(g1 * 4, g2.cpu().numpy() * 3, what="empty_query_g")
        s1 = leaf(s_np[:1])
        one = f(s1, leaf(v_np[:1]), [1], t[:1])
        g, = torch.autograd.grad(one.sum(), [s1])
        assert torch.isfinite(one).all() and torch.isfinite(g).all()


def test_lists_over_8192_are_unsupported():
    n = 8193
    s = torch.rand(n, device="cuda") + 1.0
    t = torch.zeros(n)
    for f in (lambda: RL.MLEDisLoss()(s, s, [n], t, 0), lambda: RL.Listnet_For_Gauss()(s, s, [n], t, 0),
              lambda: RL.Listnetlognorm()(s, s, [n], t, 0), lambda: RL.Listnet_For_evidential()(s, s, s, [n], t, 0),
              lambda: RL.Listnet_with_uq()(s, [n], t, 0.5, 1, 3, 0), lambda: RL.Dirichlet_uq()(s, [n], t, 0.5, 1, 3, 0)):
        with pytest.raises(RuntimeError, match="status -4"):
            f()


def test_evidential_shapes_other_than_the_two_forms_are_refused():
    x = torch.ones(5, 1, device="cuda") + 1
    with pytest.raises(ValueError):
        RL.evidential_loss_new(x, x, x, x, torch.zeros(5, 1), 0)
    with pytest.raises(ValueError):
        RL.evidential_loss_new(x[:, 0], x[:, 0], x[:, 0], x, torch.zeros(5), 0)
    with pytest.raises(ValueError):
        RL.evidential_loss_new(x[:4], x[:4], x[:4], x[:4], torch.zeros(5), 0)


@pytest.mark.parametrize("task", NEW_TASKS)
def test_batch_loss_matches_the_reference_branch(task, V):
    P = f"train.{task}."
    scope = V["train.scope"].tolist()
    epoch, epochs, max_coeff = V["train.args"].tolist()
    o = leaf(V[P + "output"])
    l = TL.batch_loss(task, o, scope, torch.tensor(V[P + "targets"]), 0, int(epoch), int(epochs), max_coeff)
    g, = torch.autograd.grad(l.sum(), o)
    close(l, V[P + "loss"], what=task)
    close(g, V[P + "grad"], what=task + "_g")


HEADS = {  # task type -> build_model arguments of the head it trains (as examples/train_synthetic.py picks them)
    "mledis_gaussian": dict(task_num=2, ffn_last_layer="with_softplus"),
    "listnetdis_gauss": dict(task_num=2, ffn_last_layer="with_softplus"),
    "listnetdis_lognorm": dict(task_num=2, ffn_last_layer="with_softplus", task_type="listnetdis_lognorm"),
    "listnet_uq": dict(task_num=1, ffn_last_layer="with_uncertainty", task_type="listnet"),
    "dirichlet_uq": dict(task_num=1, ffn_last_layer="with_uncertainty", task_type="listnet"),
    "regression_exploss": dict(task_num=1, ffn_last_layer="with_softplus"),
    "evidential": dict(task_num=4, ffn_last_layer="with_softplus"),
    "mle_evidential": dict(task_num=4, ffn_last_layer="with_softplus"),
    "mledis_evidential": dict(task_num=4, ffn_last_layer="with_softplus"),
    "listnet_evidential": dict(task_num=4, ffn_last_layer="with_softplus"),
}


def _batches(seed0, n, nq, nc):
    out = []
    for i in range(n):
        qb = synth.make_queries(seed0 + i, nq, nc, atoms_lo=6, atoms_hi=12)
        tg = np.array([s.edges.shape[0] for s in qb.p_specs], np.float32) * 0.3 + qb.add_features[:, 0]
        tg = ((tg - tg.mean()) / (tg.std() + 1e-6) + 1e-3 * np.arange(len(tg), dtype=np.float32)).astype(np.float32)
        out.append(dict(r=featurization.BatchMolGraph(qb.r_specs, K=4), p=featurization.BatchMolGraph(qb.p_specs, K=4),
                        scope=qb.scope, targets=torch.tensor(tg), add=qb.add_features))
    return out


@pytest.mark.parametrize("task", NEW_TASKS)
def test_two_epoch_training_runs(task, tmp_path):
    torch.manual_seed(0)
    model = build_model(hidden_size=32, mpnn_depth=2, mpnn_diff_depth=2, ffn_depth=2, use_bias=True, dropout=0.0,
                        add_features_dim=1, **HEADS[task])
    model = model.cuda()
    opt = TU.build_optimizer(model)
    sch = TU.build_lr_scheduler(opt, warmup_epochs=1, total_epochs=2, train_data_size=3 * 4, batch_size=4, init_lr=1e-4,
                                max_lr=5e-4, final_lr=1e-4)
    path = str(tmp_path / "ck" / "model.pt")
    hist = TL.train(model, sch, _batches(100, 3, 4, 9), _batches(200, 1, 4, 9), path, opt, 2, seed=3, gpu=0, task_type=task)
    assert len(hist) == 2
    assert all(np.isfinite(h["train_loss"]) for h in hist), hist
    assert hist[0]["checkpoint"] and os.path.exists(path)
