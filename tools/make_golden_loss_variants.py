#!/usr/bin/env python3
"""Generate tests/golden/loss_variants.npz by running the REFERENCE ITSELF, in the manner of tools/make_golden.py (whose
rdkit stub and reference import it reuses; the reference's modules are imported unmodified).  Writes that one file only.

  loss cases:    MLEDisLoss, Listnet_For_Gauss, Listnetlognorm, Listnet_For_evidential, Listnet_with_uq, Dirichlet_uq,
                 evidential_loss_new (elementwise and M x M cross form), Lognorm, and the regression_exploss expression,
                 on make_golden's LOSS_SCOPES shapes: value and the gradient with respect to every input
  trainer cases: for each task type the reference's train() forms with these losses, a preset [M, task_num] output, its
                 loss and d loss / d output (the branch expressions of train_listwise.py:196-279, restated below)

Fixed seeds: a rerun reproduces every array.

Usage: python tools/make_golden_loss_variants.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (installs the rdkit stub and puts the reference on sys.path)

from reactranker.train.loss import (MLEloss, GaussDisLoss, MLEDisLoss, Listnet_For_Gauss, Listnetlognorm,  # noqa: E402
                                    Listnet_For_evidential, Listnet_with_uq, Dirichlet_uq, evidential_loss_new, Lognorm)

OUT = MG.OUT
UQ_ARGS = (0.5, 2, 5)                 # max_coeff, epoch, epochs: annealing coefficient 0.5 * (2 / 4) ** 3
NIG_LAM = 0.3
TRAIN_SCOPE = [7, 12, 1, 30]
TRAIN_ARGS = (1, 3, 0.2)              # epoch, epochs, max_coeff
TRAIN_TASKS = {                       # task type -> task_num of the head it trains
    "mledis_gaussian": 2, "listnetdis_gauss": 2, "listnetdis_lognorm": 2, "listnet_uq": 1, "evidential": 4,
    "mle_evidential": 4, "mledis_evidential": 4, "listnet_evidential": 4, "dirichlet_uq": 1, "regression_exploss": 1,
}


def softplus(x):
    return np.log1p(np.exp(x))


def std_targets(rng, scope):
    t = np.concatenate([rng.permutation(c).astype(np.float32) * 0.37 - 0.1 * c + rng.random(1).astype(np.float32)
                        for c in scope])
    return ((t - t.mean()) / (t.std() + 1e-6)).astype(np.float32)


def leaf(a):
    return torch.tensor(np.asarray(a, np.float32), requires_grad=True)


def grads(loss, leaves):
    return [g.numpy() for g in torch.autograd.grad(loss.sum(), leaves)]


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):          # Lognorm prints its value
        return fn(*a, **k)


def gen_loss_cases(out):
    rng = np.random.default_rng(4242)
    for name, scope in MG.LOSS_SCOPES.items():
        m = sum(scope)
        P = name + "."
        arrays = dict(
            scope=np.asarray(scope, np.int32), targets=std_targets(rng, scope),
            score=(rng.standard_normal(m) * 1.5).astype(np.float32),
            var=(softplus(rng.standard_normal(m)) + 1e-6).astype(np.float32),
            pos=(softplus(rng.standard_normal(m)) + 0.1).astype(np.float32),
            conc=(softplus(rng.standard_normal(m)) + 1.0 + 1e-6).astype(np.float32),
            mu=rng.standard_normal(m).astype(np.float32),
            nu=(softplus(rng.standard_normal(m)) + 1e-6).astype(np.float32),
            alpha=(softplus(rng.standard_normal(m)) + 1.0 + 1e-6).astype(np.float32),
            beta=(softplus(rng.standard_normal(m)) + 1e-6).astype(np.float32),
        )
        for k, v in arrays.items():
            out[P + k] = v
        t = torch.tensor(arrays["targets"])

        s, v = leaf(arrays["score"]), leaf(arrays["var"])
        l = MLEDisLoss()(s[:, None], v[:, None], scope, t, None)
        out[P + "mledis"], (out[P + "mledis_gs"], out[P + "mledis_gv"]) = l.detach().numpy(), grads(l, [s, v])

        s, v = leaf(arrays["score"]), leaf(arrays["var"])
        l = Listnet_For_Gauss()(s[:, None], v[:, None], scope, t, None)
        out[P + "lgauss"], (out[P + "lgauss_gs"], out[P + "lgauss_gv"]) = l.detach().numpy(), grads(l, [s, v])

        s, v = leaf(arrays["pos"]), leaf(arrays["var"])
        l = Listnetlognorm()(s[:, None], v[:, None], scope, t, None)
        out[P + "llognorm"], (out[P + "llognorm_gs"], out[P + "llognorm_gv"]) = l.detach().numpy(), grads(l, [s, v])

        s, v, a = leaf(arrays["score"]), leaf(arrays["nu"]), leaf(arrays["alpha"])
        l = Listnet_For_evidential()(s[:, None], v[:, None], a[:, None], scope, t, None)
        out[P + "levid"] = l.detach().numpy()
        out[P + "levid_gs"], out[P + "levid_gv"], out[P + "levid_ga"] = grads(l, [s, v, a])

        s = leaf(arrays["pos"])
        l = Listnet_with_uq()(s, scope, t, *UQ_ARGS, None)
        out[P + "uq"], (out[P + "uq_g"],) = l.detach().numpy(), grads(l, [s])

        a = leaf(arrays["conc"])
        l = Dirichlet_uq()(a, scope, t, *UQ_ARGS, None)
        out[P + "dir"], (out[P + "dir_g"],) = l.detach().numpy(), grads(l, [a])

        for key, col in (("nig", False), ("nigx", True)):
            ps = [leaf(arrays[k]) for k in ("mu", "nu", "alpha", "beta")]
            args = [p[:, None] for p in ps] if col else ps
            l = evidential_loss_new(*args, t, None, lam=NIG_LAM)
            out[P + key] = l.detach().numpy()
            out[P + key + "_gmu"], out[P + key + "_gv"], out[P + key + "_ga"], out[P + key + "_gb"] = grads(l, ps)

        s, v = leaf(arrays["pos"]), leaf(arrays["var"])
        l = quiet(Lognorm(), s, v, t, None)
        out[P + "lognorm"], (out[P + "lognorm_gs"], out[P + "lognorm_gv"]) = l.detach().numpy(), grads(l, [s, v])

        s = leaf(arrays["score"] * 0.5)
        l = torch.mean((torch.exp(t) - torch.exp(s)) ** 2)
        out[P + "expmse_x"] = arrays["score"] * 0.5
        out[P + "expmse"], (out[P + "expmse_g"],) = l.detach().numpy(), grads(l, [s])
    out["uq_args"] = np.asarray(UQ_ARGS, np.float64)
    out["nig_lam"] = np.float64(NIG_LAM)


def branch_loss(task, o, scope, t, epoch, epochs, max_coeff):
    """The loss the reference's train() forms for one batch of task type `task` (train_listwise.py:196-279), restated."""
    if task == "mledis_gaussian":
        return MLEDisLoss()(o[:, 0::2], torch.exp(o[:, 1::2]), scope, t, None) + GaussDisLoss()(o[:, 0], o[:, 1], t, None)
    if task == "listnetdis_gauss":
        return Listnet_For_Gauss()(o[:, 0::2], o[:, 1::2], scope, t, None) + GaussDisLoss()(o[:, 0], o[:, 1], t, None)
    if task == "listnetdis_lognorm":
        return quiet(Lognorm(), o[:, 0], o[:, 1], t, None)
    if task == "listnet_uq":
        return Listnet_with_uq()(o, scope, t, max_coeff, epoch, epochs, None)
    if task == "dirichlet_uq":
        return Dirichlet_uq()(o, scope, t, max_coeff, epoch, epochs, None)
    if task == "regression_exploss":
        return torch.mean((torch.exp(t) - torch.exp(o)) ** 2)
    mu, lam, alpha, beta = o[:, 0::4], o[:, 1::4], o[:, 2::4], o[:, 3::4]
    evid = evidential_loss_new(mu, lam, alpha, beta, t, None, lam=0.2 if task == "mle_evidential" else 0.1)
    if task == "evidential":
        return evid
    if task == "mle_evidential":
        return MLEloss()(o[:, 0], scope, t, None) + evid
    variance = beta / (lam * (alpha - 1))
    if task == "mledis_evidential":
        return MLEDisLoss()(mu, variance, scope, t, None) + evid
    assert task == "listnet_evidential"
    return Listnet_For_Gauss()(mu, variance, scope, t, None) + evid


def gen_trainer_cases(out):
    rng = np.random.default_rng(777)
    epoch, epochs, max_coeff = TRAIN_ARGS
    m = sum(TRAIN_SCOPE)
    out["train.scope"] = np.asarray(TRAIN_SCOPE, np.int32)
    out["train.args"] = np.asarray(TRAIN_ARGS, np.float64)
    for task, k in TRAIN_TASKS.items():
        raw = rng.standard_normal((m, k)).astype(np.float32)
        if k == 4:                                             # the evidential_with_softplus head: v, beta > 0, alpha > 1
            o = raw.copy()
            o[:, 1] = softplus(raw[:, 1]) + 1e-6
            o[:, 2] = softplus(raw[:, 2]) + 1.0 + 1e-6
            o[:, 3] = softplus(raw[:, 3]) + 1e-6
        elif task == "listnetdis_lognorm":                     # both columns positive
            o = softplus(raw) + 1e-6
        elif k == 2:                                           # variance column positive (GaussDisLoss takes its log)
            o = raw.copy()
            o[:, 1] = softplus(raw[:, 1])
        elif task == "regression_exploss":
            o = (raw[:, 0] * 0.5)
        else:                                                  # listnet_with_uncertainty head: softplus + 1
            o = softplus(raw[:, 0]) + 1.0
        o = np.ascontiguousarray(o, np.float32)
        t = torch.tensor(std_targets(rng, TRAIN_SCOPE))
        ol = leaf(o)
        l = branch_loss(task, ol, TRAIN_SCOPE, t, epoch, epochs, max_coeff)
        g, = grads(l, [ol])
        P = f"train.{task}."
        out[P + "output"], out[P + "targets"], out[P + "loss"], out[P + "grad"] = o, t.numpy(), l.detach().numpy(), g


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(4)
    out = {}
    gen_loss_cases(out)
    gen_trainer_cases(out)
    np.savez_compressed(os.path.join(OUT, "loss_variants.npz"), **out)
    print("wrote loss_variants.npz with", len(out), "arrays")
