#!/usr/bin/env python3
"""Generate tests/golden/task_steps.npz by running the REFERENCE ITSELF (imported unmodified through tools/make_golden.py's
rdkit stub, like tools/make_golden_loss_variants.py): for each of the four older composite task types the reference's
train() forms - mle_gaussian, listnet_gauss, mle_regression, listnet_regression (train_listwise.py:203-209, 223-226,
261-264, restated below) - a preset head output, the targets, the loss and d loss / d output, on the scopes `single`,
`tiny`, `c64`, `ragged` of make_golden's LOSS_SCOPES and one list of 300 candidates.  Writes that one file only.

Fixed seeds: a rerun reproduces every array.

Usage: python tools/make_golden_task_steps.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (installs the rdkit stub and puts the reference on sys.path)

from reactranker.train.loss import MLEloss, ListnetLoss, GaussDisLoss  # noqa: E402

OUT = MG.OUT
CASES = {k: MG.LOSS_SCOPES[k] for k in ("single", "tiny", "c64", "ragged")}
CASES["list300"] = [300]
TASKS = {"mle_gaussian": 2, "listnet_gauss": 2, "mle_regression": 1, "listnet_regression": 1}    # task type -> task_num


def softplus(x):
    return np.log1p(np.exp(x))


def std_targets(rng, scope):
    t = np.concatenate([rng.permutation(c).astype(np.float32) * 0.37 - 0.1 * c + rng.random(1).astype(np.float32)
                        for c in scope])
    return ((t - t.mean()) / (t.std() + 1e-6)).astype(np.float32)


def branch_loss(task, o, scope, t):
    """The loss the reference's train() forms for one batch of task type `task`, restated."""
    if task == "mle_gaussian":
        return MLEloss()(o[:, 0], scope, t, None) + GaussDisLoss()(o[:, 0], o[:, 1], t, None)
    if task == "listnet_gauss":
        return ListnetLoss()(o[:, 0], scope, t, None) + GaussDisLoss()(o[:, 0], o[:, 1], t, None)
    if task == "mle_regression":
        return torch.nn.MSELoss()(o, t) + MLEloss()(o, scope, t, None)
    assert task == "listnet_regression"
    return ListnetLoss()(o, scope, t, None) + torch.nn.MSELoss()(o, t)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    rng = np.random.default_rng(9091)
    out = {}
    for case, scope in CASES.items():
        m = sum(scope)
        out[f"{case}.scope"] = np.asarray(scope, np.int32)
        for task, k in TASKS.items():
            raw = (rng.standard_normal((m, k)) * 1.5).astype(np.float32)
            if k == 2:                                         # variance column positive (GaussDisLoss takes its log)
                raw[:, 1] = softplus(raw[:, 1]) + 1e-3
                o = raw
            else:
                o = raw[:, 0]
            o = np.ascontiguousarray(o, np.float32)
            t = torch.tensor(std_targets(rng, scope))
            ol = torch.tensor(o, requires_grad=True)
            l = branch_loss(task, ol, scope, t)
            g, = torch.autograd.grad(l.sum(), [ol])
            P = f"{case}.{task}."
            out[P + "output"], out[P + "targets"], out[P + "loss"], out[P + "grad"] = o, t.numpy(), l.detach().numpy(), g.numpy()
    path = os.path.join(OUT, "task_steps.npz")
    np.savez_compressed(path, **out)
    print("wrote task_steps.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
