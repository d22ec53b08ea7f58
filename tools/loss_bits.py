"""Every output of the list losses, the pointwise losses and the small ops of csrc/loss.hip, csrc/pairwise.hip and
csrc/task_loss.hip that tools/window_loss_bits.py and tools/per_query_bits.py do not reach, as one .npz - to be run with two
builds of the library (RR_LIB_PATH) on one MI355X and compared byte for byte:
    python tools/loss_bits.py --out A.npz
    python tools/loss_bits.py --compare A.npz B.npz    (prints the array count and the names that differ; status 1 on any)
Per seed, a ragged window with list lengths 0, 1, 2, 63, 64, 65, 300, 1000, 8192 and tied targets: loss and every gradient
column of the nine list losses, from contiguous inputs and from columns of an [M, 4] tensor, with the fused step on and off,
for `backward(loss)`, a plain `loss.backward()` and an upstream gradient of 0.37; their forward and step entry points at the
C ABI with a NaN-filled `partial` and the ticket word.  Then the four pointwise losses and the elementwise NIG loss at n = 0
(forward), 1, 255, 257, 262149, the cross NIG loss at M = 1, 63, 65, 1025, digamma, LogCumsumExp at n = 1, 64, 65, 8192,
pair_softmax_mse at B = 1, 257, 262149, the pair accuracy at B = 1, 1000, and every entry of TASK_STEPS on the window
without its 8192 list."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import eval as RE  # noqa: E402
from reactranker_amd import loss as RL  # noqa: E402
from reactranker_amd._lib import check, lib, ptr, stream  # noqa: E402
from tools.window_loss_bits import compare  # noqa: E402

SEEDS = (0, 1)
LENGTHS = (0, 1, 2, 63, 64, 65, 300, 1000, 8192)
POINT_N = (0, 1, 255, 257, 262149)
OUT = {}


def put(name, x):
    assert name not in OUT, name
    OUT[name] = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def window(seed, lengths):
    """scope, targets with ties inside every longer list, and four input columns: a score and three positive ones"""
    rng = np.random.default_rng(seed)
    scope = [int(c) for c in rng.permutation(lengths)]
    M = sum(scope)
    targets = np.round(rng.standard_normal(M) * 2).astype(np.float32) / 2
    score = rng.standard_normal(M).astype(np.float32)
    pos = [(np.log1p(np.exp(rng.standard_normal(M))) + a).astype(np.float32) for a in (1.0, 0.25, 1.5)]
    return scope, targets, score, pos


# name -> (loss(columns, scope, targets), the columns it reads of (score, pos0, pos1, pos2), C-ABI stem, takes a coefficient)
LIST_LOSSES = {
    "listmle": (lambda c, sc, t: RL.MLEloss()(c[0], sc, t, 0), (0,), "listmle", False),
    "listnet": (lambda c, sc, t: RL.ListnetLoss()(c[0], sc, t, 0), (0,), "listnet", False),
    "uc_listwise": (lambda c, sc, t: RL.evidential_ranking()(c, sc, t, gpu=0), (0, 2), "evidential_ranking", False),
    "mledis": (lambda c, sc, t: RL.MLEDisLoss()(c[0], c[1], sc, t, 0), (0, 2), "mledis", False),
    "listnet_gauss": (lambda c, sc, t: RL.Listnet_For_Gauss()(c[0], c[1], sc, t, 0), (0, 2), "listnet_gauss", False),
    "listnet_lognorm": (lambda c, sc, t: RL.Listnetlognorm()(c[0], c[1], sc, t, 0), (1, 2), "listnet_lognorm", False),
    "listnet_evidential": (lambda c, sc, t: RL.Listnet_For_evidential()(c[0], c[1], c[2], sc, t, 0), (0, 2, 3),
                           "listnet_evidential", False),
    "listnet_uq": (lambda c, sc, t: RL.Listnet_with_uq()(c[0], sc, t, 0.01, 2, 4, 0), (1,), "listnet_uq", True),
    "dirichlet_uq": (lambda c, sc, t: RL.Dirichlet_uq()(c[0], sc, t, 0.01, 2, 4, 0), (1,), "dirichlet_uq", True),
}


def list_outputs(seed):
    scope, targets, score, pos = window(seed, LENGTHS)
    t = torch.tensor(targets)
    table = np.stack([score] + pos, 1)
    for kind, (fn, cols, stem, has_coef) in LIST_LOSSES.items():
        data = np.ascontiguousarray(table[:, list(cols)])
        for layout in ("flat", "column"):
            for fused in (True, False):
                for up in ("unit", "ones", "0.37"):
                    RL.FusedStep.enabled = fused
                    if layout == "flat":              # contiguous vectors (UC-Listwise: a contiguous [M, 2])
                        if kind == "uc_listwise":
                            leaves = [torch.tensor(data).cuda().requires_grad_(True)]
                            x = leaves[0]
                        else:
                            leaves = [torch.tensor(data[:, k].copy()).cuda().requires_grad_(True) for k in range(len(cols))]
                            x = leaves
                    else:                             # columns of an [M, 4] tensor
                        wide = np.zeros((len(score), 4), np.float32)
                        wide[:, :len(cols)] = data
                        leaves = [torch.tensor(wide).cuda().requires_grad_(True)]
                        x = leaves[0][:, :2] if kind == "uc_listwise" else [leaves[0][:, k] for k in range(len(cols))]
                    loss = fn(x, scope, t)
                    if up == "unit":
                        RL.backward(loss)
                    elif up == "ones":
                        loss.backward()
                    else:
                        (loss * 0.37).backward()
                    tag = f"s{seed}/{kind}/{layout}/fused{int(fused)}/{up}"
                    put(tag + "/loss", loss)
                    for k, leaf in enumerate(leaves):
                        put(f"{tag}/grad{k}", leaf.grad)
        RL.FusedStep.enabled = True
        # the C ABI with the caller's partial buffer: the forward of all nine, the step of the three that have one
        Q, L, M = len(scope), max(scope), len(score)
        seg = torch.tensor(np.concatenate([[0], np.cumsum(scope)]).astype(np.int32)).cuda()
        tg = t.cuda()
        x = torch.tensor(data).cuda()
        n_in = len(cols)
        if kind == "uc_listwise":
            ins = [ptr(x[:, 0]), ptr(x[:, 1]), n_in]
        else:
            ins = [a for k in range(n_in) for a in (ptr(x[:, k]), n_in)]
        head = ins + [ptr(tg), ptr(seg), Q, L] + ([M] if kind == "listnet" else []) + ([0.00125] if has_coef else [])
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        for step in ((False, True) if kind in ("listmle", "listnet", "uc_listwise") else (False,)):
            loss = torch.full((1,), float("nan"), device="cuda")
            part = torch.full((Q,), float("nan"), device="cuda")
            d = torch.zeros(M, n_in, device="cuda")
            if step:
                name = f"rr_{stem}_step_f32"
                tail = [ptr(loss), ptr(part), ptr(counter)] + [ptr(d[:, k]) for k in range(n_in)] + [n_in]
            else:
                name, tail = f"rr_{stem}_fwd_f32", [ptr(loss), ptr(part)]
            check(getattr(lib(), name)(*head, *tail, stream()), name)
            for what, v in (("loss", loss), ("partial", part.view(torch.int32)), ("d", d), ("counter", counter)):
                put(f"s{seed}/abi/{name}/{what}", v)


def pointwise_outputs():
    rng = np.random.default_rng(7)
    n_max = max(POINT_N)
    x = rng.standard_normal(n_max).astype(np.float32)
    pos = (np.log1p(np.exp(rng.standard_normal(n_max))) + 0.25).astype(np.float32)
    tg = rng.standard_normal(n_max).astype(np.float32)
    kinds = {   # name -> (module, its inputs, C-ABI stem)
        "mse": (lambda a, t: RL.MSELoss()(a[0], t), (x,), "mse"),
        "gauss_nll": (lambda a, t: RL.GaussDisLoss()(a[0], a[1], t, 0), (x, pos), "gauss_nll"),
        "lognorm": (lambda a, t: RL.Lognorm()(a[0], a[1], t, 0), (pos + 0.5, pos), "lognorm"),
        "exp_mse": (lambda a, t: RL.ExpMSELoss()(a[0], t), (x * 0.5,), "exp_mse"),
    }
    for kind, (fn, ins, stem) in kinds.items():
        for n in POINT_N:
            # the forward at the C ABI: n == 0 needs real pointers, and `partial` is the caller's
            dev = [torch.tensor(a[:max(n, 1)].copy()).cuda() for a in ins]
            t = torch.tensor(tg[:max(n, 1)].copy()).cuda()
            loss = torch.full((1,), 0.5, device="cuda")
            part = torch.full((int(lib().rr_pointwise_partial_count(n)),), float("nan"), device="cuda")
            name = f"rr_{stem}_fwd_f32"
            check(getattr(lib(), name)(*[ptr(a) for a in dev], 1, ptr(t), n, ptr(loss), ptr(part), stream()), name)
            put(f"point/{kind}/n{n}/abi/loss", loss.view(torch.int32))
            put(f"point/{kind}/n{n}/abi/partial", part.view(torch.int32))
            if n == 0:
                continue
            for layout in ("flat", "column"):
                for up in ("ones", "0.37"):
                    if layout == "flat":
                        leaves = [torch.tensor(a[:n].copy()).cuda().requires_grad_(True) for a in ins]
                        cols = leaves
                    else:
                        leaves = [torch.tensor(np.stack([a[:n] for a in ins] + [tg[:n]] * (4 - len(ins)), 1)).cuda().requires_grad_(True)]
                        cols = [leaves[0][:, k] for k in range(len(ins))]
                    loss = fn(cols, torch.tensor(tg[:n].copy()))
                    (loss if up == "ones" else loss * 0.37).backward()
                    put(f"point/{kind}/n{n}/{layout}/{up}/loss", loss)
                    for k, leaf in enumerate(leaves):
                        put(f"point/{kind}/n{n}/{layout}/{up}/grad{k}", leaf.grad)


def nig_outputs():
    rng = np.random.default_rng(11)
    for cross, sizes in ((0, POINT_N), (1, (1, 63, 65, 1025))):
        for n in sizes:
            m = max(n, 1)
            mu = rng.standard_normal(m).astype(np.float32)
            v, alpha, beta = [(np.log1p(np.exp(rng.standard_normal(m))) + a).astype(np.float32) for a in (0.1, 1.1, 0.2)]
            tg = rng.standard_normal(m).astype(np.float32)
            tag = f"nig/cross{cross}/n{n}"
            dev = [torch.tensor(a).cuda() for a in (mu, v, alpha, beta)]
            t = torch.tensor(tg).cuda()
            loss = torch.full((1,), 0.5, device="cuda")
            part = torch.full((m,), float("nan"), device="cuda")
            args = [a for x in dev for a in (ptr(x), 1)] + [ptr(t), n, cross, 0.3, 1e-4]
            check(lib().rr_nig_fwd_f32(*args, ptr(loss), ptr(part), stream()), "rr_nig_fwd_f32")
            put(tag + "/abi/loss", loss.view(torch.int32))
            put(tag + "/abi/partial", part.view(torch.int32))
            if n == 0:
                continue
            for up in ("ones", "0.37"):
                shape = (n, 1) if cross else (n,)
                leaves = [torch.tensor(a.reshape(shape)).cuda().requires_grad_(True) for a in (mu, v, alpha, beta)]
                loss = RL.evidential_loss_new(*leaves, tg, 0, lam=0.3)
                (loss if up == "ones" else loss * 0.37).backward()
                put(f"{tag}/{up}/loss", loss)
                for k, leaf in enumerate(leaves):
                    put(f"{tag}/{up}/grad{k}", leaf.grad)


def small_op_outputs():
    rng = np.random.default_rng(13)
    put("digamma", RL.digamma(torch.tensor((np.abs(rng.standard_normal(70001)) * 4 + 1e-3).astype(np.float32)).cuda()))
    for n in (1, 64, 65, 8192):
        x = torch.tensor(rng.standard_normal(n).astype(np.float32)).cuda().requires_grad_(True)
        y = RL.LogCumsumExp.apply(x)
        (y * torch.arange(n, device="cuda").float().cos()).sum().backward()
        put(f"lce/n{n}/y", y)
        put(f"lce/n{n}/grad", x.grad)
    for B in (1, 257, 262149):
        t = torch.tensor(rng.standard_normal((B, 2)).astype(np.float32))
        for up in ("ones", "0.37"):
            y = torch.tensor((np.log1p(np.exp(rng.standard_normal((B, 2)))) + 0.1).astype(np.float32)).cuda().requires_grad_(True)
            loss = RL.pair_softmax_mse(y, t)
            (loss if up == "ones" else loss * 0.37).backward()
            put(f"pair_mse/B{B}/{up}/loss", loss)
            put(f"pair_mse/B{B}/{up}/grad", y.grad)
    for B in (1, 1000):
        y = torch.tensor(rng.standard_normal((B, 2)).astype(np.float32)).cuda()
        put(f"pair_acc/B{B}", RE.pair_acc_from_outputs(y, torch.tensor(np.round(rng.standard_normal((B, 2))).astype(np.float32))))


def task_outputs(seed):
    scope, targets, score, pos = window(seed, [c for c in LENGTHS if c != 8192])
    t = torch.tensor(targets)
    for task, (_, _, cols, _) in RL.TASK_STEPS.items():
        if task in ("listnet_uq", "dirichlet_uq"):
            data = pos[0]
        elif cols == 1:
            data = score
        else:
            data = np.stack([score, pos[1]], 1)
        for up in ("unit", "0.37"):
            out = torch.tensor(data).cuda().requires_grad_(True)
            loss = RL.task_step_loss(task, out, scope, t, 0, coef=0.00125)
            assert loss is not None, task
            if up == "unit":
                RL.backward(loss)
            else:
                (loss * 0.37).backward()
            put(f"s{seed}/task/{task}/{up}/loss", loss)
            put(f"s{seed}/task/{task}/{up}/grad", out.grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar="NPZ", default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    for seed in SEEDS:
        list_outputs(seed)
        task_outputs(seed)
    pointwise_outputs()
    nig_outputs()
    small_op_outputs()
    np.savez(args.out, **OUT)
    print(f"{len(OUT)} arrays -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
