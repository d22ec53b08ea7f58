"""Every output of the five window losses (RankNet, LambdaRank, ApproxNDCG, BetaNet, beta-evidential) and the per-epoch losses
of the train_pairwise loops, as one .npz - to be run in two trees on one MI355X and compared byte for byte:
    python tools/window_loss_bits.py --out A.npz            (in each tree; only public loss.py functions and the C ABI)
    python tools/window_loss_bits.py --compare A.npz B.npz  (prints the array count and the names that differ; status 1 on any)
Per seed, a ragged window with list lengths 0, 1, 2, 63, 64, 65, 300, 1000, 8192: loss, count and gradient of every loss,
from a contiguous [M] score and from the first column of an [M, 2] tensor (strided), with the fused step on and off, for
`backward(loss)` (the library's constant one), a plain `loss.backward()` and an upstream gradient of 0.37, with and without
the host normaliser of the two losses that take one; ranknet_lambda and soft_rank with its backward; the count-carrying entry
points at the C ABI with their `partial` buffers.  Then two epochs of each loop on `synth` windows, single process."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import featurization, pairs, ranknet_baseline, synth  # noqa: E402
from reactranker_amd import loss as RL  # noqa: E402
from reactranker_amd import train_pairwise as TP  # noqa: E402
from reactranker_amd import train_utils as TU  # noqa: E402
from reactranker_amd._lib import check, lib, ptr, stream  # noqa: E402
from reactranker_amd.base_model import build_model  # noqa: E402

SEEDS = (0, 1)
LENGTHS = (0, 1, 2, 63, 64, 65, 300, 1000, 8192)
OUT = {}


def put(name, x):
    assert name not in OUT, name
    OUT[name] = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def window(seed):
    rng = np.random.default_rng(seed)
    scope = [int(c) for c in rng.permutation(LENGTHS)]
    M = sum(scope)
    score = rng.standard_normal(M).astype(np.float32)
    targets = np.round(rng.standard_normal(M) * 2).astype(np.float32) / 2        # ties inside every longer list
    return scope, score, targets


def losses_of(scope, targets, pairs_n):
    Q = len(scope)
    return {   # name -> (function of the score column, needs positive scores, normalised twin or None, has a step entry)
        "ranknet": (lambda y: RL.ranknet_loss(y, scope, targets, 1.0, 0), False, None, False),
        "lambdarank": (lambda y: RL.lambdarank_loss(y, scope, targets, 0.5, 10, 0), False,
                       lambda y: RL.lambdarank_loss(y, scope, targets, 0.5, 10, 0, pairs=pairs_n), True),
        "approx_ndcg": (lambda y: RL.approx_ndcg_loss(y, scope, targets, 0.7, 10, 0), False,
                        lambda y: RL.approx_ndcg_loss(y, scope, targets, 0.7, 10, 0, queries=Q), True),
        "betanet": (lambda y: RL.betanet_loss(y, scope, targets, 100.0, 0), False, None, False),
        "beta_evidential": (lambda y: RL.beta_evidential_loss(y, scope, targets, 0.004, 0), True, None, False),
    }


def window_outputs(seed):
    scope, score, targets = window(seed)
    t = torch.tensor(targets)
    positive = (np.log1p(np.exp(score)) + 1.0).astype(np.float32)
    pairs_n = int(RL.ranknet_loss(torch.tensor(score).cuda(), scope, t, 1.0, 0)[1])
    for kind, (fn, pos, fn_norm, has_step) in losses_of(scope, t, pairs_n).items():
        base = positive if pos else score
        for layout in ("flat", "column"):
            for form, f in (("sum", fn), ("norm", fn_norm)):
                if f is None:
                    continue
                for fused in ((True, False) if has_step else (True,)):
                    for up in (("unit", "ones", "0.37") if has_step else ("ones", "0.37")):
                        RL.FusedStep.enabled = fused
                        if layout == "flat":
                            leaf = torch.tensor(base).cuda().requires_grad_(True)
                            y = leaf
                        else:
                            leaf = torch.tensor(np.stack([base, -base], 1)).cuda().requires_grad_(True)
                            y = leaf[:, 0]
                        loss, count = f(y)
                        if up == "unit":
                            RL.backward(loss)
                        elif up == "ones":
                            loss.backward()
                        else:
                            (loss * 0.37).backward()
                        tag = f"s{seed}/{kind}/{layout}/{form}/fused{int(fused)}/{up}"
                        put(tag + "/loss", loss)
                        put(tag + "/count", count)
                        put(tag + "/grad", leaf.grad)
    RL.FusedStep.enabled = True
    s = torch.tensor(np.stack([score, -score], 1)).cuda().requires_grad_(True)
    put(f"s{seed}/ranknet_lambda", RL.ranknet_lambda(s, scope, t, 1.0, 0))
    r = RL.soft_rank(s, scope, 0.7, 0)
    (r * torch.arange(r.shape[0], device="cuda").float().cos()).sum().backward()
    put(f"s{seed}/soft_rank", r)
    put(f"s{seed}/soft_rank/grad", s.grad)
    # the C ABI with the caller's partial buffer
    sc, tg = torch.tensor(score).cuda(), t.cuda()
    seg = torch.tensor(np.concatenate([[0], np.cumsum(scope)]).astype(np.int32)).cuda()
    Q, L, M = len(scope), max(scope), len(score)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    for kind, hyper, has_step in (("ranknet", (1.0,), False), ("lambdarank", (0.5, 10), True), ("approx_ndcg", (0.7, 10), True)):
        for step in ((False, True) if has_step else (False,)):
            loss = torch.full((1,), float("nan"), device="cuda")
            count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            part = torch.full((2 * Q,), float("nan"), device="cuda")
            d = torch.zeros(M, device="cuda")
            head = [ptr(sc), 1, ptr(tg), ptr(seg), Q, L, *hyper]
            if step:
                name, tail = f"rr_{kind}_step_f32", [0.37, ptr(loss), ptr(count), ptr(part), ptr(counter), ptr(d), 1]
            else:
                name, tail = f"rr_{kind}_fwd_f32", [ptr(loss), ptr(count), ptr(part)]
            check(getattr(lib(), name)(*head, *tail, stream()), name)
            for what, x in (("loss", loss), ("count", count), ("partial", part.view(torch.int32)), ("dscore", d), ("counter", counter)):
                put(f"s{seed}/abi/{name}/{what}", x)


def synth_windows(seed0, scopes):
    out = []
    for i, scope in enumerate(scopes):
        qb = synth.make_queries(seed0 + i, len(scope), scope, atoms_lo=6, atoms_hi=12)
        tg = np.array([s.edges.shape[0] for s in qb.p_specs], np.float32) * 0.7 + 3.0 * qb.add_features[:, 0]
        tg = (tg + 0.05 * np.arange(len(tg), dtype=np.float32)).astype(np.float32)
        tg = (tg - tg.mean()) / tg.std()
        out.append(dict(r=featurization.BatchMolGraph(qb.r_specs, K=4), p=featurization.BatchMolGraph(qb.p_specs, K=4),
                        scope=qb.scope, targets=torch.tensor(tg), add=qb.add_features, mols_r=qb.r_specs, mols_p=qb.p_specs))
    return out


def trainer_outputs():
    kw = dict(hidden_size=32, mpnn_depth=2, mpnn_diff_depth=2, ffn_depth=2, use_bias=True, dropout=0.0)
    scopes = [[4, 3, 5], [2, 6, 1, 3], [1, 1], [5, 5]]                   # the third window has no pair: skipped by every loop
    loops = {
        "sum_session": ("no_softplus", lambda ep, m, o, s, w: TP.factorized_training_loop(ep, m, o, s, w, 1.0, "sum_session", gpu=0)),
        "accelerate_grad": ("no_softplus", lambda ep, m, o, s, w: TP.factorized_training_loop(ep, m, o, s, w, 1.0, "accelerate_grad", gpu=0)),
        "lambdarank": ("no_softplus", lambda ep, m, o, s, w: TP.factorized_training_loop(ep, m, o, s, w, 1.0, "lambdarank", gpu=0, ndcg_k=3)),
        "approx_ndcg": ("no_softplus", lambda ep, m, o, s, w: TP.factorized_training_loop(ep, m, o, s, w, 1.0, "approx_ndcg", gpu=0,
                                                                                          temperature=0.5)),
        "beta_dis": ("no_softplus", lambda ep, m, o, s, w: TP.beta_dis_train_loop(ep, m, o, s, w, alpha0=100, gpu=0)),
        "beta_evi": ("evidential", lambda ep, m, o, s, w: TP.beta_evi_train_loop(ep, m, o, s, w, max_coeff=0.01, epochs=3, gpu=0)),
        "baseline": (None, lambda ep, m, o, s, w: TP.baseline_pairwise_training_loop(ep, 2, m, o, s, w, batch_size=12, gpu=0)),
    }
    for name, (last, loop) in loops.items():
        torch.manual_seed(0)
        w = synth_windows(100, scopes)
        if last is None:
            model = ranknet_baseline.build_model(task_num=2, ffn_last_layer="evidential", **kw).cuda()
            w = [pb for b in w if max(b["scope"]) > 1
                 for pb in pairs.pair_windows(b["mols_r"], b["mols_p"], b["scope"], b["targets"].numpy(), 12)]
        else:
            model = build_model(task_num=1, ffn_last_layer=last, add_features_dim=1, **kw).cuda()
        opt = TU.build_optimizer(model)
        sch = TU.build_lr_scheduler(opt, warmup_epochs=1.0, total_epochs=2, train_data_size=16, batch_size=4, init_lr=1e-4,
                                    max_lr=5e-4, final_lr=1e-4)
        put(f"train/{name}/epoch_losses", np.array([loop(ep, model, opt, sch, w) for ep in range(2)], np.float64))
        put(f"train/{name}/weights", torch.cat([p.detach().reshape(-1) for p in model.parameters()]))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    names = sorted(set(A.files) | set(B.files))
    bad = [n for n in names if n not in A.files or n not in B.files or A[n].dtype != B[n].dtype or A[n].shape != B[n].shape
           or A[n].tobytes() != B[n].tobytes()]
    print(f"{len(names)} arrays, {len(bad)} differ" + "".join(f"\n  {n}" for n in bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar="NPZ", default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    for seed in SEEDS:
        window_outputs(seed)
    trainer_outputs()
    np.savez(args.out, **OUT)
    print(f"{len(OUT)} arrays -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
