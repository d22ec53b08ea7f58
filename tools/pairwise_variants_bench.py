#!/usr/bin/env python3
"""Time the pairwise trainer's new kernels against a torch restatement of the reference's formula on the same device:
BetaNet and BetaNet_envidential (forward + backward, one loss call and one autograd backward per step) and the pairwise
evaluation kernel (pairwise_acc + eval_cross_entropy_loss in one pass), at 64 queries x 64 candidates (the reference's
data have C <= 64) and at one query of 2000 candidates.  Device events over a warmed-up loop.  Needs an MI355X.

The torch restatement is float32, one query at a time like the reference's loops; the kernels evaluate every entry in
float64 (BetaNet cancels lgamma values near 360).

    python tools/pairwise_variants_bench.py [--iters 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reactranker_amd import eval as RE  # noqa: E402
from reactranker_amd import loss as RL  # noqa: E402


def torch_betanet(s, scope, t, a0):
    total, off = 0.0, 0
    for c in scope:
        tau, pi = torch.sigmoid(t[off:off + c]), torch.sigmoid(s[off:off + c])
        ta, pa = tau.unsqueeze(0).expand(c, c), pi.unsqueeze(0).expand(c, c)
        tb, pb = ta.t(), pa.t()
        x1, x2 = ta / (ta + tb), tb / (ta + tb)
        aT, bT, aP, bP = x1 * a0, x2 * a0, pa / (pa + pb) * a0, pb / (pa + pb) * a0
        lt = (aT - 1) * torch.log(x1) + (bT - 1) * torch.log(x2) - (torch.lgamma(aT) + torch.lgamma(bT) - torch.lgamma(aT + bT))
        lp = (aP - 1) * torch.log(x1) + (bP - 1) * torch.log(x2) - (torch.lgamma(aP) + torch.lgamma(bP) - torch.lgamma(aP + bP))
        total = total + torch.sum(torch.exp(lt) * (lt - lp))
        off += c
    return total


def torch_beta_evi(p, scope, t, coef):
    total, off = 0.0, 0
    for c in scope:
        tau, q = torch.sigmoid(t[off:off + c]), p[off:off + c]
        ta, pa = tau.unsqueeze(0).expand(c, c), q.unsqueeze(0).expand(c, c)
        tb, pb = ta.t(), pa.t()
        T1, T2, P1, P2 = ta / (ta + tb), tb / (ta + tb), pa / (pa + pb), pb / (pa + pb)
        err = (T1 - P1) ** 2 + (T2 - P2) ** 2
        var = P1 * (1 - P1) / (pa + pb + 1) + P2 * (1 - P2) / (pa + pb + 1)
        pen = 2 * torch.abs(torch.log(T1 / P1) * (pa - 1))
        total = total + torch.sum(err + var + coef * pen)
        off += c
    return total


def torch_eval(s, scope, t, sigma):
    acc, n, ce, pairs, off = 0.0, 0, 0.0, 0.0, 0
    for c in scope:
        sq, tq = s[off:off + c].unsqueeze(1), t[off:off + c].unsqueeze(1)
        rel = tq - tq.t()
        pos, neg = (rel > 0).float(), (rel < 0).float()
        npos = pos.sum()
        d = sq - sq.t()
        acc = acc + 1 - torch.sum(torch.abs((d > 0).float() - pos)) / (2 * npos)
        C = 0.5 * (1 - (pos - neg)) * sigma * d - F.logsigmoid(-sigma * d)
        ce = ce + torch.sum(C * (pos + neg))
        pairs = pairs + 2 * npos
        n += 1
        off += c
    return acc / n, ce / pairs


def timed(f, iters, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000.0 / iters, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    res = {}
    for label, scope, iters in (("64x64", [64] * 64, args.iters), ("1x2000", [2000], max(3, args.iters // 10))):
        M = sum(scope)
        s = torch.tensor((rng.standard_normal(M) * 1.5).astype(np.float32)).cuda().requires_grad_(True)
        p = torch.tensor((np.log1p(np.exp(rng.standard_normal(M))) + 1.0).astype(np.float32)).cuda().requires_grad_(True)
        t = torch.tensor(rng.standard_normal(M).astype(np.float32)).cuda()
        cases = {
            "betanet fwd+bwd": (lambda: RL.betanet_loss(s, scope, t, 100.0, 0)[0].backward(),
                                lambda: torch_betanet(s, scope, t, 100.0).backward()),
            "beta_evidential fwd+bwd": (lambda: RL.beta_evidential_loss(p, scope, t, 0.004, 0)[0].backward(),
                                        lambda: torch_beta_evi(p, scope, t, 0.004).backward()),
            "pairwise eval": (lambda: RE.pairwise_stats_from_scores(s.detach(), scope, t, 1.0, 0),
                              lambda: torch_eval(s.detach(), scope, t, 1.0)),
        }
        for name, (hip, ref) in cases.items():
            a, b = timed(hip, iters, args.warmup), timed(ref, iters, args.warmup)
            res[f"{name} {label}"] = dict(hip_us=a, torch_us=b)
            print(f"{name:26s} {label:7s} HIP {a:10.1f} us   torch restatement {b:10.1f} us   ratio {b / a:6.2f}x")
    print(json.dumps(dict(us_per_call=res)))


if __name__ == "__main__":
    main()
