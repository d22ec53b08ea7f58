#!/usr/bin/env python3
"""Time each of the reference trainer's remaining losses at 64 queries x 64 candidates, forward + backward (one loss call
and one autograd backward per step), with device events over a warmed-up loop.  Needs an MI355X.

    python tools/loss_variants_bench.py [--iters 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reactranker_amd import loss as RL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    Q, C = 64, 64
    M = Q * C
    scope = [C] * Q
    rng = np.random.default_rng(0)
    sp = lambda x: np.log1p(np.exp(x))                                          # noqa: E731
    out = torch.tensor(np.stack([rng.standard_normal(M), sp(rng.standard_normal(M)) + 1e-6,
                                 sp(rng.standard_normal(M)) + 1 + 1e-6, sp(rng.standard_normal(M)) + 1e-6], 1)
                       .astype(np.float32)).cuda().requires_grad_(True)           # an [M, 4] NIG head output
    pos = torch.tensor((sp(rng.standard_normal(M)) + 1.0).astype(np.float32)).cuda().requires_grad_(True)
    t = torch.tensor(rng.standard_normal(M).astype(np.float32)).cuda()
    cases = {
        "MLEDisLoss": lambda: RL.MLEDisLoss()(out[:, 0:1], out[:, 1:2], scope, t, 0),
        "Listnet_For_Gauss": lambda: RL.Listnet_For_Gauss()(out[:, 0:1], out[:, 1:2], scope, t, 0),
        "Listnetlognorm": lambda: RL.Listnetlognorm()(out[:, 2:3], out[:, 1:2], scope, t, 0),
        "Listnet_For_evidential": lambda: RL.Listnet_For_evidential()(out[:, 0:1], out[:, 1:2], out[:, 2:3], scope, t, 0),
        "Listnet_with_uq": lambda: RL.Listnet_with_uq()(pos, scope, t, 0.5, 1, 3, 0),
        "Dirichlet_uq": lambda: RL.Dirichlet_uq()(pos, scope, t, 0.5, 1, 3, 0),
        "evidential_loss_new[M]": lambda: RL.evidential_loss_new(out[:, 0], out[:, 1], out[:, 2], out[:, 3], t, 0),
        "evidential_loss_new[M,1] (M x M)": lambda: RL.evidential_loss_new(out[:, 0:1], out[:, 1:2], out[:, 2:3], out[:, 3:4], t, 0),
        "Lognorm": lambda: RL.Lognorm()(pos, out[:, 1], t, 0),
        "ExpMSELoss": lambda: RL.ExpMSELoss()(out[:, 0], t),
    }
    res = {}
    for name, f in cases.items():
        for _ in range(args.warmup):
            f().sum().backward()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            f().sum().backward()
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) * 1000.0 / args.iters, 1)
        print(f"{name:36s} {res[name]:8.1f} us / step (fwd + bwd, {Q} x {C})")
    print(json.dumps(dict(queries=Q, candidates=C, us_per_step=res)))


if __name__ == "__main__":
    main()
