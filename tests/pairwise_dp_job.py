"""A short BetaNet training job through run_train_pairwise.run_train, for 1 or N processes (not a test module:
tests/test_gpu_pairwise_variants.py starts it - once as a plain process, once under `python -m torch.distributed.run
--nproc-per-node 2` - and compares the histories rank 0 writes).  Built like tests/dp_trainer_job.py: every rank builds the
SAME global steps (seeded) and keeps its contiguous block of whole queries of each.  Half of the steps carry the window's
`sq_pairs` in their `global` counts, the other half leave it to the trainer's all-reduce.  Backend: $RR_DIST_BACKEND
(default "nccl" = RCCL); RR_SINGLE_DEVICE=1 puts every rank on GPU 0 (a one-GPU box)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SCOPES = [[5, 3, 7, 2, 6], [4, 8, 3, 6, 5, 2], [9, 2, 4], [6, 6, 1, 3, 7]]       # global steps: ragged lists
VAL_SCOPES = [[5, 4, 7], [3, 8, 2, 6]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", required=True)
    ap.add_argument("--ckpt", required=True)
    args = ap.parse_args()
    import torch.distributed as dist
    from reactranker_amd import dp, featurization, synth
    from reactranker_amd.base_model import build_model
    from reactranker_amd.loss import sq_pairs
    from reactranker_amd.run_train_pairwise import run_train
    from reactranker_amd.train_utils import build_lr_scheduler, build_optimizer
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = 0 if os.environ.get("RR_SINGLE_DEVICE") else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group(os.environ.get("RR_DIST_BACKEND", "nccl"), rank=rank, world_size=world)

    def batches(seed0, scopes):
        out = []
        for i, scope in enumerate(scopes):
            qb = synth.make_queries(seed0 + i, len(scope), scope, atoms_lo=6, atoms_hi=12)
            tg = np.array([s.edges.shape[0] for s in qb.p_specs], np.float32) * 0.7 + 3.0 * qb.add_features[:, 0]
            qb.targets = (tg + 0.05 * np.arange(len(tg), dtype=np.float32)).astype(np.float32)
            mine, glob = dp.shard_query_batch(qb, rank, world)
            if i % 2 == 0:
                glob = dict(glob, sq_pairs=sq_pairs(scope))
            b = dict(scope=mine.scope, targets=torch.tensor(mine.targets), add=mine.add_features, **{"global": glob})
            if len(mine.scope):
                b["r"] = featurization.BatchMolGraph(mine.r_specs, K=4)        # global pad width on every rank
                b["p"] = featurization.BatchMolGraph(mine.p_specs, K=4)
            else:
                b["r"] = b["p"] = None
            out.append(b)
        return out

    torch.manual_seed(0)
    model = build_model(hidden_size=64, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.0, task_num=1,
                        ffn_last_layer="no_softplus", add_features_dim=1).cuda(local)
    opt = build_optimizer(model)
    sch = build_lr_scheduler(opt, warmup_epochs=1.0, total_epochs=args.epochs, train_data_size=sum(len(s) for s in SCOPES),
                             batch_size=5, init_lr=1e-4, max_lr=4e-4, final_lr=1e-4)
    hist = run_train(model, sch, batches(7000, SCOPES), batches(7100, VAL_SCOPES), args.ckpt, opt, args.epochs, 0, local,
                     train_strategy="sum_session", task_type="BetaNet", target_name="ea", save_metric=None)
    if rank == 0:
        with open(args.out, "w") as f:
            json.dump(dict(world=world, backend=os.environ.get("RR_DIST_BACKEND", "nccl") if world > 1 else None,
                           history=hist), f)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
