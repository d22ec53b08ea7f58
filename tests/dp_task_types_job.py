"""A short listwise training job per task type, for 1 or N processes (not a test module: tests/test_gpu_dp_task_types.py
starts it - once as a plain process, once under `python -m torch.distributed.run --nproc-per-node 2` - and compares the
histories rank 0 writes).  Modelled on tests/dp_trainer_job.py: every rank builds the SAME global steps (seeded), keeps its
contiguous block of whole queries of each (reactranker_amd.dp.shard_query_batch: ragged lists, so the shards are ragged
too) and hands train_listwise.train its shards.  The task types here sum terms with different normalisers (or are served by
one pointwise kernel): the trainer divides every term by the whole step's count and sums the ranks' gradients unweighted.
The four NIG task types must be refused, on every rank, before any step: `--refused` records the error each rank got.
Backend: $RR_DIST_BACKEND (default "nccl" = RCCL); RR_SINGLE_DEVICE=1 puts every rank on GPU 0 (a one-GPU box)."""
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

HEADS = {  # task type -> build_model arguments of the head it trains (as examples/train_synthetic.py picks them)
    "mle_gaussian": dict(task_num=2, ffn_last_layer="with_softplus"),
    "listnet_gauss": dict(task_num=2, ffn_last_layer="with_softplus"),
    "mle_regression": dict(task_num=1, ffn_last_layer="with_softplus"),
    "listnet_regression": dict(task_num=1, ffn_last_layer="with_softplus"),
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", required=True)
    ap.add_argument("--refused", default="")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch.distributed as dist
    from reactranker_amd import dp, featurization, synth
    from reactranker_amd import loss as RL
    from reactranker_amd import train_listwise as TL
    from reactranker_amd import train_utils as TU
    from reactranker_amd.base_model import build_model
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
            # learnable, well separated targets, standardised over the whole step (the same numbers on every rank)
            tg = np.array([s.edges.shape[0] for s in qb.p_specs], np.float32) * 0.7 + 3.0 * qb.add_features[:, 0]
            tg = tg + 0.05 * np.arange(len(tg), dtype=np.float32)
            qb.targets = ((tg - tg.mean()) / (tg.std() + 1e-6)).astype(np.float32)
            mine, glob = dp.shard_query_batch(qb, rank, world)
            b = dict(scope=mine.scope, targets=torch.tensor(mine.targets), add=mine.add_features, **{"global": glob})
            if len(mine.scope):
                b["r"] = featurization.BatchMolGraph(mine.r_specs, K=4)        # global pad width on every rank
                b["p"] = featurization.BatchMolGraph(mine.p_specs, K=4)
            else:
                b["r"] = b["p"] = None
            out.append(b)
        return out

    def job(task):
        torch.manual_seed(0)
        model = build_model(hidden_size=64, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.0,
                            add_features_dim=1, **HEADS[task]).cuda(local)
        opt = TU.build_optimizer(model)
        sch = TU.build_lr_scheduler(opt, warmup_epochs=1, total_epochs=args.epochs, train_data_size=len(SCOPES) * 5, batch_size=5,
                                    init_lr=1e-4, max_lr=4e-4, final_lr=1e-4)
        return TL.train(model, sch, batches(7000, SCOPES), batches(7100, VAL_SCOPES), None, opt, args.epochs, seed=3, gpu=local,
                        task_type=task, save_metric="all", max_coeff=0.2)

    result, refused = {}, {}
    for task in [t for t in args.tasks.split(",") if t]:
        hits = RL.FusedStep.hits
        hist = job(task)
        result[task] = dict(history=hist, fused_hits=RL.FusedStep.hits - hits)
    for task in [t for t in args.refused.split(",") if t]:
        steps = []
        orig = TL.batch_loss
        TL.batch_loss = lambda *a, **k: (steps.append(1), orig(*a, **k))[1]
        try:
            job(task)
            err = None
        except ValueError as e:
            err = str(e)
        finally:
            TL.batch_loss = orig
        errs = [None] * world
        if world > 1:
            dist.all_gather_object(errs, dict(error=err, steps=len(steps)))
        else:
            errs = [dict(error=err, steps=len(steps))]
        refused[task] = errs
    if rank == 0:
        with open(args.out, "w") as f:
            json.dump(dict(world=world, backend=os.environ.get("RR_DIST_BACKEND", "nccl") if world > 1 else None,
                           result=result, refused=refused), f)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
