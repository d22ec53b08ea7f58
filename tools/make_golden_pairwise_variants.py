#!/usr/bin/env python3
"""Generate tests/golden/pairwise_variants.npz by running the REFERENCE ITSELF, in the manner of tools/make_golden.py (whose
rdkit stub and reference import it reuses; the reference's modules are imported unmodified).  Writes that one file only.

  beta loops:  the real beta_dis_train_loop / beta_evi_train_loop driven with stub model / processor / optimizer objects, one
               call per group of two queries (batch_size=2, so the loops' broken end-of-epoch flush is never reached): the
               group's normalised loss and its gradient with respect to the preset scores
  evaluation:  pairwise_acc, eval_cross_entropy_loss and pairwise_baseline_acc on preset scores
  pair order:  DataProcessor.generate_query_pairs on a small pandas frame, as row-index lists
  pair model:  models/ranknet_baseline.build_model(hidden_size=32, ...) on synth graphs: outputs in eval mode, and the real
               baseline_pairwise_training_loop in train mode with dropout = 0: outputs, loss and every parameter gradient

Fixed seeds: a rerun reproduces every array.

Usage: python tools/make_golden_pairwise_variants.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402  (installs the rdkit stub and puts the reference on sys.path)

from reactranker.data.load_reactions import DataProcessor  # noqa: E402
from reactranker.models import ranknet_baseline as ref_pair_model  # noqa: E402
from reactranker.train import eval as ref_eval  # noqa: E402
from reactranker.train.train_pairwise import (baseline_pairwise_training_loop, beta_dis_train_loop,  # noqa: E402
                                              beta_evi_train_loop)

from reactranker_amd import pairs, synth  # noqa: E402

OUT = MG.OUT
ALPHA0 = 100
EVI_ARGS = (0.01, 2, 5)              # max_coeff, epoch, epochs: coefficient 0.01 * (2 / 4) ** 3
SIGMA = 1.0
# every case is one group of two queries = one optimizer step of the reference's loops
SQ_CASES = {
    "c1_c2": ([1, 2], 1.0), "c2_c5": ([2, 5], 1.0), "c64": ([64, 64], 1.0), "c64_s3": ([64, 33], 3.0),
    "c300": ([300, 7], 1.0), "c300_s3": ([300, 129], 3.0), "c2000": ([2000, 3], 1.0), "tied": ([6, 9], 1.0),
}
EVAL_SCOPE = [5, 1, 8, 4, 64, 3, 2]
PAIR_CASE = dict(hidden_size=32, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, task_num=2,
                 ffn_last_layer="evidential", scope=[3, 4, 2], seed=57, wseed=131, batch_size=12)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def f32_exact(x):
    """float32-representable values: the reference compares targets in float64, the kernels in float32."""
    x = np.asarray(x, np.float32)
    assert np.array_equal(x.astype(np.float64).astype(np.float32), x)
    return x


class _QueryProcessor:
    df = None

    def __init__(self, scope, targets):
        self.scope, self.targets = scope, targets

    def generate_batch_per_query(self, **kw):
        off = 0
        for c in self.scope:
            yield np.array([["r", "p%d" % i] for i in range(c)]), self.targets[off:off + c].astype(np.float64)
            off += c

    def get_num_pairs(self):
        n, off = 0, 0
        for c in self.scope:
            t = self.targets[off:off + c]
            n += int((t[:, None] != t[None, :]).sum())
            off += c
        return n


class _Leaves:
    def __init__(self, leaves):
        self._it = iter(leaves)

    def __call__(self, *a, **k):
        return next(self._it)

    def eval(self):
        pass

    def zero_grad(self):
        pass


def gen_sq(out):
    rng = np.random.default_rng(777)
    names = []
    for name, (scope, scale) in SQ_CASES.items():
        m = sum(scope)
        t = (rng.standard_normal(m) * scale).astype(np.float32)
        if name == "tied":
            t = np.round(t * 2) / 2
            t[:3] = t[0]
        t = f32_exact(t)
        s = (rng.standard_normal(m) * 1.5).astype(np.float32)
        p = (np.log1p(np.exp(rng.standard_normal(m))) + 1.0).astype(np.float32)
        P = "sq." + name + "."
        out[P + "scope"], out[P + "targets"], out[P + "score"], out[P + "pos"] = np.asarray(scope, np.int32), t, s, p
        for key, x in (("betanet", s), ("beta_evidential", p)):
            leaves = [torch.tensor(q, requires_grad=True) for q in np.split(x, np.cumsum(scope)[:-1])]
            proc = _QueryProcessor(scope, t)
            if key == "betanet":
                val = quiet(beta_dis_train_loop, 0, _Leaves(leaves), None, MG._Noop(), MG._Noop(), MG._StubGraphs(), proc,
                            batch_size=2, alpha0=ALPHA0, gpu=None)
            else:
                val = quiet(beta_evi_train_loop, EVI_ARGS[1], _Leaves(leaves), MG._Noop(), MG._Noop(), MG._StubGraphs(), proc,
                            batch_size=2, max_coeff=EVI_ARGS[0], epochs=EVI_ARGS[2], gpu=None)
            out[P + key] = np.float32(val)                       # group loss / group pairs
            out[P + key + "_g"] = np.concatenate([l.grad.numpy() for l in leaves])
        names.append(name)
    out["sq_cases"] = np.asarray(names)
    out["alpha0"] = np.float32(ALPHA0)
    out["evi_args"] = np.asarray(EVI_ARGS, np.float64)


def gen_eval(out):
    rng = np.random.default_rng(778)
    scope = EVAL_SCOPE
    m = sum(scope)
    t = np.round(rng.standard_normal(m) * 4) / 4                 # quarter steps: ties, exact in float32
    t[5] = 0.5                                                   # the one-candidate query
    t[-5:-2] = 1.25                                              # a query with one distinct value: no pair, skipped
    t = f32_exact(t)
    s = np.round(rng.standard_normal(m) * 3) / 2
    s = f32_exact(s)                                             # half steps: tied scores
    out["eval.scope"], out["eval.targets"], out["eval.scores"] = np.asarray(scope, np.int32), t, s
    out["eval.sigma"] = np.float32(SIGMA)
    split = np.cumsum(scope)[:-1]
    rows = [torch.tensor(q) for q in np.split(s, split)]
    proc = _QueryProcessor(scope, t)
    out["eval.pairwise_acc"] = np.float64(quiet(ref_eval.pairwise_acc, _Leaves(rows), None, proc, MG._StubGraphs(),
                                                show_info=False))
    # eval_cross_entropy_loss skips pair-less queries BEFORE the model call, and needs [C, 1] predictions
    used = [bool((q[:, None] > q[None, :]).any()) for q in np.split(t, split)]
    cols = [r.reshape(-1, 1) for r, u in zip(rows, used) if u]
    ce = quiet(ref_eval.eval_cross_entropy_loss, _Leaves(cols), None, proc, 0, MG._StubGraphs(), sigma=SIGMA)
    out["eval.cross_entropy"] = np.float64(float(ce))
    out["eval.used"] = np.asarray(used)

    # pairwise_baseline_acc: preset [B, 2] outputs per batch
    B = [7, 7, 3]
    ys = [f32_exact(np.round(rng.random((b, 2)) * 8) / 8 + 0.125) for b in B]
    ts = [f32_exact(np.round(rng.standard_normal((b, 2)) * 4) / 4) for b in B]

    class Loader:
        def generate_query_pair_batch(self, **kw):
            for y, tt in zip(ys, ts):
                x = np.array([["r", "p"]] * len(y))
                yield x, tt[:, :1], x, tt[:, 1:]
    acc = quiet(ref_eval.pairwise_baseline_acc, _Leaves([torch.tensor(y) for y in ys]), None, Loader(), MG._StubGraphs())
    out["pairacc.sizes"] = np.asarray(B, np.int32)
    out["pairacc.y"], out["pairacc.t"] = np.concatenate(ys), np.concatenate(ts)
    out["pairacc.acc"] = np.float64(acc)


def gen_pair_order(out):
    cases = {"distinct": [0.5, -1.0, 2.0, 0.25], "tied": [1.0, 1.0, 2.0, 1.0, 3.0, 2.0], "one_value": [4.0, 4.0, 4.0],
             "single": [1.5]}
    for name, vals in cases.items():
        df = pd.DataFrame(dict(idx=np.arange(len(vals)), rsmi=["R"] * len(vals), psmi=["P%d" % i for i in range(len(vals))],
                               ea=vals))
        x_i, y_i, x_j, y_j = DataProcessor.generate_query_pairs(None, df, "R", "ea", seed=0)
        ii = [int(p[1:]) for p in x_i[:, 1]] if len(x_i) else []
        jj = [int(p[1:]) for p in x_j[:, 1]] if len(x_j) else []
        assert np.array_equal(np.asarray(vals)[ii], y_i.reshape(-1)) and np.array_equal(np.asarray(vals)[jj], y_j.reshape(-1))
        out["order." + name + ".targets"] = np.asarray(vals, np.float32)
        out["order." + name + ".i"], out["order." + name + ".j"] = np.asarray(ii, np.int32), np.asarray(jj, np.int32)
    out["order_cases"] = np.asarray(list(cases))


def gen_pair_model(out):
    c = PAIR_CASE
    kw = {k: c[k] for k in ("hidden_size", "mpnn_depth", "mpnn_diff_depth", "ffn_depth", "use_bias", "task_num", "ffn_last_layer")}
    model = ref_pair_model.build_model(dropout=0.0, **kw)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = synth.seeded_weights(shapes, c["wseed"])
    model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    qb = synth.make_queries(c["seed"], len(c["scope"]), c["scope"], atoms_lo=5, atoms_hi=10)
    t = f32_exact(np.round(qb.targets * 8) / 8)
    ii, jj = pairs.window_pairs(c["scope"], t)
    B = c["batch_size"]
    assert len(ii) > B, "need one whole batch and a short one"
    names_r = {id(s): "r%d" % k for k, s in enumerate({id(s): s for s in qb.r_specs}.values())}
    graphs = {}
    for k, (r, p) in enumerate(zip(qb.r_specs, qb.p_specs)):
        graphs[names_r[id(r)]] = r
        graphs["p%d" % k] = p

    class Graphs:
        def parsing_smiles(self, smi):
            return MG.ref_batch([graphs[s] for s in smi])

    def x_of(rows, prod):
        return np.array([[names_r[id(qb.r_specs[a])], "p%d" % b] for a, b in zip(rows, prod)])

    class Loader:
        def generate_query_pair_batch(self, **kw):
            for lo in range(0, len(ii), B):
                a, b = ii[lo:lo + B], jj[lo:lo + B]
                yield x_of(a, a), t[a].reshape(-1, 1), x_of(a, b), t[b].reshape(-1, 1)

    # eval mode, whole first batch and the short last one
    model.eval()
    outs = []
    for lo in range(0, len(ii), B):
        a, b = ii[lo:lo + B], jj[lo:lo + B]
        g = Graphs()
        rb, p1b, p2b = (g.parsing_smiles(x[:, col]) for x, col in ((x_of(a, a), 0), (x_of(a, a), 1), (x_of(a, b), 1)))
        # one pad width in all three graphs: the encoder's output depends on it (reactranker_amd.pairs packs with the widest)
        assert rb.max_num_bonds == p1b.max_num_bonds == p2b.max_num_bonds, "pick a seed whose batches share the pad width"
        with torch.no_grad():
            outs.append(model(rb, p1b, p2b, gpu=None).numpy())
    out["pair.out_eval"] = np.concatenate(outs)

    # the real training loop, train mode, dropout 0: only the first (whole) batch trains, the short one is skipped
    class Opt:
        grads = None

        def step(self):
            assert Opt.grads is None, "one whole batch expected"
            Opt.grads = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}
    model.train()
    model.zero_grad()
    val = quiet(baseline_pairwise_training_loop, 0, 5, model, Opt(), MG._Noop(), Graphs(), Loader(), batch_size=B, gpu=None)
    out["pair.loss"] = np.float32(val)
    for k, v in Opt.grads.items():
        out["pair.g." + k] = v
    for k, v in w.items():
        out["pair.w." + k] = v
    out["pair.scope"], out["pair.targets"] = np.asarray(c["scope"], np.int32), t
    out["pair.i"], out["pair.j"] = ii, jj
    out["pair.cfg"] = np.asarray([c["hidden_size"], c["mpnn_depth"], c["mpnn_diff_depth"], c["ffn_depth"], c["task_num"], c["seed"],
                                  c["wseed"], B], np.int64)


def main():
    out = {}
    gen_sq(out)
    gen_eval(out)
    gen_pair_order(out)
    gen_pair_model(out)
    path = os.path.join(OUT, "pairwise_variants.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
