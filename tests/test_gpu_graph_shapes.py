"""Graph shapes the synthetic generator never draws (tests/graph_shapes.py), through the whole model on the GPU: hubs with five
and six neighbours (pad width K = 6, bond-to-bond width Kb = 5: the generic-K loops of the forward gather and of the fused
backward gather), molecules without bonds and a batch whose bond table is the padding row alone, two-atom molecules
(K = 1, an empty bond-to-bond table), disconnected molecules, a pad width wider than any atom needs, and ragged lists with
one and with seventy candidates (copy tables 70 wide in the shared-prefix backward).

Each batch is held (i) in eval mode against the float64 oracle, with and without reactant de-duplication, (ii) in train mode
through tests/test_gpu_headline_kernels.py's training-step harness with its rules unchanged (gate flips only within 1e-5 of
zero; scores and loss within max(1e-5, 3 x the fp32 oracle's own distance to fp64); every parameter gradient within
max(5e-5 x scale + 1e-6, 3 x the fp32 oracle's noise) under the HIP step's gates), and (iii) plan against per-op path, bit for bit.
tests/conftest.py keys the GEMM arithmetic on module names; this module sets it itself: the oracle comparisons run in both
forms, the bit-identity tests are pinned to the three-term form."""
import functools

import pytest
import torch

from reactranker_amd import featurization, synth
from reactranker_amd import functions as Fn
from oracle import ref_cpu as O
from tests import graph_shapes as G
from tests.test_gpu_headline_kernels import train_step_vs_fp64_oracle
from tests.test_gpu_model import close, make_model
from tests.test_gpu_plan import _run, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["bf16x3", "f16x2"])
def arith(request):
    """The encoder GEMMs' arithmetic (functions.SplitGemm.f16), restored afterwards."""
    old = Fn.SplitGemm.f16
    Fn.SplitGemm.f16 = request.param == "f16x2"
    try:
        yield request.param
    finally:
        Fn.SplitGemm.f16 = old


@pytest.fixture
def three_term():
    old = Fn.SplitGemm.f16
    Fn.SplitGemm.f16 = False
    try:
        yield
    finally:
        Fn.SplitGemm.f16 = old


def _cfg(H, depth, evidential=False):
    return dict(hidden_size=H, mpnn_depth=depth, mpnn_diff_depth=depth, ffn_depth=3, use_bias=True, task_num=2 if evidential else 1,
                ffn_last_layer="no_softplus" if evidential else "with_softplus", task_type="evidential_ranking" if evidential else None,
                add_features_dim=1)


@functools.lru_cache(maxsize=None)
def _batch(name):
    qb, K = G.make(name)
    return qb, K, featurization.BatchMolGraph(qb.r_specs, K=K), featurization.BatchMolGraph(qb.p_specs, K=K)


@functools.lru_cache(maxsize=None)
def _weights(H, depth, evidential=False):
    c = _cfg(H, depth, evidential)
    return synth.seeded_weights(O.model_shapes(H, depth, depth, 3, c["task_num"], 1, True), 5)


@functools.lru_cache(maxsize=None)
def _eval_oracle64(name, K):
    """Eval-mode scores of the float64 oracle for the H = 32, depth 3 model (computed once per batch and pad width)."""
    qb = _batch(name)[0]
    P = {k: v.double() for k, v in O.params_from_numpy(_weights(32, 3)).items()}

    def gt(specs):
        g = O.graph_tensors(O.pack_batch(specs, K=K))
        g["f_atoms"], g["f_bonds"] = g["f_atoms"].double(), g["f_bonds"].double()
        return g
    return O.reaction_forward(P, dict(depth=3, diff_depth=3, ffn_depth=3, task_type="with_softplus"), gt(qb.r_specs), gt(qb.p_specs),
                              torch.tensor(qb.add_features).double()).detach()


@pytest.mark.parametrize("dedup", ["auto", False])
@pytest.mark.parametrize("name", G.NAMES)
def test_eval_forward_against_the_fp64_oracle(name, dedup, arith):
    qb, K, rb, pb = _batch(name)
    model = make_model(_cfg(32, 3), _weights(32, 3)).eval()
    model.dedup_reactants = dedup
    with torch.no_grad():
        out = model(rb, pb, gpu=0, add_features=qb.add_features)
    close(out, _eval_oracle64(name, K), tol=1e-5, what=f"{name} eval scores (dedup {dedup}, {arith})")


TRAIN = ([(n, 32, 3, False) for n in G.NAMES] + [(n, 300, 3, False) for n in ("wide6", "lone", "ragged")] +
         [(n, 32, 5, False) for n in ("wide6", "ragged")] + [("wide6", 32, 3, True)])


@pytest.mark.parametrize("name,H,depth,evidential", TRAIN)
def test_train_step_against_the_fp64_oracle(name, H, depth, evidential, arith, parity_log):
    """Train mode, dropout 0.1, step plan, shared reactant prefix: scores, loss and EVERY parameter gradient against the fp64
    oracle with identical dropout masks (depth 5: the multi-source gather over the copies of the shared-prefix backward)."""
    qb, K, rb, pb = _batch(name)
    parity_log(f"{name}: scope {qb.scope}, {rb.n_atoms} atom rows, {rb.n_bonds} / {pb.n_bonds} bond rows, K {rb.max_num_bonds} / "
               f"{pb.max_num_bonds}, H {H} depth {depth}, {arith}")
    train_step_vs_fp64_oracle(_cfg(H, depth, evidential), qb, K, "evidential" if evidential else "mle", 0.1, seed=700 + H + depth,
                              log=parity_log)


@pytest.mark.parametrize("dedup", ["auto", False])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("name", G.NAMES)
def test_plan_is_bit_identical_to_the_per_op_path(name, train, dedup, three_term):
    """Scores, loss and every gradient of the step plan (csrc/plan.hip) equal the per-op path's, in all three reactant modes."""
    qb, K, rb, pb = _batch(name)
    model = make_model(_cfg(32, 3), _weights(32, 3), dropout=0.1 if train else 0.0)
    model = model.train() if train else model.eval()
    model.dedup_reactants = dedup
    a = _run(model, rb, pb, qb, 4242, plan=False)
    b = _run(model, rb, pb, qb, 4242, plan=True)
    _same(a, b)
    _same(b, _run(model, rb, pb, qb, 4242, plan=True))


@pytest.mark.parametrize("name,depth", [("wide6", 5), ("ragged", 5), ("wide6", 3)])
def test_plan_is_bit_identical_to_the_per_op_path_h300(name, depth, three_term):
    qb, K, rb, pb = _batch(name)
    model = make_model(_cfg(300, depth), _weights(300, depth), dropout=0.1).train()
    a = _run(model, rb, pb, qb, 99, plan=False)
    _same(a, _run(model, rb, pb, qb, 99, plan=True))


def test_wider_pad_width_changes_the_scores_and_each_matches_its_own_oracle(arith):
    """Hazard H1 with real padding columns in every table: the same molecules packed with K = 8 score differently from their
    natural pad width (by more than 1e-4), and each packing matches the oracle run with that width."""
    qb = _batch("padded8")[0]
    model = make_model(_cfg(32, 3), _weights(32, 3)).eval()
    outs = {}
    for K in (None, 8):
        rb, pb = featurization.BatchMolGraph(qb.r_specs, K=K), featurization.BatchMolGraph(qb.p_specs, K=K)
        assert rb.max_num_bonds == (8 if K else 4)
        with torch.no_grad():
            outs[K] = model(rb, pb, 0, qb.add_features)
        close(outs[K], _eval_oracle64("padded8", K), tol=1e-5, what=f"padded8 K={K} ({arith})")
    assert float((outs[None] - outs[8]).abs().max()) > 1e-4
