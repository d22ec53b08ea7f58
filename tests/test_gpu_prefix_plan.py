"""A shared-prefix (RR_STEP_PREFIX) training step through the step plan with the fused sum over the copies of the backward
(rr_gather2_sum_dropmask_f32) and with RR_NO_PREFIX_FUSE=1, which restores the two launches it replaces: scores, loss and
every gradient torch.equal - and both equal to the per-op path of reactranker_amd/functions.py under the criterion of
tests/test_gpu_plan.py (bit-identical).  (The forward's rr_gather_sum_dropsrc_f32 is not wired into the plan: it was not faster
stand-alone than the gather it would replace, profiles/prefix_fuse_ab.txt.)

Depth 2: the inner table of the two-level sum is b2t (K = 1); 3: the headline's; 4 and 6: two and four per-copy layers (their
dZ still summed by the separate rr_gather_sum_multi_f32 launch - the second accumulator was not built); 8: more than four.

The model enters prefix mode only when a reactant repeats inside the batch, so an outer width of 1 cannot be reached through
it: the batch of single-candidate queries runs (and is held equal) in plain mode, the batch [1, 2] gives a transposed copy
table of width 2 whose first reactant fills one column; width 1 itself is covered in tests/test_gpu_prefix_gathers.py."""
import pytest
import torch

from reactranker_amd import featurization, synth
from reactranker_amd import functions as Fn
from oracle import ref_cpu as O
from tests.test_gpu_model import make_model
from tests.test_gpu_plan import _run, _same

pytestmark = pytest.mark.gpu

BATCHES = {
    "q3": (21, 3, [4, 3, 5]),
    "q2": (22, 2, [5, 3]),
    "single_and_pair": (23, 2, [1, 2]),
    "singles": (24, 3, [1, 1, 1]),
}


def _model(H, d, p=0.1):
    cfg = dict(hidden_size=H, mpnn_depth=d, mpnn_diff_depth=2, ffn_depth=2, use_bias=True, task_num=1,
               ffn_last_layer="with_softplus", task_type=None, add_features_dim=1)
    w = synth.seeded_weights(O.model_shapes(H, d, 2, 2, 1, 1, True), 5)
    return make_model(cfg, w, dropout=p).train()


def _batch(name):
    seed, nq, nc = BATCHES[name]
    qb = synth.make_queries(seed, nq, nc, atoms_lo=5, atoms_hi=8)
    return qb, featurization.BatchMolGraph(qb.r_specs, K=4), featurization.BatchMolGraph(qb.p_specs, K=4)


def _three_ways(model, batch, monkeypatch):
    qb, rb, pb = batch
    fused = _run(model, rb, pb, qb, 7, plan=True)
    per_op = _run(model, rb, pb, qb, 7, plan=False)
    monkeypatch.setenv("RR_NO_PREFIX_FUSE", "1")
    unfused = _run(model, rb, pb, qb, 7, plan=True)
    monkeypatch.delenv("RR_NO_PREFIX_FUSE")
    _same(fused, unfused)
    _same(fused, per_op)
    return fused


@pytest.mark.parametrize("d", [2, 3, 4, 6, 8])
@pytest.mark.parametrize("H", [32, 300])
@pytest.mark.parametrize("streams", [True, False])
def test_fused_prefix_step_equals_the_unfused_step_and_the_per_op_path(d, H, streams, monkeypatch):
    model = _model(H, d)
    monkeypatch.setattr(Fn.SideStream, "enabled", streams)
    monkeypatch.setattr(Fn.AuxStream, "enabled", streams)
    for name in ("q3", "q2") if H == 32 else ("q3",):
        _three_ways(model, _batch(name), monkeypatch)


@pytest.mark.parametrize("name", ["single_and_pair", "singles"])
def test_fused_prefix_step_on_narrow_copy_tables(name, monkeypatch):
    batch = _batch(name)
    bmap_t = batch[1].unique_bonds()[1]
    assert bmap_t.shape[1] == (2 if name == "single_and_pair" else 1)
    for d in (2, 3):
        _three_ways(_model(32, d), batch, monkeypatch)


def test_the_knob_changes_nothing_on_the_two_f16_term_layout(monkeypatch):
    """That layout keeps today's launches (it needs their magnitude outputs): with and without the knob the same kernels run."""
    monkeypatch.setattr(Fn.SplitGemm, "f16", True)
    model = _model(64, 3)
    qb, rb, pb = _batch("q3")
    a = _run(model, rb, pb, qb, 7, plan=True)
    monkeypatch.setenv("RR_NO_PREFIX_FUSE", "1")
    _same(a, _run(model, rb, pb, qb, 7, plan=True))


def test_the_dropout_seed_still_changes_the_fused_step():
    model = _model(32, 3)
    qb, rb, pb = _batch("q3")
    a, b = _run(model, rb, pb, qb, 7, plan=True), _run(model, rb, pb, qb, 8, plan=True)
    assert not torch.equal(a[0], b[0])
