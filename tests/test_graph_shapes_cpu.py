"""The hand-built batches of tests/graph_shapes.py really have the shapes they are named after (checked on the packer's host
tables, no GPU), and the oracle takes them: finite scores, loss and gradients in float32 and float64."""
import numpy as np
import pytest
import torch

from reactranker_amd import featurization, synth
from oracle import ref_cpu as O
from tests import graph_shapes as G


def _packed(name):
    qb, K = G.make(name)
    return qb, K, featurization.BatchMolGraph(qb.r_specs, K=K), featurization.BatchMolGraph(qb.p_specs, K=K)


def test_every_batch_has_the_shape_it_is_named_after():
    for name in G.NAMES:
        qb, K, rb, pb = _packed(name)
        assert sum(qb.scope) == len(qb.r_specs) == len(qb.p_specs) <= 80
        assert rb.n_atoms == pb.n_atoms and all(p.f_atoms is r.f_atoms for r, p in zip(qb.r_specs, qb.p_specs))
        for b in (rb, pb):                                 # the backward tables the packer derives: widths and pad counts
            h = b._host
            assert h["b2b_t"].shape == (b.n_bonds, max(1, b.max_num_bonds - 1))
            deg = (h["a2b"] > 0).sum(1)
            assert np.array_equal(h["npad"][1:], b.max_num_bonds - deg[1:])
    qb, K, rb, pb = _packed("wide6")
    assert (rb.max_num_bonds, pb.max_num_bonds) == (6, 6) and rb._host["b2b_t"].shape[1] == 5
    assert (rb._host["b2b_t"] >= 0).all(1).any() and (pb._host["b2b_t"] >= 0).all(1).any()      # a full five-wide row on both sides
    assert sorted(np.bincount(qb.r_specs[0].edges.reshape(-1)))[-2:] == [5, 6]                     # a degree-5 atom beside the hub
    qb, K, rb, pb = _packed("wide5")
    assert (rb.max_num_bonds, pb.max_num_bonds) == (5, 5) and (rb._host["b2b_t"] >= 0).all(1).any()
    qb, K, rb, pb = _packed("lone")
    assert any(s.n_atoms == 1 for s in qb.r_specs) and any(s.n_atoms > 1 for s in qb.r_specs) and 1 in qb.scope
    qb, K, rb, pb = _packed("lone_only")
    assert (rb.n_bonds, pb.n_bonds, rb.max_num_bonds) == (1, 1, 1) and all(s.n_atoms == 1 for s in qb.r_specs)
    qb, K, rb, pb = _packed("pairs")
    assert rb.max_num_bonds == pb.max_num_bonds == 1 and (rb._host["b2b_t"] == -1).all() and (pb._host["b2b_t"] == -1).all()
    assert any(r.n_bonds == 2 and p.n_bonds == 0 for r, p in zip(qb.r_specs, qb.p_specs))       # a product that lost its only bond
    assert any(r.n_bonds == 0 and p.n_bonds == 2 for r, p in zip(qb.r_specs, qb.p_specs))
    qb, K, rb, pb = _packed("fragments")
    comps = {G.n_components(s) for s in qb.r_specs}
    assert {2, 3} <= comps and any(G.n_components(p) < G.n_components(r) for r, p in zip(qb.r_specs, qb.p_specs))
    qb, K, rb, pb = _packed("padded8")
    assert K == 8 and rb.max_num_bonds == 8 and max(G.max_degree(s) for s in qb.r_specs + qb.p_specs) <= 4
    qb, K, rb, pb = _packed("ragged")
    assert qb.scope == [1, 70, 1, 2] and rb.unique_bonds()[1].shape[1] == 70


@pytest.mark.parametrize("name", G.NAMES)
def test_the_oracle_takes_every_batch(name):
    qb, K = G.make(name)
    w = synth.seeded_weights(O.model_shapes(32, 3, 3, 3, 1, 1, True), 5)
    outs = []
    for dt in (torch.float32, torch.float64):
        P = {k: v.detach().to(dt).requires_grad_(v.requires_grad) for k, v in O.params_from_numpy(w, requires_grad=True).items()}

        def gt(specs):
            g = O.graph_tensors(O.pack_batch(specs, K=K))
            g["f_atoms"], g["f_bonds"] = g["f_atoms"].to(dt), g["f_bonds"].to(dt)
            return g
        out = O.reaction_forward(P, dict(depth=3, diff_depth=3, ffn_depth=3, task_type="with_softplus"), gt(qb.r_specs), gt(qb.p_specs),
                                 torch.tensor(qb.add_features).to(dt))
        loss = O.listmle_loss(out, qb.scope, torch.tensor(qb.targets).to(dt))
        names = [k for k in P if P[k].requires_grad]
        grads = torch.autograd.grad(loss.sum(), [P[k] for k in names], allow_unused=True)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(loss).all())
        assert all(g is None or bool(torch.isfinite(g).all()) for g in grads)
        outs.append(out.detach().double())
    assert float((outs[0] - outs[1]).abs().max()) < 1e-4
