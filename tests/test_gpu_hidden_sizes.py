"""The assembled model at every hidden size a dispatcher branches on (tests/hidden_sizes.py: the ladder and what each rung
crosses - split geometry, f32 layout above 608, FFN-chain instantiation and per-wave tile counts, 64 KiB of LDS, plan / no plan).
The kernel-level suites hold each leaf against f64 with synthetic operands; the model-level suites only use H in
{30, 32, 50, 64, 300, 600}.  Here, per rung:
  - one training step (train mode, dropout 0.1, depth 2 / 2, three FFN layers, biases, one appended feature) against the fp64
    oracle with identical dropout masks: scores, loss and every gradient, gate flips separated from rounding
    (tests/test_gpu_headline_kernels.py: train_step_vs_fp64_oracle, its bounds) - H % 4 != 0 on the per-op path with the bounds of
    tests/test_gpu_model.py: test_train_mode_dropout_matches_oracle_with_same_masks;
  - the FFN chain's status as the table predicts it (0, or -4 at 644 and 1024) and, where it runs, torch.equal against the
    layers issued one by one at M = 515 - a partial row tile and several workgroups in front of every tile-count branch;
  - forward chains of growing LDS demand inside one process (launch_chain's opt-in must not depend on the first size seen).
All in the library's default arithmetic; tests/test_gpu_plan.py and tests/test_gpu_f16x2.py run the same rungs plan against
per-op mirror and two-term against three-term."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from reactranker_amd import featurization, synth
from reactranker_amd import functions as Fn
from reactranker_amd import loss as RL
from tests import hidden_sizes as L
from tests.test_gpu_ffn import _chain_backward, _chain_forward, _layers
from tests.test_gpu_headline_kernels import train_step_vs_fp64_oracle
from tests.test_gpu_model import _masks_for, close, make_model

pytestmark = pytest.mark.gpu
dev = "cuda"


def _cfg(H, F=1, evidential=False):
    return dict(hidden_size=H, mpnn_depth=2, mpnn_diff_depth=2, ffn_depth=3, use_bias=True, task_num=2 if evidential else 1,
                ffn_last_layer="no_softplus" if evidential else "with_softplus", task_type="evidential_ranking" if evidential else None,
                add_features_dim=F)


def _batch(F=1):
    """the 24-candidate batch of tests/test_gpu_plan.py, with F appended feature columns (F = 1: its own)"""
    qb = synth.make_queries(17, 4, [7, 3, 9, 5], atoms_lo=5, atoms_hi=14)
    if F == 1:
        return qb
    add = None if F == 0 else np.random.default_rng(170 + F).random((len(qb.p_specs), F)).astype(np.float32)
    return dataclasses.replace(qb, add_features=add)


def _summary(log, what, r):
    log(f"{what}: scores {r['scores']:.2e} (fp32 oracle {r['scores32']:.2e}), loss {r['loss']:.2e} (fp32 oracle {r['loss32']:.2e}), worst "
        f"gradient / its tensor's max {r['grad']:.2e} at {r['grad_at']}, {r['flips']} of {r['gates']} gates flipped")


@pytest.mark.parametrize("H", L.RUNGS_MULT4)
def test_train_step_against_the_fp64_oracle_at_every_rung(H, parity_log):
    geo, plan, chain, counts, lds = L.LADDER[H]
    assert plan
    r = train_step_vs_fp64_oracle(_cfg(H), _batch(), 4, "mle", 0.1, 700 + H, parity_log)
    _summary(parity_log, f"H {H} [{geo}, chain {chain}, tiles per wave {counts}, LDS {lds}]", r)


@pytest.mark.parametrize("H", [200, 608])
def test_train_step_with_the_evidential_ranking_head(H, parity_log):
    r = train_step_vs_fp64_oracle(_cfg(H, evidential=True), _batch(), 4, "evidential", 0.1, 900 + H, parity_log)
    _summary(parity_log, f"H {H} evidential_ranking", r)


@pytest.mark.parametrize("H,F", [(h, f) for h in (64, 300) for f in (0, 3, 4)])
def test_train_step_with_zero_three_and_four_appended_features(H, F, parity_log):
    """ffn[0].in = H + F: 0 and 3 (mod 4) next to the 1 (mod 4) of every other model-level test"""
    r = train_step_vs_fp64_oracle(_cfg(H, F=F), _batch(F), 4, "mle", 0.1, 800 + H + F, parity_log)
    _summary(parity_log, f"H {H} F {F}", r)


@pytest.mark.parametrize("H", L.RUNGS_ODD)
def test_train_step_without_a_plan_against_the_fp64_oracle(H, parity_log):
    """H % 4 != 0: the per-op path (no plan, so no saved gates to dictate), f32 layout, scalar gathers, materialised masks.
    Scores and loss within 1e-5 (1 + |ref|), every gradient within 1e-4 of its tensor's largest entry + 1e-6."""
    p = 0.1
    cfg = _cfg(H)
    assert L.LADDER[H][:3] == (L.F32, False, L.PER_LAYER)
    w = synth.seeded_weights(O.model_shapes(H, 2, 2, 3, 1, 1, True), 700 + H)
    model = make_model(cfg, w, dropout=p).train()
    model.dropout_seed = 0xC0FFEE1234
    qb = _batch()
    rb, pb = featurization.BatchMolGraph(qb.r_specs, K=4), featurization.BatchMolGraph(qb.p_specs, K=4)
    scope, targets = qb.scope, torch.tensor(qb.targets)
    masks = _masks_for(model, model.dropout_seed, rb, pb, len(qb.p_specs), 1, p)
    dt = torch.float64
    P = {k: v.detach().to(dt).requires_grad_(v.requires_grad) for k, v in O.params_from_numpy(w, requires_grad=True).items()}

    def gt(specs):
        g = O.graph_tensors(O.pack_batch(specs, K=4))
        g["f_atoms"], g["f_bonds"] = g["f_atoms"].to(dt), g["f_bonds"].to(dt)
        return g
    mc = dict(depth=2, diff_depth=2, ffn_depth=3, task_type=O.resolve_task_type(1, "with_softplus", None), dropout=p)
    ref = O.reaction_forward(P, mc, gt(qb.r_specs), gt(qb.p_specs), torch.tensor(qb.add_features).to(dt),
                             masks={k: v.to(dt) for k, v in masks.items()})
    Fn.StepPlan.keep_last = True
    try:
        out = model(rb, pb, gpu=0, add_features=qb.add_features)
        assert Fn.StepPlan.last is None                    # no plan took this step
    finally:
        Fn.StepPlan.keep_last, Fn.StepPlan.last = False, None
    e_s = close(out, ref, tol=1e-5, what=f"H {H} train-mode out")
    l_ref = O.listmle_loss(ref, scope, targets.to(dt))
    l = RL.MLEloss()(out, scope, targets, 0)
    e_l = close(l, l_ref, tol=1e-5, what=f"H {H} train-mode loss")
    names = [k for k in P if P[k].requires_grad]
    g_ref = torch.autograd.grad(l_ref.sum(), [P[k] for k in names], allow_unused=True)
    l.sum().backward()
    got = dict(model.named_parameters())
    worst, at = 0.0, ""
    for k, gr in zip(names, g_ref):
        gr = torch.zeros_like(P[k]) if gr is None else gr
        g = got[k].grad
        g = torch.zeros_like(got[k]) if g is None else g
        err = float((g.detach().cpu().double() - gr).abs().max())
        scale = float(gr.abs().max())
        bound = 1e-4 * scale + 1e-6                       # + absolute floor for analytically-zero gradients
        if scale >= 1e-12 and err / scale > worst:
            worst, at = err / scale, k
        assert err <= bound, f"H {H} train grad {k}: |err| {err:.3e} > {bound:.3e}"
    parity_log(f"H {H} [no plan, f32 layout]: scores {e_s:.2e}, loss {e_l:.2e}, worst gradient / its tensor's max {worst:.2e} at {at} "
               f"(against the fp64 oracle's own gates)")
    model.eval()
    out_eval = model(rb, pb, gpu=0, add_features=qb.add_features)
    assert float((out_eval.detach() - out.detach()).abs().max()) > 1e-4      # dropout really acted


@pytest.mark.parametrize("H", L.RUNGS_MULT4)
def test_the_ffn_chain_takes_the_path_the_table_predicts(H, parity_log):
    """widths [H + 1, H, H, 1] at M = 515 (33 workgroups, the last with 3 rows): the status the table predicts, and where the
    chain runs, every layer's output and the input gradient bit for bit the per-layer launches'"""
    M, p = 515, 0.1
    widths = L.forward_widths(H)
    want, inst, counts, lds = L.chain_of(widths)
    bwant, binst, bcounts, blds = L.chain_of(L.backward_widths(H), rowdot=False)
    assert (want == 0) == (L.LADDER[H][2] != L.PER_LAYER) and bwant == want
    torch.manual_seed(H)
    K0 = widths[0]
    x = torch.randn(M, L.r4(K0), device=dev)
    layers = _layers(widths, True, 3)
    ref_out, saved = Fn.ffn_forward(x[:, :K0], layers, p, 91, 0)
    ref_hs, ref_raw = saved
    st, hs = _chain_forward(x, K0, layers, p, 91)
    assert st == want, (H, st, want)
    d = torch.randn(M, 1, device=dev)
    old = Fn.SideStream.enabled
    Fn.SideStream.enabled = False
    try:
        ref_dx, _ = Fn.ffn_backward(layers, p, 0, saved, d, need_dx=True, dx_cols=H)
    finally:
        Fn.SideStream.enabled = old
    bst, outs = _chain_backward(d, layers, ref_hs, p, H)
    assert bst == bwant, (H, bst, bwant)
    torch.cuda.synchronize()
    if want != 0:
        parity_log(f"H {H}: forward and backward chain refused with {st} / {bst}, as the table says")
        return
    for li in range(len(layers) - 1):
        n = widths[li + 1]
        assert torch.equal(hs[li][:, :n], ref_hs[li + 1][:, :n]), (H, li, float((hs[li][:, :n] - ref_hs[li + 1][:, :n]).abs().max()))
    assert torch.equal(hs[-1], ref_raw), (H, float((hs[-1] - ref_raw).abs().max()))
    assert float((ref_hs[1] == 0).float().mean()) > 0.3 and bool(torch.isfinite(ref_raw).all())
    assert torch.equal(outs[-1][:, :H], ref_dx), (H, float((outs[-1][:, :H] - ref_dx).abs().max()))
    parity_log(f"H {H}: chain <{inst[0]},{inst[1]}>, tiles per wave {sorted(counts)}, LDS {lds} B forward / {blds} B backward - "
               f"bit-identical to the per-layer launches at M = {M}")


ASCENDING = {
    (8, 1): [[600, 64, 1], [800, 64, 1], [1024, 64, 1]],
    (8, 3): [[600, 256, 1], [800, 256, 1], [1024, 256, 1]],
    (8, 5): [[513, 512, 512, 1], [601, 600, 600, 1], [641, 640, 640, 1], [1024, 640, 1]],
}


def test_growing_lds_demand_inside_one_process(parity_log):
    """Each instantiation's opt-in to more than 64 KiB of dynamic LDS is asked for once per device: a later launch of the same
    instantiation that needs MORE than the first one did must still run (a hidden-size sweep in one process: 512, then 600,
    then 640).  Every entry above 64 KiB, in ascending order per instantiation, then the smallest again; status 0 and the
    per-layer launches' bits."""
    M, p = 100, 0.1
    for inst, entries in ASCENDING.items():
        sizes = []
        for widths in entries + entries[:1]:
            st_want, got_inst, _, lds = L.chain_of(widths)
            assert st_want == 0 and got_inst == inst and lds > L.LDS_OPT_IN, (widths, got_inst, lds)
            sizes.append(lds)
            torch.manual_seed(widths[0] + widths[1])
            K0 = widths[0]
            x = torch.randn(M, L.r4(K0), device=dev)
            layers = _layers(widths, True, 7)
            _, (ref_hs, ref_raw) = Fn.ffn_forward(x[:, :K0], layers, p, 33, 0)
            st, hs = _chain_forward(x, K0, layers, p, 33)
            assert st == 0, (inst, widths, lds, st)
            for li in range(len(layers) - 1):
                n = widths[li + 1]
                assert torch.equal(hs[li][:, :n], ref_hs[li + 1][:, :n]), (widths, li)
            assert torch.equal(hs[-1], ref_raw), (widths, float((hs[-1] - ref_raw).abs().max()))
        assert sizes[:-1] == sorted(set(sizes[:-1])) and sizes[-1] == sizes[0]
        parity_log(f"<{inst[0]},{inst[1]}>: LDS {sizes} B in this order, every launch status 0 and bit-identical to the per-layer launches")
    assert ASCENDING[(8, 1)][-1][0] == L.CHAIN_KMAX and L.chain_of(ASCENDING[(8, 5)][-1])[3] == 131584
