"""CPU-side checks of the pairwise trainer's remaining strategies (BetaNet, BetaNet_envidential, the baseline pair model):
the new entry points are exported, bound and reject bad arguments before any launch; run_train's selectors; the pair order
of reactranker_amd.pairs and the float64 restatements of tests/pairwise_variants_ref.py against vectors the reference itself
produced (tests/golden/pairwise_variants.npz, written by tools/make_golden_pairwise_variants.py); state-dict compatibility of
the pair model with base_model."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import pairwise_variants_ref as R

from reactranker_amd import _lib, base_model, pairs, ranknet_baseline, synth
from reactranker_amd import run_train_pairwise as RT

NEW_SYMBOLS = ["rr_betanet_fwd_f32", "rr_betanet_bwd_f32", "rr_beta_evidential_fwd_f32", "rr_beta_evidential_bwd_f32",
               "rr_pairwise_eval_f32", "rr_pair_partial_count", "rr_pair_softmax_mse_fwd_f32", "rr_pair_softmax_mse_bwd_f32",
               "rr_pair_acc_f32", "rr_pair_combine_f32"]


@pytest.fixture(scope="module")
def V(golden_dir):
    return np.load(os.path.join(golden_dir, "pairwise_variants.npz"))


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert a.shape == b.shape
    return float(np.max(np.abs(a - b) / (1 + np.abs(b)))) if a.size else 0.0


def test_new_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(raw, s), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert getattr(_lib.lib(), s).argtypes is not None
    assert _lib.lib().rr_version() == _lib.ABI_VERSION == 8          # additive: new symbols only


def test_entry_points_reject_bad_arguments_before_any_launch():
    l = _lib.lib()
    one = ctypes.c_void_p(256)
    for fwd, bwd, param in ((l.rr_betanet_fwd_f32, l.rr_betanet_bwd_f32, 100.0),
                            (l.rr_beta_evidential_fwd_f32, l.rr_beta_evidential_bwd_f32, 0.01)):
        assert fwd(None, 1, one, one, 1, 4, param, one, one, one, None) == -1          # null scores
        assert fwd(one, 1, one, None, 1, 4, param, one, one, one, None) == -1          # null seg_off
        assert fwd(one, 1, one, one, 1, 4, param, one, one, None, None) == -1          # null partials
        assert fwd(one, 0, one, one, 1, 4, param, one, one, one, None) == -1           # stride < 1
        assert fwd(one, 1, one, one, -1, 4, param, one, one, one, None) == -1          # Q < 0
        assert fwd(one, 1, one, one, 1, 8193, param, one, one, one, None) == -4        # list too long
        assert bwd(one, 1, one, one, 1, 4, param, None, one, 1, None) == -1            # null upstream gradient
        assert bwd(one, 1, one, one, 1, 4, param, one, one, 0, None) == -1             # gradient stride < 1
        assert bwd(one, 1, one, one, 1, 8193, param, one, one, 1, None) == -4
        assert bwd(one, 1, one, one, 0, 4, param, one, one, 1, None) == 0              # no queries: nothing launched
    assert l.rr_betanet_fwd_f32(one, 1, one, one, 1, 4, 0.0, one, one, one, None) == -1          # alpha0 must be positive
    assert l.rr_pairwise_eval_f32(one, 1, one, one, 1, 4, 1.0, None, one, None) == -1
    assert l.rr_pairwise_eval_f32(one, 1, one, one, -1, 4, 1.0, one, one, None) == -1
    assert l.rr_pairwise_eval_f32(one, 1, one, one, 1, 8193, 1.0, one, one, None) == -4
    assert l.rr_pair_softmax_mse_fwd_f32(one, 1, one, 2, 4, one, one, None) == -1                 # rows hold two columns
    assert l.rr_pair_softmax_mse_fwd_f32(one, 2, None, 2, 4, one, one, None) == -1
    assert l.rr_pair_softmax_mse_bwd_f32(one, 2, one, 2, 4, one, one, 1, None) == -1
    assert l.rr_pair_softmax_mse_bwd_f32(one, 2, one, 2, 0, one, one, 2, None) == 0               # no pairs: nothing launched
    assert l.rr_pair_acc_f32(one, 2, one, 2, 0, one, None) == -1                                  # a mean over no pair
    assert l.rr_pair_acc_f32(one, 2, one, 2, 4, None, None) == -1
    assert l.rr_pair_combine_f32(None, one, one, 32, None, None, None, 4, 32, one, 32, None) == -1
    assert l.rr_pair_combine_f32(one, one, one, 16, None, None, None, 4, 32, one, 32, None) == -1  # pitch below the width
    assert l.rr_pair_combine_f32(one, one, one, 32, None, None, None, 4, 30, one, 32, None) == -2  # RR_ERR_ALIGN: H % 4
    assert l.rr_pair_combine_f32(ctypes.c_void_p(260), one, one, 32, None, None, None, 4, 32, one, 32, None) == -2
    assert l.rr_pair_combine_f32(one, one, one, 32, None, None, None, 0, 32, one, 32, None) == 0   # no rows: nothing launched
    assert l.rr_pair_partial_count(0) >= 1 and l.rr_pair_partial_count(10 ** 7) <= 1024


def test_run_train_selectors():
    assert RT.select_loop("baseline", "baseline") == "pair_baseline"
    assert RT.select_loop("sum_session", "baseline") == "sum_session"
    assert RT.select_loop("accelerate_grad", "baseline") == "accelerate_grad"
    assert RT.select_loop("sum_session", "BetaNet") == "BetaNet"
    assert RT.select_loop("anything", "BetaNet_envidential") == "BetaNet_envidential"
    for bad in (("sum_sessions", "baseline"), ("sum_session", "betanet"), ("baseline", "listnet")):
        with pytest.raises(ValueError, match="pairwise selectors"):
            RT.select_loop(*bad)
    with pytest.raises(ValueError, match="pairwise selectors"):          # refused before anything touches a device
        RT.run_train(None, None, [], [], None, None, 1, 0, 0, train_strategy="nope", task_type="baseline")
    with pytest.raises(ValueError, match="epochs >= 2"):                 # the reference's ZeroDivisionError, said up front
        RT.run_train(None, None, [], [], None, None, 1, 0, 0, task_type="BetaNet_envidential")


def test_pair_order_equals_the_reference(V):
    for name in V["order_cases"].tolist():
        t = V[f"order.{name}.targets"]
        ii, jj = pairs.query_pairs(t)
        assert ii.tolist() == V[f"order.{name}.i"].tolist(), name
        assert jj.tolist() == V[f"order.{name}.j"].tolist(), name
        ri, rj = R.query_pair_order(t)
        assert ri.tolist() == ii.tolist() and rj.tolist() == jj.tolist()
    assert len(V["order.one_value.i"]) == 0 and len(V["order.single.i"]) == 0       # one distinct value: no pairs
    assert len(V["order.tied.i"]) == 22                                             # 6 rows, values x3 x2 x1: 30 - 6 - 2


def test_pair_windows_batches_and_indices(V):
    scope = V["pair.scope"].tolist()
    hidden, d, dd, fd, tn, seed, wseed, B = V["pair.cfg"].tolist()
    qb = synth.make_queries(seed, len(scope), scope, atoms_lo=5, atoms_hi=10)
    t = V["pair.targets"]
    batches = list(pairs.pair_windows(qb.r_specs, qb.p_specs, scope, t, B))
    ii = np.concatenate([b["pairs"][0] for b in batches])
    jj = np.concatenate([b["pairs"][1] for b in batches])
    assert ii.tolist() == V["pair.i"].tolist() and jj.tolist() == V["pair.j"].tolist()
    assert [len(b["targets"]) for b in batches] == [B, len(ii) - B] and [b["full"] for b in batches] == [True, False]
    for b in batches:
        assert np.array_equal(b["targets"], np.stack([t[b["pairs"][0]], t[b["pairs"][1]]], axis=1))
        u, ir, i1, i2 = b["index"]
        assert b["r"].max_num_bonds == b["p1"].max_num_bonds == b["p2"].max_num_bonds == u.max_num_bonds
        assert b["r"].n_atoms == b["p1"].n_atoms == b["p2"].n_atoms == len(ir) == len(i1) == len(i2)
        assert ir[0] == i1[0] == i2[0] == 0
        # the rows the indices name hold the same atoms
        fu = u._host["f_atoms"]
        for g, ix in ((b["r"], ir), (b["p1"], i1), (b["p2"], i2)):
            assert np.array_equal(g._host["f_atoms"][1:], fu[ix[1:]])
        assert u.n_mols < b["r"].n_mols + b["p1"].n_mols + b["p2"].n_mols
    assert list(pairs.pair_windows(qb.r_specs[:2], qb.p_specs[:2], [2], [1.0, 1.0], 4)) == []


def test_float64_restatements_reproduce_the_reference(V):
    """Evaluated in float32 the restatements ARE the reference's formula, to rounding (1e-6).  In float64 they sit where
    float32 rounding puts the reference: BetaNet's lt - lp adds six terms of magnitude up to lgamma(100) = 359, each rounded
    to 2^-24 relative (6 * 359 * 6e-8 = 1.3e-4 per entry), weighted with a Beta density of up to ~8 at alpha0 = 100 and
    averaged over as few as two entries: 1e-3.  The evidential form has no cancellation: a few float32 roundings, 2e-6."""
    a0 = float(V["alpha0"])
    mc, ep, eps = V["evi_args"].tolist()
    coef = mc * (ep / (eps - 1)) ** 3
    for name in V["sq_cases"].tolist():
        P = f"sq.{name}."
        scope, t = V[P + "scope"].tolist(), V[P + "targets"]
        for key, x, param, tol in (("betanet", V[P + "score"], a0, 1e-3), ("beta_evidential", V[P + "pos"], coef, 2e-6)):
            loss, npairs, g = R.sq_loss(key, x, scope, t, param)
            assert npairs == sum(c * c - c for c in scope)
            assert rel(loss / npairs, V[P + key]) <= tol, (name, key)
            assert rel(g / npairs, V[P + key + "_g"]) <= tol, (name, key)
            # and the same restatement evaluated in float32 is the reference to rounding
            l32, _, g32 = R.sq_loss(key, x, scope, t, param, dtype=torch.float32)
            assert rel(l32 / npairs, V[P + key]) <= 1e-6 and rel(g32 / npairs, V[P + key + "_g"]) <= 1e-6, (name, key)
    acc, ce, rows = R.pairwise_stats(V["eval.scores"], V["eval.scope"].tolist(), V["eval.targets"], float(V["eval.sigma"]))
    assert abs(acc - float(V["eval.pairwise_acc"])) <= 1e-6
    assert rel(ce, V["eval.cross_entropy"]) <= 1e-5
    assert (rows[:, 0] > 0).tolist() == V["eval.used"].tolist()
    off, accs = 0, []
    for b in V["pairacc.sizes"].tolist():
        accs.append(R.pair_acc(V["pairacc.y"][off:off + b], V["pairacc.t"][off:off + b]))
        off += b
    assert abs(np.mean(accs) - float(V["pairacc.acc"])) <= 1e-6


def test_targets_of_the_eval_fixture_are_exact_in_float32(V):
    for k in ("eval.targets", "eval.scores", "pairacc.t", "pairacc.y", "pair.targets"):
        a = V[k]
        assert a.dtype == np.float32 and np.array_equal(np.round(a.astype(np.float64) * 8) / 8, a.astype(np.float64)), k


def test_pair_model_shares_the_state_dict_of_base_model():
    kw = dict(hidden_size=32, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.1, task_num=2)
    pair = ranknet_baseline.build_model(ffn_last_layer="evidential", **kw)
    base = base_model.build_model(ffn_last_layer="no_softplus", **kw)
    sd_p, sd_b = pair.state_dict(), base.state_dict()
    assert len(sd_p) == 20 and list(sd_p) == list(sd_b)
    assert all(sd_p[k].shape == sd_b[k].shape for k in sd_p)
    pair.load_state_dict(sd_b)
    assert all(torch.equal(pair.state_dict()[k], sd_b[k]) for k in sd_b)
    base.load_state_dict(ranknet_baseline.build_model(ffn_last_layer="evidential", **kw).state_dict())
    # head strings as the reference forms them (models/ranknet_baseline.py:79-86)
    assert pair.ffn.task_type == "evidential"
    assert ranknet_baseline.build_model(task_num=2, ffn_last_layer="with_softplus", hidden_size=32).ffn.task_type == "gaussian_with_softplus"
    assert ranknet_baseline.build_model(task_num=4, ffn_last_layer="with_softplus", hidden_size=32).ffn.task_type == "evidential_with_softplus"
    assert ranknet_baseline.build_model(task_num=1, ffn_last_layer="no_softplus", hidden_size=32).ffn.task_type == "no_softplus"


def test_row_blocked_restatements_equal_the_unblocked_ones(V):
    """sq_loss(block=...) / pairwise_stats(block=...) evaluate a query's C x C arrays a few rows at a time (the long-list GPU
    tests need that: 5462^2 float64 entries, twenty times over under autograd).  Same terms, summed block by block: float64
    agreement to 1e-12 relative on the golden sq.c300 case, for a block that does not divide 300; the integer counts of
    pairwise_stats exactly."""
    a0 = float(V["alpha0"])
    mc, ep, eps = V["evi_args"].tolist()
    coef = mc * (ep / (eps - 1)) ** 3
    P = "sq.c300."
    scope, t = V[P + "scope"].tolist(), V[P + "targets"]
    for key, x, param in (("betanet", V[P + "score"], a0), ("beta_evidential", V[P + "pos"], coef)):
        l0, n0, g0 = R.sq_loss(key, x, scope, t, param)
        l1, n1, g1 = R.sq_loss(key, x, scope, t, param, block=64)
        assert n0 == n1
        assert abs(l1 - l0) <= 1e-12 * abs(l0), key
        assert np.max(np.abs(g1 - g0)) <= 1e-12 * np.max(np.abs(g0)), key
    a, c, rows = R.pairwise_stats(V["eval.scores"], V["eval.scope"].tolist(), V["eval.targets"], float(V["eval.sigma"]))
    ab, cb, rows_b = R.pairwise_stats(V["eval.scores"], V["eval.scope"].tolist(), V["eval.targets"], float(V["eval.sigma"]), block=3)
    assert np.array_equal(rows[:, :2], rows_b[:, :2]) and a == ab
    assert np.max(np.abs(rows[:, 2] - rows_b[:, 2])) <= 1e-12 * np.max(np.abs(rows[:, 2])) and abs(c - cb) <= 1e-12 * abs(c)
