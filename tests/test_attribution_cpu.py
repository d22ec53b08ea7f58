"""CPU-side checks of the attributions: the three new symbols declared, exported and bound; both entries
rejecting bad arguments before any launch; the Python layer's ValueErrors; the gate margin of every (fixture, node) the GPU
tests compare against the oracle; and the properties of the float64 restatement tests/attribution_ref.py alone.

Bounds.  Euler: a bias-free model with a raw head is positively homogeneous of degree one, so gradient x input sums to the
score exactly; in f64 the sum of a few thousand terms of size <= 1 leaves 1e-12 with three orders of margin.  Integrated
gradients: the midpoint rule's error falls at least linearly in the node count for a piecewise-smooth integrand, 16-fold
from 4 to 64 nodes; a factor 4 is asked."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import attribution_ref as AR

from reactranker_amd import _lib, featurization
from reactranker_amd.base_model import build_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rr_input_attribution_f32", "rr_input_attribution_max_k", "rr_attribution_reduce_f32"]


# ------------------------------------------------------------------------------------------------ symbols and statuses
def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(REPO, "include", "reactranker_hip.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\b(rr_\w+)\s*\(", text))
    assert re.search(r"#define\s+RR_ATTR_MAX_K\s+128\b", text) and re.search(r"#define\s+RR_ATTR_MAX_SEG\s+4\b", text)
    with open(os.path.join(REPO, "reactranker_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS\s*:=\s*(.*)$", f.read(), re.M).group(1).split()
    assert "attribution.hip" in srcs
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert getattr(_lib.lib(), s).argtypes is not None
    assert _lib.lib().rr_version() == _lib.ABI_VERSION == 8          # additive: new symbols only
    from reactranker_amd import attribution as A
    assert _lib.lib().rr_input_attribution_max_k() == A.MAX_K == 128


def _attr_args():
    one = ctypes.c_void_p(256)
    seg = (ctypes.c_int32 * 2)(61, 83)
    #        0 dz 1 ld  2 w 3 ld 4 x  5 ld 6 add 7 ld 8 idx 9 M 10 N 11 K 12 seg 13 n 14 alpha 15 acc 16 attr 17 ld 18 dx 19 ld 20 stream
    return [one, 300, one, 83, one, 84, one, 84, one, 4, 300, 83, seg, 2, 1.0, 0, one, 2, one, 83, None]


def test_input_attribution_rejects_bad_arguments_before_any_launch():
    fn = _lib.lib().rr_input_attribution_f32
    for k in (0, 2):                                                                  # required pointers
        a = _attr_args()
        a[k] = None
        assert fn(*a) == -1, k
    a = _attr_args()
    a[4] = None                                                                       # attr without x
    assert fn(*a) == -1
    a = _attr_args()
    a[16] = a[18] = None                                                              # both outputs null
    assert fn(*a) == -1
    a = _attr_args()
    a[12] = None                                                                      # attr without segments
    assert fn(*a) == -1
    for k in (6, 8):                                                                  # add and add_idx come together
        a = _attr_args()
        a[k] = None
        assert fn(*a) == -1, k
    for seg in ((83, 61), (61, 61), (61, 82), (61, 84), (0, 83)):                     # not ascending / not ending at K
        a = _attr_args()
        a[12] = (ctypes.c_int32 * 2)(*seg)
        assert fn(*a) == -1, seg
    for n_seg in (0, 5):
        a = _attr_args()
        a[12], a[13] = (ctypes.c_int32 * 5)(10, 20, 30, 40, 83), n_seg
        assert fn(*a) == -1, n_seg
    for k, bad in ((1, 299), (3, 82), (5, 82), (7, 82), (17, 1), (19, 82), (9, -1), (10, 0), (11, 0), (15, 2)):
        a = _attr_args()
        a[k] = bad                                                                    # a pitch below its width, bad sizes
        assert fn(*a) == -1, (k, bad)
    a = _attr_args()
    a[11], a[3], a[5], a[7], a[19], a[12] = 129, 129, 129, 129, 129, (ctypes.c_int32 * 2)(61, 129)
    assert fn(*a) == -4                                                               # K = 129: RR_ERR_UNSUPPORTED
    a = _attr_args()
    a[9] = 0
    assert fn(*a) == 0                                                                # no rows: nothing launched
    a = _attr_args()
    a[9], a[0] = 0, None
    assert fn(*a) == -1                                                               # ... and the checks come first


def test_attribution_reduce_rejects_bad_arguments_before_any_launch():
    fn = _lib.lib().rr_attribution_reduce_f32
    one = ctypes.c_void_p(256)
    #        0 fa 1 ld 2 fb 3 ld 4 a2b 5 b2revb 6 scope 7 nA 8 nB 9 M 10 K 11 atom 12 bond 13 sym 14 total 15 stream
    good = [one, 1, one, 2, one, one, one, 8, 9, 2, 4, one, one, one, one, None]
    for k in (0, 2, 4, 5, 6, 11, 12, 13, 14):
        a = list(good)
        a[k] = None
        assert fn(*a) == -1, k
    for k, bad in ((1, 0), (3, 1), (7, 0), (8, 0), (9, -1), (10, 0)):
        a = list(good)
        a[k] = bad
        assert fn(*a) == -1, (k, bad)


def _model(H=32, task_num=1, F=1):
    return build_model(hidden_size=H, mpnn_depth=2, mpnn_diff_depth=2, ffn_depth=3, dropout=0.0, task_num=task_num,
                       add_features_dim=F)


def test_python_layer_checks_its_arguments_without_a_gpu():
    from reactranker_amd import attribution as A
    qb = AR.batch()
    rb, pb = featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs)
    model = _model()
    feat = qb.add_features
    with pytest.raises(ValueError, match="grad_x_input"):
        A.attribute(model, rb, pb, feat, method="saliency")
    for steps in (0, -3, 2.5):
        with pytest.raises(ValueError, match="steps"):
            A.attribute(model, rb, pb, feat, method="integrated_gradients", steps=steps)
    for column in (1, -1, 0.0):
        with pytest.raises(ValueError, match=r"0\.\.0"):
            A.attribute(model, rb, pb, feat, column=column)
        with pytest.raises(ValueError, match=r"0\.\.0"):
            A.input_gradients(model, rb, pb, feat, column=column)
    with pytest.raises(ValueError, match=r"0\.\.1"):
        A.input_gradients(_model(task_num=2), rb, pb, feat, column=2)
    other = featurization.BatchMolGraph(qb.p_specs[:-1])
    with pytest.raises(ValueError, match="same molecules"):
        A.attribute(model, rb, other, feat)
    with pytest.raises(ValueError, match="width 1"):
        A.attribute(model, rb, pb, None)
    with pytest.raises(ValueError, match="width 1"):
        A.input_gradients(model, rb, pb, np.zeros((len(qb.p_specs), 2), np.float32))
    with pytest.raises(ValueError, match="width 0"):
        A.attribute(_model(F=0), rb, pb, feat)


# ------------------------------------------------------------------------------------------------ the fixtures' gate margin
@pytest.mark.parametrize("fx", AR.FIXTURES, ids=AR.fixture_id)
def test_fixture_gate_margins(fx):
    """Every (fixture, node) the GPU tests compare against the oracle keeps its smallest non-zero pre-activation at least
    1e-6 of its layer's largest - more than ten times the f32 forward error (2.9e-8) - so no ReLU gate can differ."""
    H, depth, dd, bias, ig = fx
    qb = AR.batch()
    w = AR.weights(H, depth, dd, bias)
    cfg = AR.cfg_of(depth, dd, "listnet_with_softplus")
    nodes = [1.0] + ([(s + 0.5) / AR.IG_STEPS for s in range(AR.IG_STEPS)] if ig else [])
    got = [AR.margin(AR.gradients(w, cfg, qb, 0, a)["trace"]) for a in nodes]
    print(AR.fixture_id(fx), " ".join(f"{m:.2e}" for m in got))
    assert min(got) >= AR.MIN_MARGIN, got


def test_extra_fixtures_gate_margins():
    """... and the same for the two-column, the feature-less and the bias-free fixtures of the GPU tests."""
    qb = AR.batch()
    for w, cfg, feats in ((AR.weights(64, 2, 2, True, task_num=2), AR.cfg_of(2, 2, "gaussian_with_softplus"), True),
                          (AR.weights(64, 2, 2, True, F=0), AR.cfg_of(2, 2, "listnet_with_softplus"), False),
                          (AR.zero_biases(AR.weights(64, 2, 2, True)), AR.cfg_of(2, 2, "no_softplus"), True)):
        m = AR.margin(AR.gradients(w, cfg, qb, 0, 1.0, feats)["trace"])
        assert m >= AR.MIN_MARGIN, m


# ------------------------------------------------------------------------------------------------ the restatement alone
@pytest.mark.parametrize("H", [32, 64])
def test_restatement_gradient_x_input_is_complete_without_biases(H):
    qb = AR.batch()
    w = AR.zero_biases(AR.weights(H, 2, 2, True))
    ref = AR.attribute(w, AR.cfg_of(2, 2, "no_softplus"), qb, method="grad_x_input")
    assert np.abs(ref["total"] - ref["score"]).max() <= 1e-12
    assert np.abs(ref["score"]).max() > 1e-3                                          # (not the identity 0 == 0)


def test_restatement_gradient_x_input_is_not_complete_with_biases():
    qb = AR.batch()
    ref = AR.attribute(AR.weights(64, 2, 2, True), AR.cfg_of(2, 2, "no_softplus"), qb, method="grad_x_input")
    assert np.abs(ref["total"] - ref["score"]).max() > 1e-3


@pytest.mark.parametrize("H", [32, 64])
def test_restatement_integrated_gradients_converge(H):
    qb = AR.batch()
    w, cfg = AR.weights(H, 2, 2, True), AR.cfg_of(2, 2, "no_softplus")
    gaps = {}
    for steps in (4, 64):
        ref = AR.attribute(w, cfg, qb, method="integrated_gradients", steps=steps)
        assert np.array_equal(ref["gap"], ref["total"] - (ref["score"] - ref["baseline_score"]))
        gaps[steps] = np.abs(ref["gap"]).max()
    print(f"H={H}: max |gap| {gaps[4]:.2e} at 4 nodes, {gaps[64]:.2e} at 64")
    assert gaps[64] < 0.25 * gaps[4]


def test_numpy_kernel_restatements_agree_with_einsum():
    rng = np.random.default_rng(5)
    M, N, K = 37, 30, 83
    dz, w, x = rng.standard_normal((M, N)), rng.standard_normal((N, K + 5)), rng.standard_normal((M, K + 1))
    add, idx = rng.standard_normal((6, K)), rng.integers(0, 6, M)
    attr0, dx0 = rng.standard_normal((M, 2)), rng.standard_normal((M, K))
    attr, dx = AR.np_input_attribution(dz, w, K, x, add, idx, (61, 83), 0.25, True, attr0, dx0)
    dX = np.einsum("mn,nk->mk", dz, w[:, :K]) + add[idx]
    want = np.stack([np.einsum("mk,mk->m", x[:, :61], dX[:, :61]), np.einsum("mk,mk->m", x[:, 61:K], dX[:, 61:])], 1)
    assert np.abs(attr - (attr0 + 0.25 * want)).max() <= 1e-12
    assert np.abs(dx - (dx0 + 0.25 * dX)).max() <= 1e-12
    # the finish on a real packed graph: every term lands in exactly one atom / one molecule
    from oracle import ref_cpu as O
    g = O.pack_batch(AR.batch().p_specs, K=6)                                          # a2b wider than every degree
    nA, nB = g["f_atoms"].shape[0], g["f_bonds"].shape[0]
    fa, fb = rng.standard_normal(nA), rng.standard_normal((nB, 2))
    fa[0], fb[0] = 0.0, 0.0
    atom, bond, sym, tot = AR.np_attribution_reduce(fa, fb, g["a2b"], g["b2revb"], g["a_scope"], dtype=np.float64)
    src = g["b2a"]
    want_atom = fa + np.bincount(src, weights=fb[:, 0], minlength=nA)
    assert np.abs(atom - want_atom).max() <= 1e-12
    assert np.array_equal(bond, fb[:, 1]) and np.abs(sym - (fb[:, 1] + fb[g["b2revb"], 1])).max() == 0
    assert abs(tot.sum() - (fa.sum() + fb.sum())) <= 1e-10
    assert np.array_equal(sym, sym[g["b2revb"]])
