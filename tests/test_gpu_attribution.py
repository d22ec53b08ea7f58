"""GPU tests of the attributions: rr_input_attribution_f32 and rr_attribution_reduce_f32 against their
restatements, and input_gradients / attribute against the f64 oracle (tests/attribution_ref.py).

Kernel bounds (derived, not measured; worst-case f32 accumulation in any order, doubled):
    attr   2 (N + K) 2^-24 sum_{k in s} |x| (sum_n |dz||w| + |add|)
    dx     2 (N + 1) 2^-24 (sum_n |dz||w| + |add|)
They are stated for alpha = 1; the cases use |alpha| <= 1, which only shrinks the error.  accumulate = 1 adds ONE more f32
addition, prior + new: its rounding, 2^-24 |prior + new|, is added to the bound of those cases.
Model bounds: 1e-4 of a tensor's largest entry + 1e-6 (what test_train_step_without_a_plan_against_the_fp64_oracle holds the
per-op path to), scores 1e-5 (1 + |ref|).  The fixtures keep a gate margin >= 1e-6 (tests/test_attribution_cpu.py), so the
comparison is against the oracle's own ReLU gates and leaves nothing out."""
import numpy as np
import pytest
import torch

from tests import attribution_ref as AR
from tests import helpers, poison

from reactranker_amd import featurization, synth
from reactranker_amd.base_model import build_model

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MS = (1, 15, 16, 17, 63, 64, 65, 127, 129, 1000, 4099)
NS = (1, 3, 4, 30, 64, 300, 612, 1024)
KS = (1, 22, 61, 83, 128)


def _cases():
    out = []
    for i in range(40):
        M, N, K = MS[i % 11], NS[i % 8], KS[i % 5]
        if K == 83 and i % 4 != 1:
            segs = (61, 83)
        elif i % 4 == 1 and K >= 4:
            segs = (K // 4, K // 2, K - 1, K)
        else:
            segs = (K,)
        out.append(dict(i=i, M=M, N=N, K=K, segs=segs, pad=(0, 1, 3)[i % 3], outputs=("both", "attr", "dx")[(i // 2) % 3],
                        add=i % 2 == 1, alpha=(1.0, 0.25, -0.5)[i % 3], acc=i % 4 >= 2, window=i % 5 == 3))
    return out


CASES = _cases()


def _case_id(c):
    return (f"{c['i']}-M{c['M']}-N{c['N']}-K{c['K']}-s{len(c['segs'])}-p{c['pad']}-{c['outputs']}"
            f"{'-add' if c['add'] else ''}{'-acc' if c['acc'] else ''}{'-win' if c['window'] else ''}")


def _pitch(width, pad):
    """pad 0: the width itself; 1: the next multiple of four above it (16-byte rows); 3: an odd pitch"""
    if pad == 0:
        return width
    if pad == 1:
        return (width + 4) // 4 * 4
    return width + 3 + (width % 2 == 0)


def _dev(a, ld, fill=np.nan):
    """[rows, width] numpy -> a device tensor view with row pitch ld whose pad columns hold `fill`"""
    rows, width = a.shape
    buf = np.full((rows, ld), fill, np.float32)
    buf[:, :width] = a
    return torch.from_numpy(buf).cuda()[:, :width]


def _inputs(c, fill=np.nan):
    rng = np.random.default_rng(1000 + c["i"])
    M, N, K = c["M"], c["N"], c["K"]
    off = 7 if c["window"] else 0
    h = dict(dz=rng.standard_normal((M, N)).astype(np.float32), w=rng.standard_normal((N, off + K + (5 if off else 0))).astype(np.float32),
             x=rng.standard_normal((M, K)).astype(np.float32), off=off)
    if c["add"]:
        h["add"] = rng.standard_normal((5, K)).astype(np.float32)
        h["idx"] = rng.integers(0, 5, M).astype(np.int32)
        h["idx"][: min(M, 3)] = 0                                                     # zero and repeated indices
    h["attr0"] = rng.standard_normal((M, len(c["segs"]))).astype(np.float32)
    h["dx0"] = rng.standard_normal((M, K)).astype(np.float32)
    d = dict(dz=_dev(h["dz"], _pitch(N, c["pad"]), fill), x=_dev(h["x"], _pitch(K, c["pad"]), fill))
    wfull = h["w"].copy()
    if off:                                                                           # the columns outside the window: never read
        wfull[:, :off] = fill
        wfull[:, off + K:] = fill
    d["w"] = _dev(wfull, _pitch(wfull.shape[1], c["pad"]), fill)
    if c["add"]:
        d["add"], d["idx"] = _dev(h["add"], _pitch(K, c["pad"]), fill), torch.from_numpy(h["idx"]).cuda()
    return h, d


def _launch(c, h, d, out_fill=None):
    from reactranker_amd import attribution as A
    M, K = c["M"], c["K"]
    attr = dx = None
    if c["outputs"] in ("both", "attr"):
        attr = _dev(h["attr0"] if (c["acc"] or out_fill is None) else np.full_like(h["attr0"], out_fill),
                    _pitch(len(c["segs"]), c["pad"]), 0.0)
    if c["outputs"] in ("both", "dx"):
        dx = _dev(h["dx0"] if (c["acc"] or out_fill is None) else np.full_like(h["dx0"], out_fill), _pitch(K, c["pad"]), 0.0)
    A.input_attribution(d["dz"], d["w"], K, w_offset=h["off"], x=d["x"] if attr is not None else None, add=d.get("add"),
                        add_idx=d.get("idx"), segments=c["segs"], alpha=c["alpha"], accumulate=c["acc"], attr=attr, dx=dx, M=M)
    torch.cuda.synchronize()
    return attr, dx


def _reference(c, h):
    """f64 values and the derived bounds of both outputs"""
    K, off = c["K"], h["off"]
    dz, w, x = h["dz"].astype(np.float64), h["w"][:, off:off + K].astype(np.float64), h["x"].astype(np.float64)
    dX, A = dz @ w, np.abs(dz) @ np.abs(w)
    if c["add"]:
        dX, A = dX + h["add"].astype(np.float64)[h["idx"]], A + np.abs(h["add"].astype(np.float64))[h["idx"]]
    N = c["N"]
    attr, b_attr, lo = [], [], 0
    for hi in c["segs"]:
        attr.append(c["alpha"] * (x[:, lo:hi] * dX[:, lo:hi]).sum(1))
        b_attr.append(2 * (N + K) * U * (np.abs(x[:, lo:hi]) * A[:, lo:hi]).sum(1))
        lo = hi
    attr, b_attr = np.stack(attr, 1), np.stack(b_attr, 1)
    dx, b_dx = c["alpha"] * dX, 2 * (N + 1) * U * A
    if c["acc"]:
        attr, dx = attr + h["attr0"], dx + h["dx0"]
        b_attr, b_dx = b_attr + U * np.abs(attr), b_dx + U * np.abs(dx)
    return attr, b_attr, dx, b_dx


def _ratio(got, ref, bound):
    err = np.abs(got.double().cpu().numpy() - ref)
    assert np.isfinite(err).all()
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_input_attribution_against_f64(c, parity_log):
    h, d = _inputs(c)                                                                 # every pad column holds a NaN
    attr, dx = _launch(c, h, d)
    r_attr, b_attr, r_dx, b_dx = _reference(c, h)
    worst = 0.0
    if attr is not None:
        worst = max(worst, _ratio(attr, r_attr, b_attr))
    if dx is not None:
        worst = max(worst, _ratio(dx, r_dx, b_dx))
    parity_log(f"{_case_id(c)}: worst error / bound {worst:.3e}")
    helpers.record("input_attribution err/bound", worst, 1.0)
    assert worst <= 1.0


def test_value_coverage_of_the_case_table():
    assert {c["M"] for c in CASES} == set(MS) and {c["N"] for c in CASES} == set(NS) and {c["K"] for c in CASES} == set(KS)
    assert {len(c["segs"]) for c in CASES} == {1, 2, 4} and {c["pad"] for c in CASES} == {0, 1, 3}
    assert {c["outputs"] for c in CASES} == {"both", "attr", "dx"}
    for key in ("add", "acc", "window"):
        assert {c[key] for c in CASES} == {False, True}


BIG = dict(i=100, M=4099, N=300, K=83, segs=(61, 83), pad=1, outputs="both", add=True, alpha=0.25, acc=False, window=False)


def test_two_launches_give_the_same_bits_and_rows_do_not_depend_on_their_position():
    h, d = _inputs(BIG)
    a1, x1 = _launch(BIG, h, d)
    a2, x2 = _launch(BIG, h, d)
    assert torch.equal(a1, a2) and torch.equal(x1, x2)
    sub = dict(BIG, M=64)
    lo, hi = 1000, 1064
    hs = dict(h, attr0=h["attr0"][lo:hi], dx0=h["dx0"][lo:hi])
    ds = dict(d, dz=d["dz"][lo:hi], x=d["x"][lo:hi], idx=d["idx"][lo:hi].contiguous())
    a3, x3 = _launch(sub, hs, ds)
    assert torch.equal(a3, a1[lo:hi]) and torch.equal(x3, x1[lo:hi])


@pytest.mark.parametrize("i", [0, 13, 23, 33])
def test_poisoned_outputs_and_pad_columns_change_nothing(i):
    """accumulate = 0: what the outputs held is never read; pad columns of dz, x, w and add (and the columns of a wider weight
    outside the window) never reach a result: zeros, a large finite value and NaN there give the same bits."""
    c = dict(CASES[i], acc=False, outputs="both")
    base = None
    for fill in (0.0, 3.0e38, np.nan):
        h, d = _inputs(c, fill)
        got = _launch(c, h, d, out_fill=fill)
        bits = [poison.bits(t) for t in got]
        if base is None:
            base = bits
        else:
            assert all(torch.equal(a, b) for a, b in zip(base, bits)), fill


def test_fused_entry_agrees_with_the_two_step_form(parity_log):
    """linear() with the packed transposed weight, then an f64 row-dot: the composition the fused W_i call replaces."""
    from reactranker_amd import attribution as A
    from reactranker_amd import functions as Fn
    c = dict(i=200, M=1000, N=64, K=83, segs=(61, 83), pad=1, outputs="attr", add=False, alpha=1.0, acc=False, window=False)
    h, d = _inputs(c, 0.0)
    attr, _ = _launch(c, h, d)
    Wi = Fn.LinW(torch.from_numpy(h["w"]).cuda(), None)
    dX = Fn.linear(c["M"], 83, Wi.pk_t(0, 83), w_packed=True, a1=d["dz"], k1=c["N"])
    torch.cuda.synchronize()
    x = h["x"].astype(np.float64)
    pr = x * dX[:, :83].double().cpu().numpy()
    two = np.stack([pr[:, :61].sum(1), pr[:, 61:].sum(1)], 1)
    _, b_attr, _, b_dx = _reference(c, h)
    ax = np.abs(x) * b_dx
    tol = b_attr + np.stack([ax[:, :61].sum(1), ax[:, 61:].sum(1)], 1)
    worst = _ratio(attr, two, tol)
    parity_log(f"fused vs two-step: worst difference / (sum of both bounds) {worst:.3e}")
    assert worst <= 1.0


def test_finish_kernel_is_bit_equal_to_its_restatement():
    from reactranker_amd import attribution as A
    rng = np.random.default_rng(11)
    specs = [synth.random_reactant(rng, n) for n in (1, 7, 1, 70, 5, 9)]              # one-atom molecules, more than a wavefront
    b = featurization.BatchMolGraph(specs, K=7)                                       # a2b wider than every degree
    g = b.device_graph(0)
    assert g.K == 7
    fa = rng.standard_normal((g.nA, 1)).astype(np.float32)
    fb = rng.standard_normal((g.nB, 2)).astype(np.float32)
    fa[0], fb[0] = 0.0, 0.0
    got = A.attribution_reduce(g, torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda())
    again = A.attribution_reduce(g, torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda())
    torch.cuda.synchronize()
    want = AR.np_attribution_reduce(fa, fb, g.a2b.cpu().numpy(), g.b2revb.cpu().numpy(), g.a_scope.cpu().numpy().reshape(-1, 2))
    for name, t, t2, w in zip(("atom", "bond", "bond_sym", "mol_total"), got, again, want):
        assert torch.equal(t, t2), name
        assert torch.equal(poison.bits(t), poison.bits(torch.from_numpy(np.ascontiguousarray(w)))), name
    assert got[3].dtype == torch.float64 and got[0].dtype == torch.float32
    report, _, _ = poison.fill_dependence(lambda: A.attribution_reduce(g, torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda()),
                                          sync=torch.cuda.synchronize)
    assert not report, report


# ================================================================================================ the model against the oracle
_REF = {}


def _setup(key, H, depth, dd, bias, task_num=1, F=1, task_type="listnet", last="with_softplus", zero_bias=False):
    """(model on the GPU, batches, query batch, weights, oracle cfg) - the oracle side is computed once per key and shared"""
    qb = AR.batch()
    w = AR.weights(H, depth, dd, bias, task_num, F)
    if zero_bias:
        w = AR.zero_biases(w)
    model = build_model(hidden_size=H, mpnn_depth=depth, mpnn_diff_depth=dd, ffn_depth=3, use_bias=bias, dropout=0.0,
                        task_num=task_num, ffn_last_layer=last, task_type=task_type, add_features_dim=F)
    model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    model = model.cuda().eval()
    rb, pb = featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs)
    cfg = AR.cfg_of(depth, dd, model.ffn.task_type)
    return model, rb, pb, qb, w, cfg


def _ref(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _close(name, got, ref, log):
    ref = np.asarray(ref, np.float64)
    got = got.double().cpu().numpy().reshape(ref.shape)
    err = float(np.abs(got - ref).max())
    tol = 1e-4 * float(np.abs(ref).max()) + 1e-6
    log(f"{name}: max err {err:.3e} (bound {tol:.3e}, largest entry {float(np.abs(ref).max()):.3e})")
    helpers.record(name, err, tol)
    assert np.isfinite(got).all() and err <= tol, (name, err, tol)


def _close_score(got, ref, log):
    got = got.double().cpu().numpy()
    err = np.abs(got - ref)
    log(f"score: max err {float(err.max()):.3e}")
    assert (err <= 1e-5 * (1 + np.abs(ref))).all()


GRAD_KEYS = ("d_f_atoms_r", "d_f_bonds_r", "d_f_atoms_p", "d_f_bonds_p", "d_add_features")
ATTR_KEYS = ("atom_r", "atom_p", "bond_r", "bond_p", "bond_sym_r", "bond_sym_p", "feature", "total")


def _check_grads(model, rb, pb, qb, w, cfg, key, log, column=0, feats=True):
    from reactranker_amd import attribution as A
    got = A.input_gradients(model, rb, pb, qb.add_features if feats else None, column=column, gpu=0)
    torch.cuda.synchronize()
    ref = _ref((key, "grad"), lambda: AR.gradients(w, cfg, qb, column, 1.0, feats))
    for k in GRAD_KEYS:
        if ref[k] is None:
            assert got[k] is None
            continue
        r = ref[k][:, :got[k].shape[1]]
        _close(k, got[k], r, log)
    _close_score(got["score"], ref["score"], log)


def _check_attr(model, rb, pb, qb, w, cfg, key, log, method, column=0, feats=True):
    from reactranker_amd import attribution as A
    got = A.attribute(model, rb, pb, qb.add_features if feats else None, column=column, method=method, steps=AR.IG_STEPS, gpu=0)
    torch.cuda.synchronize()
    ref = _ref((key, method), lambda: AR.attribute(w, cfg, qb, column, method, AR.IG_STEPS, feats))
    assert min(ref["margins"]) >= AR.MIN_MARGIN
    for k in ATTR_KEYS:
        if ref[k] is None:
            assert got[k] is None
            continue
        _close(f"{method}.{k}", got[k], ref[k], log)
    _close_score(got["score"], ref["score"], log)
    assert got["total"].dtype == torch.float64
    if method == "integrated_gradients":
        _close_score(got["baseline_score"], ref["baseline_score"], log)
        want = got["total"] - (got["score"].double() - got["baseline_score"].double())
        assert torch.equal(got["gap"], want)
        log(f"{method}: max |gap| {float(got['gap'].abs().max()):.3e} (oracle {float(np.abs(ref['gap']).max()):.3e})")
    return got


@pytest.mark.parametrize("fx", AR.FIXTURES, ids=AR.fixture_id)
def test_input_gradients_against_the_oracle(fx, parity_log):
    H, depth, dd, bias, _ = fx
    _check_grads(*_setup(fx, H, depth, dd, bias), fx, parity_log)


@pytest.mark.parametrize("fx", AR.FIXTURES, ids=AR.fixture_id)
def test_grad_x_input_against_the_oracle(fx, parity_log):
    H, depth, dd, bias, _ = fx
    _check_attr(*_setup(fx, H, depth, dd, bias), fx, parity_log, "grad_x_input")


@pytest.mark.parametrize("fx", [f for f in AR.FIXTURES if f[4]], ids=AR.fixture_id)
def test_integrated_gradients_against_the_oracle(fx, parity_log):
    H, depth, dd, bias, _ = fx
    _check_attr(*_setup(fx, H, depth, dd, bias), fx, parity_log, "integrated_gradients")


def test_two_output_columns_second_column(parity_log):
    args = _setup("two", 64, 2, 2, True, task_num=2, task_type=None)
    assert args[0].ffn.task_type == "gaussian_with_softplus"
    _check_grads(*args, "two", parity_log, column=1)
    _check_attr(*args, "two", parity_log, "grad_x_input", column=1)
    _check_attr(*args, "two", parity_log, "integrated_gradients", column=1)


def test_no_appended_features(parity_log):
    args = _setup("nofeat", 64, 2, 2, True, F=0)
    _check_grads(*args, "nofeat", parity_log, feats=False)
    got = _check_attr(*args, "nofeat", parity_log, "grad_x_input", feats=False)
    assert got["feature"] is None


def test_gradient_x_input_is_complete_without_biases(parity_log):
    """Euler's theorem on the GPU: zero biases (through load_state_dict) and a raw head make the model positively homogeneous,
    so the attributions of a candidate sum to its score.  Measured and logged; held to the model bound."""
    from reactranker_amd import attribution as A
    model, rb, pb, qb, w, cfg = _setup("euler", 64, 2, 2, True, task_type=None, last="no_softplus", zero_bias=True)
    assert model.ffn.head() == 0
    got = A.attribute(model, rb, pb, qb.add_features, method="grad_x_input", gpu=0)
    torch.cuda.synchronize()
    score = got["score"].double().cpu().numpy()
    err = float(np.abs(got["total"].cpu().numpy() - score).max())
    parity_log(f"zero biases, raw head: max |total - score| {err:.3e}, max |score| {float(np.abs(score).max()):.3e}")
    assert err <= 1e-4 * float(np.abs(score).max()) + 1e-6


@pytest.mark.parametrize("method", ["grad_x_input", "integrated_gradients"])
def test_a_call_leaves_everything_as_it_was(method):
    from reactranker_amd import attribution as A
    model, rb, pb, qb, w, cfg = _setup("leave", 64, 2, 2, True)
    model.train()
    for q in model.parameters():
        if q.requires_grad:
            q.grad = torch.full_like(q, 0.5)
    with torch.no_grad():
        model.eval()
        before = model(rb, pb, gpu=0, add_features=qb.add_features).clone()
        model.train()
    g_p = featurization.device_graph_of(pb, 0)
    fbs = g_p.fb_sum()
    snap = [t.clone() for t in (g_p.f_atoms, g_p.f_bonds, fbs)]
    A.attribute(model, rb, pb, qb.add_features, method=method, steps=3, gpu=0)
    A.input_gradients(model, rb, pb, qb.add_features, gpu=0)
    torch.cuda.synchronize()
    assert model.training
    assert featurization.device_graph_of(pb, 0) is g_p and g_p.fb_sum() is fbs
    for t, s in zip((g_p.f_atoms, g_p.f_bonds, fbs), snap):
        assert torch.equal(poison.bits(t), poison.bits(s))
    for q in model.parameters():
        if q.requires_grad:
            assert torch.equal(q.grad, torch.full_like(q, 0.5))
    with torch.no_grad():
        model.eval()
        after = model(rb, pb, gpu=0, add_features=qb.add_features)
    assert torch.equal(before, after)
