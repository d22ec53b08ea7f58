"""Nearest-neighbour search on the GPU (reactranker_amd.neighbors, rr_knn_f32 / rr_row_sqnorm_f32)
against the float64 oracle of tests/neighbors_ref.py.

Bounds.  tol(m, n) = 2 (H + 3) 2^-24 (|q_m|^2 + |b_n|^2) is derived in tests/neighbors_ref.py (worst-case rounding of three
H-term f32 sums and two additions; independent of the chain order).  Integer coordinates in [-3, 3] make every product and sum
exact in f32, so those cases are compared exactly.  Where a test compares VALUES per slot instead of indices it uses that the
j-th smallest of a perturbed row lies within the largest perturbation of the j-th smallest of the exact row."""
import ctypes as C

import numpy as np
import pytest
import torch

from reactranker_amd import _lib, featurization, synth
from reactranker_amd import neighbors as N
from reactranker_amd import uncertainty as U
from reactranker_amd.base_model import build_model
from reactranker_amd.functions import StepPlan
from reactranker_amd.utils import save_checkpoint
from oracle import ref_cpu as O
from tests import helpers as Hh
from tests import neighbors_ref as R
from tests import poison, streams

pytestmark = pytest.mark.gpu

RT, BT, MAXK = N.geometry()


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def run(q, b, k, **kw):
    kw = {key: (dev(v, np.int32) if key.endswith("group") and v is not None else v) for key, v in kw.items()}
    d, i = N.knn(dev(q), dev(b), k, **kw)
    torch.cuda.synchronize()
    assert d.dtype == torch.float32 and i.dtype == torch.int64 and tuple(d.shape) == tuple(i.shape) == (len(q), k)
    return d.cpu().numpy(), i.cpu().numpy()


class splits:
    def __init__(self, s):
        self.s = s

    def __enter__(self):
        assert _lib.lib().rr_knn_set_splits(self.s) == 0

    def __exit__(self, *a):
        assert _lib.lib().rr_knn_set_splits(0) == 0


def int_case(seed, M, Nb, H, plant=True):
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, (M, H)).astype(np.float32)
    b = rng.integers(-3, 4, (Nb, H)).astype(np.float32)
    if plant and Nb > 0:
        for j in range(min(9, Nb)):                                 # duplicates of query rows: d = 0 and ties by index
            b[(7 * j + 3) % Nb] = q[(5 * j) % M]
    return q, b


# ---------------------------------------------------------------------------------------------- 1. exact inputs, exact answer
BASE = dict(M=RT + 1, Nb=3 * BT + 5, H=30, k=2)
EXACT = ([dict(BASE, M=m) for m in (1, RT - 1, RT, RT + 1, 2 * RT + 3)]
         + [dict(BASE, Nb=n) for n in (1, BT - 1, BT + 1, 3 * BT + 5)]
         + [dict(BASE, k=63, Nb=n) for n in (62, 63)] + [dict(BASE, k=1, Nb=0), dict(BASE, k=64, Nb=64), dict(BASE, k=64, Nb=63)]
         + [dict(BASE, H=h, Nb=BT + 1, k=(64 if i % 2 else 1)) for i, h in enumerate((1, 3, 4, 30, 300, 322, 600))]
         + [dict(BASE, H=300, M=2 * RT + 3, k=63)]
         + [dict(BASE, M=2 * RT + 3, H=4, k=k) for k in (1, 2, 63, 64)])


@pytest.mark.parametrize("c", EXACT, ids=lambda c: "M{M}_N{Nb}_H{H}_k{k}".format(**c))
def test_exact_inputs_give_the_exact_answer(c):
    q, b = int_case(11 + c["M"] + c["Nb"] + c["H"], c["M"], c["Nb"], c["H"])
    want_d, want_i, D = R.knn_ref(q, b, c["k"])
    got_d, got_i = run(q, b, c["k"])
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_d.astype(np.float64), want_d)
    if c["Nb"] >= 64 and c["H"] >= 4:
        assert (want_d[:, 0] == 0).any()                            # a planted duplicate was found at distance 0
    if c["Nb"] > c["k"] and c["H"] <= 4:
        srt = np.sort(D, axis=1)
        assert (srt[:, c["k"] - 1] == srt[:, c["k"]]).any()         # the cut went through a tie somewhere


# ---------------------------------------------------------------------------------------------- 2. random floats, bounded error
def float_case(seed, M, Nb, H, kind):
    rng = np.random.default_rng(seed)
    q, b = rng.standard_normal((M, H)), rng.standard_normal((Nb, H))
    if kind == "shifted":
        q, b = q + 3.0, b + 3.0
    elif kind == "scaled":
        q, b = q * 30.0, b * 30.0
    q, b = q.astype(np.float32), b.astype(np.float32)
    for j in range(8):
        b[(11 * j + 2) % Nb] = q[(3 * j) % M]                       # exact duplicates
        b[(13 * j + 5) % Nb] = q[(3 * j + 1) % M] + np.float32(1e-3) * rng.standard_normal(H).astype(np.float32)
    return q, b


@pytest.mark.parametrize("H", [1, 3, 4, 30, 300, 322, 600])
def test_random_floats_bounded_error_and_nothing_missed(H, parity_log):
    M, Nb = 2 * RT + 3, 3 * BT + 5
    worst = 0.0
    for kind, k in (("normal", 16), ("shifted", 64), ("scaled", 1)):
        q, b = float_case(100 + H, M, Nb, H, kind)
        D = R.distances64(q, b)
        T = R.tol(q, b)
        d, i = run(q, b, k)
        rows = np.arange(M)[:, None]
        assert (i >= 0).all() and (i < Nb).all()
        err = np.abs(d.astype(np.float64) - D[rows, i])
        ratio = float((err / T[rows, i]).max())
        worst = max(worst, ratio)
        parity_log(f"H {H} {kind} k {k}: worst |dist - D64| / tol = {ratio:.4f}")
        assert (err <= T[rows, i]).all()                                                       # (a)
        if k > 1:                                                                              # (b) ascending under (dist, idx)
            assert ((d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (i[:, 1:] > i[:, :-1]))).all()
        assert all(len(set(r)) == k for r in i.tolist())
        kth = i[:, k - 1]                                                                      # (c) nothing closer was left out
        bound = (D[np.arange(M), kth] - T[np.arange(M), kth])[:, None] - T
        left_out = np.ones((M, Nb), bool)
        left_out[rows, i] = False
        assert not (left_out & (D < bound)).any()
    Hh.record(f"knn H={H}: worst |dist - D64| / tol", worst, 1.0)


# ---------------------------------------------------------------------------------------------- 3. planted neighbours, wide gaps
def test_planted_neighbours_with_wide_gaps_are_found_in_order():
    rng = np.random.default_rng(5)
    M, H, J, far = RT + 6, 30, 8, 500
    q = (0.1 * rng.standard_normal((M, H))).astype(np.float32)
    planted = np.repeat(q, J, axis=0)
    for m in range(M):
        for j in range(1, J + 1):
            planted[m * J + j - 1, j] += np.float32(j * 1e-2)
    b = np.concatenate([planted, (1.0 + 0.1 * rng.standard_normal((far, H))).astype(np.float32)])
    b = b[rng.permutation(len(b))]
    want_d, want_i, D = R.knn_ref(q, b, J)
    T = R.tol(q, b)
    order = np.argsort(D, axis=1, kind="stable")[:, :J + 1]
    rows = np.arange(M)[:, None]
    gaps = np.diff(D[rows, order], axis=1)
    assert (gaps > 2 * np.maximum(T[rows, order][:, 1:], T[rows, order][:, :-1])).all()        # the oracle's own precondition
    _, got_i = run(q, b, J)
    assert np.array_equal(got_i, want_i)


# ---------------------------------------------------------------------------------------------- 4. decomposition does not show
def test_decomposition_position_pitch_and_alignment_do_not_show():
    rng = np.random.default_rng(9)
    M, Nb, H, k = RT + 6, 8 * BT + 76, 322, 16
    q, b = rng.standard_normal((M, H)).astype(np.float32), rng.standard_normal((Nb, H)).astype(np.float32)
    tq, tb = dev(q), dev(b)
    base = N.knn(tq, tb, k)
    again = N.knn(tq, tb, k)
    assert torch.equal(base[0], again[0]) and torch.equal(base[1], again[1])
    want_i = R.knn_ref(q, b, k)[1]
    assert (base[1].cpu().numpy() == want_i).mean() > 0.99           # (the bits below are compared, not these)
    for s in (1, 2, 3, 7):
        with splits(s):
            assert _lib.lib().rr_knn_splits() == s
            got = N.knn(tq, tb, k)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), s
    assert _lib.lib().rr_knn_splits() == 0
    # the same query rows at other positions of a larger M
    big = torch.randn(3 * RT + 9, H, device="cuda")
    pos = torch.from_numpy(rng.permutation(big.shape[0])[:M]).cuda()
    big[pos] = tq
    got = N.knn(big, tb, k)
    assert torch.equal(got[0][pos], base[0]) and torch.equal(got[1][pos], base[1])
    # the bank at other pitches (the pad columns hold NaN: they never reach a result) and at a 4-byte-aligned pointer
    for pitch in (H + 2, H + 5, H + 6):                               # 324: 16-byte rows; 327, 328: not / 16-byte rows
        wide = torch.full((Nb, pitch), float("nan"), device="cuda")
        wide[:, :H] = tb
        got = N.knn(tq, wide[:, :H], k)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), pitch
    flat = torch.full((Nb * H + 1,), float("nan"), device="cuda")
    flat[1:] = tb.reshape(-1)
    off = flat[1:].view(Nb, H)
    assert off.data_ptr() % 16 == 4
    got = N.knn(tq, off, k)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    got = N.knn(tq, off, k, bank_sqnorm=N.row_sqnorm(off))
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    assert torch.equal(N.row_sqnorm(off), N.row_sqnorm(tb))


# ---------------------------------------------------------------------------------------------- 5. groups and degenerate cases
def test_group_exclusion_against_the_oracle():
    q, b = int_case(21, RT + 6, 5 * BT + 60, 30)
    M, Nb = len(q), len(b)
    qg = (np.arange(M) % 8).astype(np.int32)
    for bg in ((np.arange(Nb) // 100).astype(np.int32),               # group 2 = rows 200..299 straddles the boundary at 256
               (np.arange(Nb) // (2 * BT)).astype(np.int32)):         # with 3 splits of 2 tiles: group s IS split s
        want_d, want_i, _ = R.knn_ref(q, b, 7, qg, bg)
        for s in (0, 3):
            with splits(s):
                got_d, got_i = run(q, b, 7, q_group=qg, b_group=bg)
            assert np.array_equal(got_i, want_i) and np.array_equal(got_d.astype(np.float64), want_d)
    # every bank row excluded for one query, negative ids on both sides for another
    bg = np.full(Nb, 5, np.int32)
    bg[:3] = -1
    qg3 = np.array([5, 1, -1], np.int32)
    want_d, want_i, _ = R.knn_ref(q[:3], b, 4, qg3, bg)
    got_d, got_i = run(q[:3], b, 4, q_group=qg3, b_group=bg)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d.astype(np.float64), want_d)
    assert want_i[0].tolist()[3] == -1 and set(want_i[0].tolist()[:3]) == {0, 1, 2}
    # negative ids match nothing: the same as no groups at all
    plain = run(q, b, 5)
    neg = run(q, b, 5, q_group=np.full(M, -1, np.int32), b_group=np.full(Nb, -1, np.int32))
    assert np.array_equal(plain[0], neg[0]) and np.array_equal(plain[1], neg[1])


def test_leave_one_out_of_a_bank_against_itself():
    _, b = int_case(22, 1, 2 * BT + 9, 30, plant=False)
    g = np.arange(len(b), dtype=np.int32)
    want_d, want_i, _ = R.knn_ref(b, b, 3, g, g)
    got_d, got_i = run(b, b, 3, q_group=g, b_group=g)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d.astype(np.float64), want_d)
    assert not (got_i == np.arange(len(b))[:, None]).any()
    assert (run(b, b, 1)[1][:, 0] <= np.arange(len(b))).all()         # without groups a row finds itself (or an earlier twin)


def test_nan_rows_infinite_distances_and_empty_inputs():
    q, b = int_case(23, 5, BT + 7, 30)
    b[17] = np.nan
    b[40, 3] = np.nan
    want_d, want_i, _ = R.knn_ref(q, b, 64)
    got_d, got_i = run(q, b, 64)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d.astype(np.float64), want_d)
    assert not np.isin(got_i, (17, 40)).any() and not np.isnan(got_d).any()
    # a distance that overflows to +inf is a candidate: after the finite ones, before the padding
    q, b = int_case(24, 3, 5, 30, plant=False)
    b[2] = 1e20
    want_i = R.knn_ref(q, b, 8)[1]
    got_d, got_i = run(q, b, 8)
    assert np.array_equal(got_i, want_i) and (got_i[:, 4] == 2).all() and (got_i[:, 5:] == -1).all()
    assert np.isinf(got_d[:, 4:]).all() and np.isfinite(got_d[:, :4]).all()
    # N < k and N == 0 give the padding; M == 0 launches nothing
    got_d, got_i = run(q, b[:2], 4)
    assert (got_i[:, 2:] == -1).all() and np.isinf(got_d[:, 2:]).all() and (got_i[:, :2] >= 0).all()
    got_d, got_i = run(q, b[:0], 4)
    assert (got_i == -1).all() and np.isinf(got_d).all() and (got_d > 0).all()
    got_d, got_i = run(q[:0], b, 4)
    assert got_d.shape == got_i.shape == (0, 4)
    one = torch.zeros(4, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    st = _lib.lib().rr_knn_f32(_lib.ptr(one), 4, 0, _lib.ptr(one), 4, 1, 4, 1, None, None, None, _lib.ptr(one), _lib.ptr(one),
                               _lib.ptr(ws), C.c_size_t(4096), _lib.stream())
    assert st == 0


# ---------------------------------------------------------------------------------------------- 6. what memory held
@pytest.mark.parametrize("shape", [(RT + 6, 8 * BT + 76, 16), (3, 5, 8)], ids=["split", "padded"])
def test_nothing_depends_on_what_memory_held(shape):
    M, Nb, k = shape
    rng = np.random.default_rng(31)
    tq, tb = dev(rng.standard_normal((M, 30))), dev(rng.standard_normal((Nb, 30)))
    report, counters, last = poison.fill_dependence(lambda: N.knn(tq, tb, k), sync=torch.cuda.synchronize)
    assert not report, report
    assert counters[0xFF].buffers >= 3                                # dist, idx and the workspace were all poisoned
    d, i = last
    assert not torch.isnan(d).any() and ((i >= 0) | torch.isinf(d)).all()
    if Nb < k:
        assert (i[:, Nb:] == -1).all() and torch.isinf(d[:, Nb:]).all()


# ---------------------------------------------------------------------------------------------- 7. stream order
def _stream_cases():
    def build_knn(with_norms):
        def build():
            rng = np.random.default_rng(41)
            q, b = dev(rng.standard_normal((RT + 6, 30))), dev(rng.standard_normal((8 * BT + 76, 30)))

            def fn(inputs):
                tq, tb = inputs
                if with_norms:
                    bn = N.row_sqnorm(tb)
                    return N.knn(tq, tb, 8, bank_sqnorm=bn) + (bn,)
                return N.knn(tq, tb, 8)
            return [q, b], fn
        return build
    return [streams.Case("rr_knn_f32", build_knn(False)), streams.Case("rr_row_sqnorm_f32+rr_knn_f32", build_knn(True))]


@pytest.mark.parametrize("case", _stream_cases(), ids=lambda c: c.name)
def test_entry_points_are_ordered_on_the_callers_stream(case, parity_log):
    streams.check_table("neighbors", _stream_cases())
    res = streams.staged(case, log=parity_log)
    assert res.status == "armed"


# ---------------------------------------------------------------------------------------------- 8. the Python layer
def _close(got, ref, tol=1e-5, what=""):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.max(np.abs(got - ref) / (1 + np.abs(ref))) if got.size else 0.0
    Hh.record(what, err, tol)
    assert err <= tol, f"{what}: err {err:.3e} > {tol}"


@pytest.mark.parametrize("path", Hh.model_case_files(), ids=lambda p: p.split("model_")[-1][:-4])
def test_reaction_vectors_against_reference_vectors(path):
    """the criterion of tests/test_gpu_model.py for `vecs`: |err| <= 1e-5 (1 + |ref|)"""
    d, cfg = Hh.load_case(path)
    H = cfg["hidden_size"]
    shapes = O.model_shapes(H, cfg["mpnn_depth"], cfg["mpnn_diff_depth"], cfg["ffn_depth"], cfg["task_num"],
                            cfg["add_features_dim"], cfg["use_bias"])
    kw = {k: cfg[k] for k in ("hidden_size", "mpnn_depth", "mpnn_diff_depth", "ffn_depth", "use_bias", "task_num",
                              "ffn_last_layer", "task_type", "add_features_dim")}
    model = build_model(dropout=0.1, **kw)
    model.load_state_dict({k: torch.tensor(v) for k, v in Hh.case_weights(d, cfg, shapes).items()})
    model = model.cuda().train()
    qb = Hh.case_queries(cfg)
    rb, pb = featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs)
    add = d["add_features"] if "add_features" in d.files else None
    batches = [(rb, pb, cfg["scope"], torch.tensor(d["targets"]), add), (rb, pb, [], torch.zeros(0), None)]
    sentinel = object()
    StepPlan.last = sentinel
    try:
        assert StepPlan.keep_last is False
        full = N.reaction_vectors(model, batches, 0, include_features=True)
        vec = N.reaction_vectors(model, batches, 0)
        assert model.training and StepPlan.keep_last is False and StepPlan.last is sentinel
    finally:
        StepPlan.last = None
    _close(full, d["vecs"], what="reaction_vectors(include_features)")
    assert tuple(vec.shape) == (d["vecs"].shape[0], H) and torch.equal(vec, full[:, :H]) and vec.is_contiguous()
    model.eval()
    with torch.no_grad():
        out = model(rb, pb, gpu=0, add_features=add)
        _close(model.ffn(full), out, what="ffn(reaction_vectors) vs model(r, p)")
        model.dedup_reactants = False
        plain = N.reaction_vectors(model, batches, 0, include_features=True)
    _close(plain, full, what="dedup_reactants False vs auto")
    _close(plain, d["vecs"], what="reaction_vectors(dedup_reactants=False)")


CFG = dict(hidden_size=64, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, task_num=1,
           ffn_last_layer="with_softplus", add_features_dim=1)


def _model(wseed, dropout=0.1):
    m = build_model(dropout=dropout, **CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in synth.seeded_weights(O.model_shapes(64, 3, 3, 3, 1, 1, True), wseed).items()})
    return m.cuda()


def _batch(seed, nq=12):
    rng = np.random.default_rng(seed)
    scope = [int(c) for c in rng.integers(3, 13, nq)]
    qb = synth.make_queries(seed, nq, scope, atoms_lo=5, atoms_hi=12)
    return (featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs), qb.scope,
            torch.tensor(qb.targets), qb.add_features)


@pytest.fixture(scope="module")
def bank_case():
    model = _model(41)
    train = [_batch(61), _batch(62, nq=5)]
    return model, train, N.ReactionBank.from_batches(model, train, 0)


def test_reaction_bank_round_trip(bank_case, tmp_path):
    model, train, bank = bank_case
    sizes = [c for b in train for c in b[2]]
    n = sum(sizes)
    assert len(bank) == n and tuple(bank.vectors.shape) == (n, 64)
    assert torch.equal(bank.vectors, N.reaction_vectors(model, train, 0))
    assert bank.group.dtype == torch.int32 and bank.group.cpu().tolist() == [g for g, c in enumerate(sizes) for _ in range(c)]
    assert torch.equal(bank.targets.cpu(), torch.cat([b[3].float() for b in train]))
    assert torch.equal(bank.sqnorm, N.row_sqnorm(bank.vectors))
    path = str(tmp_path / "bank.pt")
    bank.save(path)
    back = N.ReactionBank.load(path, "cuda")
    for name in ("vectors", "sqnorm", "targets", "group"):
        assert torch.equal(getattr(back, name), getattr(bank, name)) and getattr(back, name).is_cuda, name
    probe = bank.vectors[::3] + 1e-3
    dist, idx, tgt = bank.query(probe, 5)
    d2, i2, t2 = back.query(probe, 5)
    assert torch.equal(dist, d2) and torch.equal(idx, i2) and torch.equal(tgt, t2)
    assert torch.equal(tgt, bank.targets[idx]) and (idx >= 0).all()
    want_i = R.knn_ref(probe.cpu().numpy(), bank.vectors.cpu().numpy(), 5)[1]
    assert (idx.cpu().numpy() == want_i).mean() > 0.95
    # neighbours from OTHER queries only
    dist, idx, tgt = bank.query(bank.vectors, 4, group=bank.group)
    assert (idx >= 0).all() and not (bank.group[idx] == bank.group[:, None]).any()
    # more neighbours asked for than the bank has outside the row's query: padding, NaN targets
    small = N.ReactionBank(bank.vectors[:6], bank.targets[:6], torch.tensor([0, 0, 0, 1, 1, 1]))
    dist, idx, tgt = small.query(small.vectors, 4, group=small.group)
    assert (idx[:, 3] == -1).all() and torch.isinf(dist[:, 3]).all() and torch.isnan(tgt[:, 3]).all() and (idx[:, :3] >= 0).all()


def test_latent_distance_against_the_oracle():
    rng = np.random.default_rng(71)
    H, k = 30, 8
    b, q = rng.standard_normal((400, H)).astype(np.float32), rng.standard_normal((50, H)).astype(np.float32)
    bank = N.ReactionBank(dev(b), torch.zeros(400), torch.arange(400) // 10)
    got = N.latent_distance(bank, dev(q), k).cpu().numpy().astype(np.float64)
    want_d, want_i, _ = R.knn_ref(q, b, k)
    want = R.latent_distance_ref(want_d, want_i)
    # slot j of the kernel's list is within T = max_n tol(m, n) of slot j of the oracle's; through the square root that is
    # min(sqrt(T), T / sqrt(D)); the mean of k such terms, plus the f32 sqrt / sum / division (k + 2 roundings of the result)
    T = R.tol(q, b).max(axis=1)[:, None]
    bound = np.minimum(np.sqrt(T), T / np.sqrt(np.maximum(want_d, 1e-300))).mean(axis=1) + (k + 2) * 2.0 ** -24 * want
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / bound).max())
    Hh.record("latent_distance: worst |err| / bound", float((np.abs(got - want) / bound).max()), 1.0)
    # a group that covers the whole bank leaves no neighbour: +inf
    one = N.ReactionBank(dev(b[:10]), torch.zeros(10), torch.zeros(10, dtype=torch.int32))
    ld = N.latent_distance(one, dev(q[:4]), 3, group=torch.tensor([0, 1, 0, -1]))
    assert torch.isinf(ld[0]) and torch.isinf(ld[2]) and torch.isfinite(ld[1]) and torch.isfinite(ld[3])
    empty = N.ReactionBank(dev(b[:0]), torch.zeros(0), torch.zeros(0, dtype=torch.int32))
    assert torch.isinf(N.latent_distance(empty, dev(q[:4]), 3)).all()


def test_split_overlap_finds_exactly_the_planted_duplicates():
    rng = np.random.default_rng(72)
    H = 300
    b = rng.standard_normal((600, H)).astype(np.float32)
    v = rng.standard_normal((90, H)).astype(np.float32)
    planted = [2, 17, 40, 41, 89]
    for j, r in enumerate(planted):
        v[r] = b[100 * j + 7]
    bank = N.ReactionBank(dev(b), torch.zeros(600), torch.arange(600))
    # an exact duplicate's f32 distance is within tol = 2 (H + 3) 2^-24 (|q|^2 + |b|^2) of 0: that coefficient as rel_tol
    res = N.split_overlap(bank, dev(v), rel_tol=2 * (H + 3) * 2.0 ** -24)
    assert res["count"] == len(planted) and res["rows"].cpu().tolist() == planted
    assert res["nearest"][planted].cpu().tolist() == [100 * j + 7 for j in range(len(planted))]
    # integer coordinates: the distance of a duplicate is exactly 0, so the default tolerance finds them
    qi, bi = int_case(73, 40, 300, 30, plant=False)
    qi += 7.0
    qi[[4, 9]] = bi[[250, 3]]
    res = N.split_overlap(N.ReactionBank(dev(bi), torch.zeros(300), torch.arange(300)), dev(qi))
    assert res["rows"].cpu().tolist() == [4, 9] and res["count"] == 2 and (res["dist"][[4, 9]] == 0).all()


def test_cosine_metric_against_the_oracle_on_normalised_rows():
    rng = np.random.default_rng(74)
    H, k = 30, 6
    q, b = rng.standard_normal((40, H)).astype(np.float32) * 5, rng.standard_normal((300, H)).astype(np.float32) * 0.2
    q[3] = 0.0
    d, i = run(q, b, k, metric="cosine")

    def unit(x):
        x = x.astype(np.float64)
        n = np.linalg.norm(x, axis=1, keepdims=True)
        return np.where(n > 0, x / np.where(n > 0, n, 1), 0.0)
    D = 0.5 * R.distances64(unit(q), unit(b))
    # f32 normalisation moves a unit row by at most e = (H / 2 + 3) u, half the squared distance of two rows at most 2 apart by
    # 4 e + 2 e^2; the kernel adds half of tol on unit rows, 2 (H + 3) u: (4 H + 18) u and second-order terms
    bound = (4 * H + 18) * 2.0 ** -24 * 1.01
    rows = np.arange(len(q))[:, None]
    assert (np.abs(d - D[rows, i]) <= bound).all()
    assert (np.abs(d - np.sort(D, axis=1)[:, :k]) <= bound).all()
    assert (np.abs(d[3] - 0.5) <= bound).all()                      # the zero row: 1/2 from every unit row


def test_evaluate_applicability_on_a_seeded_synthetic_model(bank_case, tmp_path):
    model, train, bank = bank_case
    path = str(tmp_path / "ck" / "0.pt")
    mean, std = 1.7, 0.6
    save_checkpoint(path, model, mean, std)
    bs = [_batch(81), _batch(82, nq=4)]
    test_b = [dict(r=b[0], p=b[1], scope=b[2], targets=b[3], add=b[4]) for b in bs]
    other = _model(7).train()
    before = StepPlan.last
    assert StepPlan.keep_last is False
    res = N.evaluate_applicability(other, bank, test_b, path, 0, k=4)
    assert other.training and StepPlan.keep_last is False and StepPlan.last is before
    scope = [c for b in bs for c in b[2]]
    n = sum(scope)
    assert res["scope"] == scope
    for key in ("distance", "pred", "targets"):
        assert tuple(res[key].shape) == (n,) and torch.isfinite(res[key]).all(), key
    assert tuple(res["qstats"].shape) == (len(scope), 12) and tuple(res["query_distance"].shape) == (len(scope),)
    want_t = np.concatenate([(-(b[3].double().numpy() - mean) / std).astype(np.float32) for b in bs])
    assert np.array_equal(res["targets"].cpu().numpy(), want_t)
    # the checkpoint's weights were used: the same vectors and scores as `model`
    std_b = [(b[0], b[1], b[2], b[3], b[4]) for b in bs]
    vec = N.reaction_vectors(model, std_b, 0)
    assert torch.equal(res["distance"], N.latent_distance(bank, vec, 4))
    model.eval()
    with torch.no_grad():
        pred = torch.cat([model(b[0], b[1], gpu=0, add_features=b[4]).reshape(-1) for b in bs])
    model.train()
    assert torch.equal(res["pred"], pred)
    cal = U.uncertainty_calibration(res["pred"], res["targets"], res["distance"])
    assert np.array_equal(res["calibration"]["spearman"], cal["spearman"], equal_nan=True)
    for key in ("fractions", "kept", "mae", "rmse"):
        assert np.array_equal(res["calibration"][key], cal[key]), key
    o = 0
    for j, c in enumerate(scope):
        assert abs(float(res["query_distance"][j]) - float(res["distance"][o:o + c].double().mean())) < 1e-12
        o += c
    with pytest.raises(ValueError):
        N.evaluate_applicability(other, bank, test_b, [path, path], 0)
