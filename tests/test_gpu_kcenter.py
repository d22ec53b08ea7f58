"""Greedy k-center selection on the GPU (reactranker_amd.neighbors.kcenter_greedy / acquire, rr_kcenter_f32, DESIGN.md section
4h) against the numpy oracle of tests/selection_ref.py.

Integer coordinates in [-3, 3] (with integer weights and integer init_dist) make every difference, product and sum exact in
f32, so those cases must equal the float64 rounds exactly, ties included.  On random floats the kernel's outputs must be the
bits of the oracle's f32 restatement of the chain (greedy32), and its picks are replayed against float64 distances under
gamma = 2 (H + 3) 2^-24: three roundings per term (difference, square, addition), at most H - 1 more per sum of non-negative
terms in any order, one for the weight; doubled, as tests/neighbors_ref.py doubles its bound."""
import numpy as np
import pytest
import torch

from reactranker_amd import _lib, featurization, synth
from reactranker_amd import neighbors as N
from reactranker_amd import uncertainty as U
from reactranker_amd.base_model import build_model
from reactranker_amd.functions import StepPlan
from oracle import ref_cpu as O
from tests import helpers as Hh
from tests import poison, streams
from tests import selection_ref as S

pytestmark = pytest.mark.gpu

W = N.KCENTER_ROWS_PER_WORKGROUP
KEYS = ("picks", "gain", "min_dist", "assign")


def dev(x, dtype=np.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def run(x, n, init=None, w=None):
    x = dev(x) if isinstance(x, np.ndarray) else x
    res = N.kcenter_greedy(x, n, init_dist=dev(init), weight=dev(w))
    torch.cuda.synchronize()
    P = x.shape[0]
    assert res["picks"].dtype == torch.int64 and res["assign"].dtype == torch.int64
    assert res["gain"].dtype == torch.float32 and res["min_dist"].dtype == torch.float32
    assert tuple(res["picks"].shape) == tuple(res["gain"].shape) == (n,)
    assert tuple(res["min_dist"].shape) == tuple(res["assign"].shape) == (P,)
    return {k: res[k].cpu().numpy() for k in KEYS}


class blocks:
    def __init__(self, b):
        self.b = b

    def __enter__(self):
        assert _lib.lib().rr_kcenter_set_blocks(self.b) == 0 and _lib.lib().rr_kcenter_blocks() == self.b

    def __exit__(self, *a):
        assert _lib.lib().rr_kcenter_set_blocks(0) == 0


def same(got, want, what=""):
    """every output equal as numbers (a NaN equals a NaN); `want` may be float64"""
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k], np.float64), np.asarray(want[k], np.float64), equal_nan=True), (what, k)


def same_bits(got, want, what=""):
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


def int_case(seed, P, H):
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (P, H)).astype(np.float32)
    for j in range(min(9, P)):                                       # planted duplicate rows
        x[(7 * j + 3) % P] = x[(5 * j) % P]
    w = rng.integers(1, 4, P).astype(np.float32)
    init = rng.integers(0, 4 * H + 2, P).astype(np.float32)
    return x, w, init


# ---------------------------------------------------------------------------------------------- 1. exact inputs, exact answer
def _exact_cases():
    cases = [dict(P=131, H=h, n=20, B=0) for h in (1, 3, 4, 5, 30, 252, 256, 257, 260, 300, 322, 600)]
    cases += [dict(P=67, H=h, n=9, B=0) for h in (1024, 1025, 1100)]          # the last register width, then the loop for wider rows
    for B in (1, 2):
        for P in (1, W - 1, W, W + 1, 3 * W * B + 5):
            cases += [dict(P=P, H=30, n=n, B=B) for n in sorted({0, 1, max(P - 1, 0), P, P + 3})]
    cases += [dict(P=P, H=30, n=P + 3, B=4096) for P in (1, W + 1)]
    cases += [dict(P=3 * W * 4096 + 5, H=5, n=3, B=4096), dict(P=517, H=1, n=40, B=3), dict(P=517, H=4, n=64, B=0)]
    return cases


@pytest.mark.parametrize("c", _exact_cases(), ids=lambda c: "P{P}_H{H}_n{n}_B{B}".format(**c))
def test_exact_inputs_give_the_exact_answer(c):
    x, w, init = int_case(11 + c["P"] + c["H"], c["P"], c["H"])
    tx = dev(x)
    tied = False
    for ww, ii in ((None, None), (w, init), (w, None), (None, init)):
        want = S.greedy64(x, c["n"], ii, ww)
        with blocks(c["B"]):
            got = run(tx, c["n"], ii, ww)
        same(got, want, ("weights" if ww is not None else "") + (" init" if ii is not None else ""))
        tied = tied or bool(want["tied"][1:].any())                  # (round 0 without init_dist is a tie of +inf everywhere)
    if c["H"] <= 4 and c["P"] >= 100:
        assert tied                                                  # at least one pick after round 0 was decided by the index


# ---------------------------------------------------------------------------------------------- 2. random floats
def float_case(seed, P, H, kind):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((P, H))
    if kind == "shifted":
        x = x + 3.0
    elif kind == "scaled":
        x = x * 30.0
    x = x.astype(np.float32)
    for j in range(6):
        x[(11 * j + 2) % P] = x[(3 * j) % P]                         # exact duplicates
    w = rng.uniform(0.5, 2.0, P).astype(np.float32)
    init = None
    if kind == "shifted":                                            # one kind also starts from a labelled set's distances
        init = (rng.uniform(0.5, 3.0, P) * H).astype(np.float32)
    return x, w, init


@pytest.mark.parametrize("H", [1, 3, 4, 30, 300, 322, 600])
def test_random_floats_are_the_chains_bits_and_near_the_float64_optimum(H, parity_log):
    P, n = 517, 40
    g = S.gamma(H)
    worst_gain = worst_opt = 0.0
    for kind in ("normal", "shifted", "scaled"):
        x, w, init = float_case(200 + H, P, H, kind)
        got = run(x, n, init, w)
        want = S.greedy32(x, n, init, w)
        want = {k: want[k].astype(got[k].dtype) for k in KEYS}
        same_bits(got, want, kind)                                                             # (a)
        assert (got["picks"] >= 0).all() and len(set(got["picks"].tolist())) == n
        s64, best = S.replay64(x, got["picks"], init, w)                                       # (b)
        gain = got["gain"].astype(np.float64)
        fin = np.isfinite(s64)
        assert np.array_equal(gain[~fin], s64[~fin]) and np.array_equal(best[~fin], s64[~fin])
        r_gain = float((np.abs(gain[fin] - s64[fin]) / (g * s64[fin])).max()) if (s64[fin] > 0).all() else np.inf
        r_opt = float(((1.0 - s64[fin] / best[fin]) / (2 * g)).max())
        parity_log(f"H {H} {kind}: worst |gain - score64| / (gamma score64) = {r_gain:.4f}, "
                   f"worst (1 - score64 / best64) / (2 gamma) = {r_opt:.4f}")
        worst_gain, worst_opt = max(worst_gain, r_gain), max(worst_opt, r_opt)
        assert (np.abs(gain[fin] - s64[fin]) <= g * s64[fin]).all()
        assert (s64[fin] >= (1.0 - 2 * g) * best[fin]).all()
    Hh.record(f"kcenter H={H}: worst |gain - score64| / (gamma score64)", worst_gain, 1.0)
    Hh.record(f"kcenter H={H}: worst (1 - score64 / best64) / (2 gamma)", worst_opt, 1.0)


# ---------------------------------------------------------------------------------------------- 3. planted clusters, wide gaps
def test_planted_clusters_with_wide_gaps_get_one_pick_each():
    rng = np.random.default_rng(5)
    c, per, H = 12, 40, 30
    centres = 100.0 * rng.standard_normal((c, H))
    member = np.repeat(np.arange(c), per)
    x = (centres[member] + 0.01 * rng.standard_normal((c * per, H))).astype(np.float32)
    perm = rng.permutation(c * per)
    x, member = x[perm], member[perm]
    D = np.stack([S.dist64(x, r) for r in range(len(x))])
    same_cluster = member[:, None] == member[None, :]
    assert D[same_cluster].max() * 1e4 < D[~same_cluster].min()      # the oracle's own precondition: radius far below separation
    got = run(x, c)
    picks = got["picks"]
    assert sorted(member[picks].tolist()) == list(range(c))          # one pick per cluster
    round_of_cluster = np.empty(c, np.int64)
    round_of_cluster[member[picks]] = np.arange(c)
    assert np.array_equal(got["assign"], round_of_cluster[member])   # assign is cluster membership
    assert picks[0] == 0 and np.isinf(got["gain"][0]) and (np.diff(got["gain"]) <= 0).all()
    assert got["min_dist"].max() <= D[same_cluster].max() * (1 + S.gamma(H))


# ---------------------------------------------------------------------------------------------- 4. nothing shows that must not
@pytest.mark.parametrize("H", [322, 300])
def test_position_pitch_alignment_grid_and_repetition_do_not_show(H):
    rng = np.random.default_rng(9 + H)
    P, n = 301, 24
    x = rng.standard_normal((P, H)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, P).astype(np.float32)
    init = (rng.uniform(0.5, 3.0, P) * H).astype(np.float32)         # distinct finite starts: no round is decided by the index
    tx, tw, ti = dev(x), dev(w), dev(init)

    def call(xx, ww=tw, ii=ti, nn=n):
        r = N.kcenter_greedy(xx, nn, init_dist=ii, weight=ww)
        return {k: r[k] for k in KEYS}

    def equal(a, b, what):
        for k in KEYS:
            assert streams.same_bits(a[k], b[k]), (what, k)
    base = call(tx)
    assert not S.greedy32(x, n, init, w)["tied"].any()
    equal(call(tx), base, "run twice")
    for b in (1, 3, 4096):
        with blocks(b):
            equal(call(tx), base, f"blocks {b}")
    assert _lib.lib().rr_kcenter_blocks() == 0
    # the same rows at other positions of a larger pool, in another order; the rows around them cannot be picked (weight 0)
    big = torch.randn(3 * P + 7, H, device="cuda")
    pos = torch.from_numpy(rng.permutation(big.shape[0])[:P]).cuda()
    big[pos] = tx
    bw = torch.zeros(big.shape[0], device="cuda")
    bw[pos] = tw
    bi = torch.full((big.shape[0],), 5.0, device="cuda")
    bi[pos] = ti
    got = call(big, bw, bi)
    assert torch.equal(got["picks"], pos[base["picks"]]) and streams.same_bits(got["gain"], base["gain"])
    assert streams.same_bits(got["min_dist"][pos], base["min_dist"]) and torch.equal(got["assign"][pos], base["assign"])
    # other pitches (the pad columns hold NaN: they never reach a result) and a base pointer 4 bytes off a 16-byte boundary
    for pitch in (H + 2, H + 5, H + 6):
        wide = torch.full((P, pitch), float("nan"), device="cuda")
        wide[:, :H] = tx
        view = wide[:, :H]
        assert view.stride(0) == pitch
        equal(call(view), base, f"pitch {pitch}")
    for pitch in (H, H + 2):
        flat = torch.full((P * pitch + 1,), float("nan"), device="cuda")
        off = flat[1:].view(P, pitch)
        off[:, :H] = tx
        assert off.data_ptr() % 16 == 4
        equal(call(off[:, :H]), base, f"pointer + 4, pitch {pitch}")


# ---------------------------------------------------------------------------------------------- 5. ineligible rows
def test_rows_that_cannot_be_picked():
    P, H = 200, 30
    x, w, init = int_case(23, P, H)
    x[17] = np.nan
    x[40, 3] = np.nan
    x[50, 29] = np.inf
    x[51, 0] = -np.inf
    bad_rows = [17, 40, 50, 51]
    w[[3, 5, 7, 9]] = [0.0, -1.0, np.nan, np.inf]
    bad_w = [3, 5, 7, 9]
    for ii in (None, init):
        want = S.greedy64(x, P + 3, ii, w)
        got = run(x, P + 3, ii, w)
        same(got, want, "ineligible")
        assert np.isnan(got["min_dist"][bad_rows]).all() and (got["assign"][bad_rows] == -1).all()
        assert not np.isin(got["picks"], bad_rows + bad_w).any()
        assert np.isfinite(got["min_dist"][bad_w]).all()
        if ii is None:                                               # (a row that starts nearer than any pick comes keeps assign = -1)
            assert (got["assign"][bad_w] >= 0).all()
        assert (got["picks"] >= 0).sum() == P - 8 and (got["picks"][P - 8:] == -1).all() and (got["gain"][P - 8:] == -1).all()
    # without weights only the non-finite rows are out
    got = run(x, P, None, None)
    same(got, S.greedy64(x, P, None, None), "non-finite rows")
    assert (got["picks"] >= 0).sum() == P - 4
    # nobody is eligible: all padding, the state stays as it started
    for ww in (np.zeros(P, np.float32), np.full(P, np.nan, np.float32)):
        got = run(x, 5, init, ww)
        assert (got["picks"] == -1).all() and (got["gain"] == -1).all() and (got["assign"] == -1).all()
        keep = np.ones(P, bool)
        keep[bad_rows] = False
        assert np.array_equal(got["min_dist"][keep], init[keep]) and np.isnan(got["min_dist"][bad_rows]).all()
    got = run(np.full((3, 4), np.nan, np.float32), 2)
    assert (got["picks"] == -1).all() and np.isnan(got["min_dist"]).all()
    # an empty pool: padding only; and nothing at all
    got = run(np.zeros((0, H), np.float32), 3)
    assert got["picks"].tolist() == [-1] * 3 and got["gain"].tolist() == [-1.0] * 3 and got["min_dist"].shape == (0,)
    got = run(np.zeros((0, H), np.float32), 0)
    assert got["picks"].shape == (0,) and got["assign"].shape == (0,)


# ---------------------------------------------------------------------------------------------- 6. what memory held, stream order
@pytest.mark.parametrize("shape", [(301, 16, 0), (3, 8, 0), (301, 16, 3)], ids=["auto", "padded", "blocks3"])
def test_nothing_depends_on_what_memory_held(shape):
    P, n, b = shape
    rng = np.random.default_rng(31)
    tx = dev(rng.standard_normal((P, 30)))
    tw, ti = dev(rng.uniform(0.5, 2.0, P)), dev(rng.uniform(1.0, 50.0, P))
    with blocks(b):
        report, counters, last = poison.fill_dependence(lambda: N.kcenter_greedy(tx, n, init_dist=ti, weight=tw),
                                                        sync=torch.cuda.synchronize)
    assert not report, report
    assert counters[0xFF].buffers >= 5                               # picks, gain, min_dist, assign and the workspace were all poisoned
    assert not torch.isnan(last["min_dist"]).any() and (last["assign"] >= -1).all()
    if P < n:
        assert (last["picks"][P:] == -1).all() and (last["gain"][P:] == -1).all() and (last["picks"][:P] >= 0).all()


def _stream_cases():
    def build_for(weighted):
        def build():
            rng = np.random.default_rng(41)
            x = dev(rng.standard_normal((600, 30)))
            init = dev(rng.uniform(1.0, 50.0, 600))
            w = dev(rng.uniform(0.5, 2.0, 600))

            def fn(inputs):
                if weighted:
                    return N.kcenter_greedy(inputs[0], 32, init_dist=inputs[1], weight=inputs[2])
                return N.kcenter_greedy(inputs[0], 32, init_dist=inputs[1])
            return ([x, init, w] if weighted else [x, init]), fn
        return build
    return [streams.Case("rr_kcenter_f32", build_for(False)), streams.Case("rr_kcenter_f32 weighted", build_for(True))]


@pytest.mark.parametrize("case", _stream_cases(), ids=lambda c: c.name)
def test_the_call_is_ordered_on_the_callers_stream(case, parity_log):
    streams.check_table("kcenter", _stream_cases())
    res = streams.staged(case, log=parity_log)
    assert res.status == "armed"


# ---------------------------------------------------------------------------------------------- 7. acquire
def _model(wseed, task_num=1, task_type=None):
    m = build_model(hidden_size=64, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, task_num=task_num,
                    ffn_last_layer="with_softplus", task_type=task_type, add_features_dim=1, dropout=0.1)
    m.load_state_dict({k: torch.tensor(v) for k, v in synth.seeded_weights(O.model_shapes(64, 3, 3, 3, task_num, 1, True), wseed).items()})
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


def _equal_to_greedy(res, want):
    assert torch.equal(res["rows"], want["picks"]) and streams.same_bits(res["gain"], want["gain"])
    assert streams.same_bits(res["min_dist"], want["min_dist"]) and torch.equal(res["assign"], want["assign"])


def test_acquire_is_kcenter_greedy_on_the_models_vectors(bank_case):
    model, train, bank = bank_case
    full = [_batch(81), _batch(82, nq=4)]
    pool = [full[0], (None, None, [], None, None), full[1][:3] + (None,) + full[1][4:]]        # an empty batch; targets may be None
    model.train()
    before = StepPlan.last
    assert StepPlan.keep_last is False
    n = 10
    res = N.acquire(model, bank, pool, n, 0)
    assert model.training and StepPlan.keep_last is False and StepPlan.last is before
    vec = N.reaction_vectors(model, full, 0)
    init = bank.query(vec, 1)[0][:, 0].contiguous()
    want = N.kcenter_greedy(vec, n, init_dist=init)
    _equal_to_greedy(res, want)
    assert streams.same_bits(res["init_dist"], init)                 # (no reaction of this pool is in the bank)
    rows = res["rows"].cpu().numpy()
    assert (rows >= 0).all() and len(set(rows.tolist())) == n
    where = [(j, q, c) for j, b in enumerate(full) for q, size in enumerate(b[2]) for c in range(size)]
    assert [tuple(t) for t in torch.stack([res["batch"], res["query"], res["candidate"]], 1).cpu().tolist()] == [where[r] for r in rows]
    assert float(res["radius_before"]) == float(init.max().sqrt()) and float(res["radius_after"]) == float(want["min_dist"].max().sqrt())
    assert float(res["radius_after"]) <= float(res["radius_before"])
    # a weight per row, and more picks than rows: padding carries -1 everywhere
    wt = torch.rand(vec.shape[0], device="cuda") + 0.5
    res = N.acquire(model, bank, pool, vec.shape[0] + 2, 0, weight=wt)
    _equal_to_greedy(res, N.kcenter_greedy(vec, vec.shape[0] + 2, init_dist=init, weight=wt))
    for key in ("rows", "batch", "query", "candidate"):
        assert res[key][-2:].cpu().tolist() == [-1, -1] and (res[key][:-2] >= 0).all(), key
    assert float(res["radius_after"]) == 0.0
    # an empty bank: every row starts at +inf
    empty = N.ReactionBank(bank.vectors[:0], torch.zeros(0), torch.zeros(0, dtype=torch.int32))
    res = N.acquire(model, empty, pool, 4, 0)
    _equal_to_greedy(res, N.kcenter_greedy(vec, 4))
    assert torch.isinf(res["radius_before"]) and torch.isfinite(res["radius_after"]) and res["rows"][0] == 0
    assert torch.isinf(res["init_dist"]).all() and res["init_dist"].shape == res["min_dist"].shape
    with pytest.raises(ValueError, match="weight"):
        N.acquire(model, bank, pool, 4, 0, weight="variance")


def test_acquire_from_the_banks_own_reactions_picks_in_index_order(bank_case, parity_log):
    """With the pool equal to the bank's own batches every init_dist is 0 and the picks come in index order.  knn alone does
    not give that: its distance is max(0, (|q|^2 + |b|^2) - 2 q.b), and for b = q the norms (64 lane chains) and the dot product
    (the matrix core's k-tile chain) round differently - measured here, 54 of the 148 rows come back at one to three times
    2^-21, within knn's bound 2 (H + 3) 2^-24 (|q|^2 + |b|^2) of 0, on which acquire first picked [13, 18, 41, 0, 8, 16].
    acquire therefore starts a pool row whose nearest bank row holds the same bits at exactly 0."""
    model, train, bank = bank_case
    res = N.acquire(model, bank, train, 6, 0)
    raw = bank.query(bank.vectors, 1)[0][:, 0]
    parity_log(f"knn distance of the bank's own rows to the bank: max {float(raw.max()):.3e}, non-zero {int((raw != 0).sum())} of {raw.numel()}")
    parity_log(f"picks {res['rows'].cpu().tolist()}, radius before {float(res['radius_before']):.3e}, after {float(res['radius_after']):.3e}")
    assert (raw.double() <= 2 * (64 + 3) * 2.0 ** -24 * 2 * bank.sqnorm.double()).all() and (raw >= 0).all()
    assert tuple(res["init_dist"].shape) == (len(bank),) and (res["init_dist"] == 0).all()
    assert res["rows"].cpu().tolist() == list(range(6)) and (res["gain"] == 0).all()
    assert (res["min_dist"] == 0).all() and (res["assign"] == -1).all()
    assert float(res["radius_before"]) == 0.0 == float(res["radius_after"])


def test_acquire_takes_labelled_reactions_last(bank_case):
    """A pool that mixes reactions of the bank with new ones: the labelled rows start at 0, the new rows at knn's distance (the
    same bits), and no labelled row is taken while a new one is left."""
    model, train, bank = bank_case
    new = _batch(81)
    pool = [train[1], new]
    n_old, n_new = int(sum(train[1][2])), int(sum(new[2]))
    res = N.acquire(model, bank, pool, n_new + 3, 0)
    vec = N.reaction_vectors(model, pool, 0)
    raw = bank.query(vec, 1)[0][:, 0]
    assert (res["init_dist"][:n_old] == 0).all() and (raw[n_old:] > 0).all()
    assert streams.same_bits(res["init_dist"][n_old:], raw[n_old:])
    _equal_to_greedy(res, N.kcenter_greedy(vec, n_new + 3, init_dist=res["init_dist"]))
    rows, gain = res["rows"].cpu().numpy(), res["gain"].cpu().numpy()
    assert (rows >= 0).all() and len(set(rows.tolist())) == n_new + 3 and (np.diff(gain) <= 0).all()
    assert gain[0] > 0 and (rows[gain > 0] >= n_old).all()           # whatever scored above 0 was a new reaction
    old = rows[rows < n_old]
    assert len(old) >= 3 and (gain[rows < n_old] == 0).all() and (np.diff(old) > 0).all()   # labelled ones: at 0, in index order


def test_acquire_weighted_by_the_heads_own_std():
    model = _model(11, 2, "evidential_ranking").train()
    train, pool = [_batch(61)], [_batch(81), _batch(82, nq=4)]
    bank = N.ReactionBank.from_batches(model, train, 0)
    res = N.acquire(model, bank, pool, 8, 0, weight="std")
    assert model.training
    std = torch.cat([r["std"] for r in U.distribution_predict(model, pool, gpu=0)])
    assert std.dtype == torch.float32 and (std > 0).all() and float(std.max()) > float(std.min())
    want = N.acquire(model, bank, pool, 8, 0, weight=std)
    for key in ("rows", "batch", "query", "candidate", "gain", "min_dist", "assign", "radius_before", "radius_after", "init_dist"):
        assert streams.same_bits(res[key], want[key]), key
    mle = _model(41)
    with pytest.raises(ValueError, match="head"):
        N.acquire(mle, N.ReactionBank.from_batches(mle, train, 0), pool, 8, 0, weight="std")
