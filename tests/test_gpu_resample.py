"""Resampled column means on the GPU (reactranker_amd.significance, rr_resample_means_f64) against the
numpy oracle of tests/resample_ref.py.

Integer tables with values in [-8, 8] make every sum exact, so those cases must equal the oracle exactly in both modes.  On
random floats the kernel's means must be the BITS of the oracle's restatement of the 64 lane chains and the butterfly
(means_chain), and lie within Q 2^-53 sum|x drawn| / n plus one rounding of the quotient of the exactly rounded means
(means_fsum).  The shapes are the smallest at which the kernel can go wrong: Q around the 64-lane and the 128-position
step, odd Q (the word-boundary padding), M on both sides of every column-group width (4, 8, 16), one or several grid passes."""
import numpy as np
import pytest
import torch

from reactranker_amd import _lib, eval as E, featurization, synth
from reactranker_amd import significance as S
from reactranker_amd.base_model import build_model
from tests import helpers as Hh
from tests import poison, streams
from tests import resample_ref as R

pytestmark = pytest.mark.gpu

MODES = (("bootstrap", R.BOOTSTRAP), ("signflip", R.SIGNFLIP))
OK, ARG, UNSUPPORTED = 0, -1, -4


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda()


def run(x, B, seed=0, mode="bootstrap", first=0):
    x = dev(x) if isinstance(x, np.ndarray) else x
    m, n = S.resample_means(x, B, seed=seed, mode=mode, first=first)
    torch.cuda.synchronize()
    M = 1 if x.dim() == 1 else x.shape[1]
    assert m.dtype == torch.float64 and n.dtype == torch.int32 and tuple(m.shape) == tuple(n.shape) == (B, M)
    return m, n


class blocks:
    def __init__(self, b):
        self.b = b

    def __enter__(self):
        assert _lib.lib().rr_resample_set_blocks(self.b) == 0 and _lib.lib().rr_resample_blocks() == self.b

    def __exit__(self, *a):
        assert _lib.lib().rr_resample_set_blocks(0) == 0


def raw(x, ld, Q, M, mode, seed, b0, B, mean, count):
    """the C entry point itself, on the current stream"""
    return _lib.lib().rr_resample_means_f64(_lib.ptr(x), ld, Q, M, mode, seed, b0, B, _lib.ptr(mean), _lib.ptr(count), _lib.stream())


def equal_to_ref(got, want, what=""):
    m, n = got
    assert torch.equal(n.cpu(), torch.from_numpy(want[1])), (what, "counts")
    assert streams.same_bits(m.cpu(), torch.from_numpy(want[0])), (what, "means")


# ---------------------------------------------------------------------------------------------- 1. exact inputs, exact answer
@pytest.mark.parametrize("Q", [1, 2, 63, 64, 65, 129, 1000])
def test_integer_tables_give_the_exact_answer(Q):
    rng = np.random.default_rng(Q)
    for M in (1, 3, 12, 32):
        x = rng.integers(-8, 9, (Q, M)).astype(np.float64)
        tx = dev(x)
        for B in (1, 5, 37):
            for name, mode in MODES:
                m, n = run(tx, B, seed=Q + M, mode=name)
                wm, wn = R.means_chain(x, B, seed=Q + M, mode=mode)
                assert torch.equal(m.cpu(), torch.from_numpy(wm)) and torch.equal(n.cpu(), torch.from_numpy(wn)), (M, B, name)
                if B == 5:
                    assert np.array_equal(wm, R.means_fsum(x, B, seed=Q + M, mode=mode)[0])      # the oracle's own exactness


def test_an_identity_table_counts_the_draws_of_every_row():
    Q = 32
    m, n = run(np.eye(Q), 37, seed=5)
    want = np.stack([np.bincount(R.rows(5, b, Q), minlength=Q) for b in range(37)]).astype(np.float64)
    assert torch.equal(m.cpu() * Q, torch.from_numpy(want)) and (n == Q).all() and want.sum(axis=1).tolist() == [Q] * 37
    m, _ = run(np.eye(Q), 37, seed=5, mode="signflip")
    want = np.stack([R.signs(5, b, Q) for b in range(37)])
    assert torch.equal(m.cpu() * Q, torch.from_numpy(want))


# ---------------------------------------------------------------------------------------------- 2. random floats
@pytest.mark.parametrize("shape", [(65, 3), (129, 12), (1000, 32)], ids=lambda s: "Q{}_M{}".format(*s))
def test_random_floats_are_the_chains_bits_and_near_the_exact_sums(shape, parity_log):
    Q, M = shape
    rng = np.random.default_rng(Q + M)
    x = rng.standard_normal((Q, M)) * np.exp(rng.standard_normal((Q, M)))
    x[:, 0] += 3.0
    B = 37
    for name, mode in MODES:
        got = run(x, B, seed=17, mode=name)
        equal_to_ref(got, R.means_chain(x, B, seed=17, mode=mode), name)
        mf, nf, mass = R.means_fsum(x, B, seed=17, mode=mode)
        bound = Q * 2.0 ** -53 * mass / nf + 2.0 ** -53 * np.abs(mf)
        err = np.abs(got[0].cpu().numpy() - mf)
        worst = float((err / bound).max())
        parity_log(f"Q {Q} M {M} {name}: worst |mean - fsum mean| / bound = {worst:.4f}, "
                   f"largest |mean - fsum mean| = {float(err.max()):.3e} ({int((err == 0).sum())} of {err.size} equal)")
        Hh.record(f"resample Q={Q} M={M} {name}: |mean - fsum mean| / (Q 2^-53 sum|x| / n + 2^-53 |mean|)", worst, 1.0)
        assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------- 3. nothing shows that must not
@pytest.mark.parametrize("name", ["bootstrap", "signflip"])
def test_pitch_alignment_grid_cut_and_repetition_do_not_show(name):
    Q, M, B, seed = 129, 12, 37, 23
    mode = dict(MODES)[name]
    x = np.random.default_rng(7).standard_normal((Q, M))
    tx = dev(x)
    base = run(tx, B, seed, name)
    equal_to_ref(base, R.means_chain(x, B, seed=seed, mode=mode))

    def same(got, what):
        assert streams.same_bits(got[0], base[0]) and torch.equal(got[1], base[1]), what
    same(run(tx, B, seed, name), "two successive calls")
    for ld in (M + 1, M + 5):                                          # the padding columns hold NaN and never reach a result
        wide = torch.full((Q, ld), float("nan"), dtype=torch.float64, device="cuda")
        wide[:, :M] = tx
        view = wide[:, :M]
        assert view.stride(0) == ld
        same(run(view, B, seed, name), f"ld {ld}")
    for ld in (M, M + 1, M + 5):                                       # 8-byte but not 16-byte aligned
        flat = torch.full((Q * ld + 1,), float("nan"), dtype=torch.float64, device="cuda")
        off = flat[1:].view(Q, ld)
        off[:, :M] = tx
        assert off.data_ptr() % 16 == 8
        same(run(off[:, :M], B, seed, name), f"pointer + 8, ld {ld}")
    for b in (0, 1, 2, 7, 4096):                                       # blocks = 2: 8 waves, five grid passes
        with blocks(b):
            same(run(tx, B, seed, name), f"blocks {b}")
    assert _lib.lib().rr_resample_blocks() == 0
    # a cut of B: rows 0..9 of one call against (first 0, B 4) and (first 4, B 6)
    whole = run(tx, 10, seed, name)
    a, b = run(tx, 4, seed, name, first=0), run(tx, 6, seed, name, first=4)
    assert streams.same_bits(torch.cat([a[0], b[0]]), whole[0]) and torch.equal(torch.cat([a[1], b[1]]), whole[1])
    assert streams.same_bits(whole[0], base[0][:10])
    # count = NULL leaves mean as it is with counts
    mean = torch.full((B, M), -1.0, dtype=torch.float64, device="cuda")
    assert raw(tx, M, Q, M, mode, seed, 0, B, mean, None) == OK
    torch.cuda.synchronize()
    assert streams.same_bits(mean, base[0])
    # a non-unit column stride is made contiguous by the wrapper
    same(run(dev(x.T.copy()).t(), B, seed, name), "transposed storage")


def test_resample_numbers_beyond_32_bits():
    x = np.random.default_rng(1).integers(-8, 9, (5, 2)).astype(np.float64)
    for name, mode in MODES:
        equal_to_ref(run(x, 3, seed=9, mode=name, first=2 ** 33), R.means_chain(x, 3, seed=9, mode=mode, first=2 ** 33), name)
    assert not np.array_equal(R.means_chain(x, 3, seed=9, first=2 ** 33)[0], R.means_chain(x, 3, seed=9, first=0)[0])


# ---------------------------------------------------------------------------------------------- 4. NaN tables, column groups, limits
def test_nan_entries_are_left_out_and_counted():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((129, 5))
    x[rng.random((129, 5)) < 0.2] = np.nan
    x[:, 2] = np.nan                                                   # an all-NaN column
    x[3, 4] = np.inf                                                   # an infinity takes part in the sums
    for name, mode in MODES[:1]:
        got = run(x, 37, seed=1, mode=name)
        equal_to_ref(got, R.means_chain(x, 37, seed=1, mode=mode), name)
        assert torch.isnan(got[0][:, 2]).all() and (got[1][:, 2] == 0).all()
        assert torch.isinf(got[0][:, 4]).any() and torch.isfinite(got[0][:, 4]).any()
    x[3, 4] = 1.0
    got = run(x, 37, seed=1, mode="signflip")
    equal_to_ref(got, R.means_chain(x, 37, seed=1, mode=R.SIGNFLIP), "signflip")
    assert torch.equal(got[1].cpu(), torch.from_numpy((~np.isnan(x)).sum(axis=0).astype(np.int32)).expand(37, 5))
    y = np.full((3, 2), np.nan)                                        # a column finite in one row only
    y[1, 0], y[:, 1] = 5.0, [1.0, 2.0, 3.0]
    got = run(y, 64, seed=3)
    want = R.means_chain(y, 64, seed=3)
    equal_to_ref(got, want, "one finite row")
    assert np.isnan(want[0][:, 0]).any() and (want[0][:, 0] == 5.0).any()


@pytest.mark.parametrize("M", [2, 4, 5, 7, 8, 9, 16, 17, 20, 31])
def test_every_column_group_width_and_both_load_widths(M):
    Q, B = 131, 9
    x = np.random.default_rng(M).standard_normal((Q, M))
    x[5, M - 1] = np.nan
    flat = torch.zeros(Q * (M + 1) + 1, dtype=torch.float64, device="cuda")
    views = {"16-byte": dev(x) if M % 2 == 0 else None, "8-byte": flat[1:1 + Q * M].view(Q, M),
             "16-byte, odd tail": flat[:Q * (M + 1)].view(Q, M + 1)[:, :M] if M % 2 == 1 else None}
    for name, mode in MODES:
        want = R.means_chain(x, B, seed=M, mode=mode)
        for what, v in views.items():
            if v is None:
                continue
            v.copy_(dev(x))
            equal_to_ref(run(v, B, seed=M, mode=name), want, (name, what))


def test_the_row_limit_and_the_refusals_above_the_limits():
    Q = 2 ** 20
    x = np.random.default_rng(2).integers(-8, 9, Q).astype(np.float64)
    tx = dev(x)
    for name, mode in MODES:
        m, n = run(tx, 2, seed=3, mode=name)
        wm, wn = R.means_chain(x, 2, seed=3, mode=mode)
        assert torch.equal(m.cpu(), torch.from_numpy(wm)) and torch.equal(n.cpu(), torch.from_numpy(wn)), name
    # above the limits: the status, nothing launched, the outputs as they were
    big = torch.zeros(Q + 1, dtype=torch.float64, device="cuda")
    mean = torch.full((2, 33), -7.0, dtype=torch.float64, device="cuda")
    count = torch.full((2, 33), -7, dtype=torch.int32, device="cuda")
    assert raw(big, 1, Q + 1, 1, 0, 3, 0, 2, mean, count) == UNSUPPORTED
    assert raw(big, 33, 100, 33, 0, 3, 0, 2, mean, count) == UNSUPPORTED
    assert raw(big, 1, 4, 1, 0, 3, 2 ** 61, 2, mean, count) == UNSUPPORTED
    assert raw(big, 1, 4, 1, 2, 3, 0, 2, mean, count) == ARG
    torch.cuda.synchronize()
    assert (mean == -7.0).all() and (count == -7).all()
    with pytest.raises(ValueError, match="2\\^20"):
        S.resample_means(big, 2)
    with pytest.raises(ValueError, match="columns"):
        S.resample_means(torch.zeros(4, 33, dtype=torch.float64, device="cuda"), 2)
    with pytest.raises(ValueError, match="float64"):
        S.resample_means(torch.zeros(4, 3, device="cuda"), 2)
    with pytest.raises(ValueError, match="mode"):
        S.resample_means(big[:4], 2, mode="jackknife")


def test_empty_inputs():
    for name, _ in MODES:
        m, n = run(torch.zeros(0, 3, dtype=torch.float64, device="cuda"), 5, mode=name)
        assert torch.isnan(m).all() and (n == 0).all()
        m, n = run(torch.zeros(7, 3, dtype=torch.float64, device="cuda"), 0, mode=name)
        assert tuple(m.shape) == (0, 3) and tuple(n.shape) == (0, 3)
    mean = torch.full((1, 3), -7.0, dtype=torch.float64, device="cuda")
    assert raw(None, 3, 0, 3, 0, 1, 0, 1, mean, None) == OK             # Q == 0 needs no table
    assert raw(None, 3, 0, 3, 0, 1, 0, 0, mean, None) == OK and raw(None, 3, 1, 3, 0, 1, 0, 1, mean, None) == ARG
    torch.cuda.synchronize()
    assert torch.isnan(mean).all()


# ---------------------------------------------------------------------------------------------- 5. what memory held, stream order
@pytest.mark.parametrize("name", ["bootstrap", "signflip"])
def test_nothing_depends_on_what_memory_held(name):
    Q, M, B = 129, 12, 37
    x = np.random.default_rng(31).standard_normal((Q, M))
    x[7, 3] = np.nan
    want = R.means_chain(x, B, seed=2, mode=dict(MODES)[name])
    for pad in (float("nan"), 1e300):                                  # the padding columns of x are poisoned as well
        wide = torch.full((Q, M + 3), pad, dtype=torch.float64, device="cuda")
        wide[:, :M] = dev(x)
        report, counters, last = poison.fill_dependence(lambda: S.resample_means(wide[:, :M], B, seed=2, mode=name),
                                                        sync=torch.cuda.synchronize)
        assert not report, report
        assert counters[0xFF].buffers >= 2                             # means and counts were both poisoned
        equal_to_ref(last, want, name)


def _stream_cases():
    def build_for(name):
        def build():
            x = dev(np.random.default_rng(41).standard_normal((600, 12)))
            return [x], lambda inputs: S.resample_means(inputs[0], 64, seed=3, mode=name)
        return build
    return [streams.Case("rr_resample_means_f64 bootstrap", build_for("bootstrap")),
            streams.Case("rr_resample_means_f64 signflip", build_for("signflip"))]


@pytest.mark.parametrize("case", _stream_cases(), ids=lambda c: c.name)
def test_the_call_is_ordered_on_the_callers_stream(case, parity_log):
    streams.check_table("resample", _stream_cases())
    res = streams.staged(case, log=parity_log)
    assert res.status == "armed"


# ---------------------------------------------------------------------------------------------- 6. the Python layer
def _close(got, want, what):
    assert got == pytest.approx(want, abs=1e-12, nan_ok=True), (what, got, want)


def test_bootstrap_ci_and_paired_test_equal_the_oracle():
    Q, M, B = 64, 4, 500
    rng = np.random.default_rng(12)
    x = rng.exponential(1.0, (Q, M))
    x[rng.random((Q, M)) < 0.1] = np.nan
    boot_seed, flip_seed = S.sample_seed(5, 0), S.sample_seed(5, 1)
    assert boot_seed != flip_seed
    means, _ = R.means_chain(x, B, seed=boot_seed)
    names = ["a", "b", "c", "d"]
    for method in ("percentile", "bca"):
        got = S.bootstrap_ci(dev(x), B, level=0.9, method=method, seed=5, names=names)
        assert list(got) == names
        for c, name in enumerate(names):
            col = x[:, c][~np.isnan(x[:, c])]
            fin = means[:, c][np.isfinite(means[:, c])]
            want = R.percentile_ci(means[:, c], 0.9) if method == "percentile" else R.bca_ci(x[:, c], means[:, c], 0.9)[:2]
            g = got[name]
            _close(g["estimate"], col.mean(), "estimate")
            _close(g["se"], fin.std(ddof=1), "se")
            _close((g["lo"], g["hi"]), want, method)
            assert g["n"] == len(col) and g["n_nan_resamples"] == B - len(fin) == 0
            assert g["lo"] < g["estimate"] < g["hi"]
    # a ratio statistic: the interval of col0 / col1 from the same resamples
    ratio = S.bootstrap_ci(dev(x), B, level=0.9, seed=5, statistic=lambda m: (m[:, 0] / m[:, 1])[:, None], names=["ratio"])["ratio"]
    r = means[:, 0] / means[:, 1]
    _close((ratio["lo"], ratio["hi"]), R.percentile_ci(r, 0.9), "ratio")
    _close(ratio["estimate"], np.nanmean(x[:, 0]) / np.nanmean(x[:, 1]), "ratio estimate")
    assert ratio["n"] == Q
    # the paired test
    y = x + 0.3 * rng.standard_normal((Q, M))
    y[:, 3] = x[:, 3]                                                  # one column where the two models agree everywhere
    y[rng.random((Q, M)) < 0.05] = np.nan
    d = x - y
    got = S.paired_test(dev(x), dev(y), B, level=0.9, seed=5, names=names)
    bm, _ = R.means_chain(d, B, seed=boot_seed)
    fm, _ = R.means_chain(d, B, seed=flip_seed, mode=R.SIGNFLIP)
    for c, name in enumerate(names):
        ok = ~np.isnan(d[:, c])
        g = got[name]
        _close(g["diff"], d[ok, c].mean(), "diff")
        _close(g["mean_a"], x[ok, c].mean(), "mean_a")
        _close(g["mean_b"], y[ok, c].mean(), "mean_b")
        _close((g["lo"], g["hi"]), R.percentile_ci(bm[:, c], 0.9), "interval of diff")
        _close(g["p_value"], R.signflip_p(d[:, c], fm[:, c]), "p")
        assert (g["wins"], g["ties"], g["losses"]) == (int((d[ok, c] > 0).sum()), int((d[ok, c] == 0).sum()), int((d[ok, c] < 0).sum()))
        assert g["n"] == int(ok.sum()) == g["wins"] + g["ties"] + g["losses"]
    assert got["d"]["p_value"] == 1.0 and got["d"]["diff"] == 0.0 and got["d"]["lo"] == got["d"]["hi"] == 0.0
    assert got["d"]["ties"] == got["d"]["n"]
    # integer differences: the count behind p is exact
    di = rng.integers(-3, 4, (Q, 2)).astype(np.float64)
    got = S.paired_test(dev(di), dev(np.zeros((Q, 2))), B, seed=8)
    fm, _ = R.means_chain(di, B, seed=S.sample_seed(8, 1), mode=R.SIGNFLIP)
    _close([got[k]["p_value"] for k in ("col0", "col1")], [R.signflip_p(di[:, c], fm[:, c]) for c in range(2)], "p on integers")


def _model(seed):
    torch.manual_seed(seed)
    return build_model(task_num=1, ffn_last_layer="no_softplus", add_features_dim=1, hidden_size=32, mpnn_depth=2,
                       mpnn_diff_depth=2, ffn_depth=2, use_bias=True, dropout=0.0).cuda()


def _batches():
    out = []
    for seed, nq in ((61, 5), (62, 3)):                                # 8 queries of 6 candidates, in two batches
        qb = synth.make_queries(seed, nq, [6] * nq, atoms_lo=5, atoms_hi=9)
        out.append((featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs), qb.scope,
                    torch.tensor(qb.targets), qb.add_features))
    return out


class _OneQueryReversed(torch.nn.Module):
    """the wrapped model with the scores of the first query of every batch in reverse order"""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, r, p, gpu=None, add_features=None):
        out = self.model(r, p, gpu=gpu, add_features=add_features)
        out = out.clone()
        out[:6] = out[:6].flip(0)
        return out


def test_query_table_intervals_and_model_comparison():
    model, batches = _model(3), _batches()
    model.train()
    table, names = S.query_table(model, 0, batches)
    assert model.training and tuple(table.shape) == (8, 12) and table.dtype == torch.float64 and names == list(S.TABLE_NAMES)
    model.eval()
    with torch.no_grad():
        outs = [model(b[0], b[1], gpu=0, add_features=b[4]) for b in batches]
    rs = torch.cat([E.ranking_stats(o, b[2], b[3], 0)[0] for o, b in zip(outs, batches)])
    rc = torch.cat([E.rank_correlation_stats(o, b[2], b[3], 0) for o, b in zip(outs, batches)])
    assert streams.same_bits(table[:, :8], rs[:, :8]) and streams.same_bits(table[:, 8:], rc[:, :4])
    # intervals: the estimates are the means every other consumer reports; the pooled tau-b is the ratio of the summed counts
    iv = S.metric_intervals(model, 0, batches, n_resamples=200, seed=1)
    assert list(iv) == list(S.TABLE_NAMES) + ["kendall_tau_pooled"]
    want = E.rank_correlation(model, 0, batches)
    assert iv["kendall_tau_pooled"]["estimate"] == want["kendall_tau_pooled"]      # (8 queries: the division by Q is exact)
    for k in ("kendall_tau", "spearman", "mrr", "regret"):
        assert iv[k]["estimate"] == pytest.approx(want[k], abs=1e-12)
    top1 = E.ranking_metrics(model, 0, batches)[0]
    assert iv["top1"]["estimate"] == pytest.approx(top1, abs=1e-12)
    for k, v in iv.items():
        assert v["lo"] <= v["hi"] and v["n"] == 8 and v["n_nan_resamples"] == 0, k
    assert iv["kendall_tau_pooled"]["lo"] < iv["kendall_tau_pooled"]["hi"] and iv["kendall_tau_pooled"]["n"] == 8
    # a model against itself
    same = S.compare_models(model, model, 0, batches, n_resamples=200, seed=1)
    assert list(same) == list(S.TABLE_NAMES)
    for k, v in same.items():
        assert v["n"] > 0 and v["diff"] == 0.0 and v["p_value"] == 1.0 and v["lo"] == v["hi"] == 0.0, (k, v)
        assert v["ties"] == v["n"] and v["wins"] == v["losses"] == 0
    # against itself with the scores of two queries reversed
    other = S.compare_models(model, _OneQueryReversed(model), 0, batches, n_resamples=200, seed=1)
    for k, v in other.items():
        assert v["wins"] + v["ties"] + v["losses"] == v["n"] and 0.0 < v["p_value"] <= 1.0, (k, v)
        assert v["ties"] >= v["n"] - 2
    assert other["kendall_tau"]["n"] == 8 and other["kendall_tau"]["ties"] == 6
    assert other["kendall_tau"]["mean_a"] == pytest.approx(want["kendall_tau"], abs=1e-12)
    assert other["kendall_tau"]["mean_b"] != other["kendall_tau"]["mean_a"]
