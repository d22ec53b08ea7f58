"""GPU tests of the calibration entries (csrc/calibration.hip) against the float64 restatement of
tests/calibration_ref.py, and of uncertainty.evaluate_calibration end to end on two small trained models.

Bounds.  rr_gauss_calibration_f64: the two counts are exact; each of the six sums lies within n * 2^-52 * sum |term| of the
restatement's, the worst-case difference of two summation orders of n terms; the PIT histogram is exact except for rows the
restatement marks as lying within 1e-9 of a bin edge, at most 0.1 % of the rows (the generator's inputs have none:
tests/test_calibration_cpu.py).  rr_top1_sets_f32: rank, in_set and the integer statistics are exact, and `before`, the
confidence, the two probabilities, the Brier score, E and the mass are ordered float64 sums, compared BIT for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import calibration_ref as CR
from tests import helpers as Hh
from tests.test_gpu_lambdarank import seg_of, windows

from reactranker_amd import _lib
from reactranker_amd import train_listwise as TL
from reactranker_amd import train_utils as TU
from reactranker_amd import uncertainty as U
from reactranker_amd.base_model import build_model
from reactranker_amd.utils import save_checkpoint

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
GAUSS_SIZES = (1, 255, 256, 257, 65537)
GAUSS_BINS = (1, 10, 20, 64)
GAUSS_SCALES = (1.0, 1.7)
TAUS = (0.0, 0.5, 0.9375, 1.0, float("inf"))
RAGGED = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 300]   # crosses the wave (64) and workgroup (256) boundaries
WINDOWS = {"ragged": RAGGED, "64x64": [64] * 64, "1000": [1000], "8192": [8192]}
KINDS = ("shares", "softmax")
BIT_STATS, EXACT_STATS = [1, 2, 4, 5, 8], [0, 3, 6, 7]


def dev(a, dtype=np.float32):
    return torch.tensor(np.asarray(a, dtype)).cuda()


# ------------------------------------------------------------------------------------------------ 1. pointwise
def raw_gauss(mean, std, target, scale, bins, fill=-7.0):
    """rr_gauss_calibration_f64 called directly: the 8 + bins doubles on the host, every entry pre-filled with `fill`"""
    m, s, t = dev(mean), dev(std), dev(target)
    n, nv = len(mean), CR.GAUSS_NSUMS + bins
    ws = torch.empty(((n + U.CAL_BLOCK - 1) // U.CAL_BLOCK) * nv, dtype=torch.float64, device="cuda")
    out = torch.full((nv,), fill, dtype=torch.float64, device="cuda")
    p = _lib.ptr
    _lib.check(_lib.lib().rr_gauss_calibration_f64(p(m), p(s), p(t), n, float(scale), bins, p(ws), ws.numel() * 8, p(out),
                                                   _lib.stream()), "rr_gauss_calibration_f64")
    return out.cpu().numpy()


@pytest.mark.parametrize("invalid", [False, True], ids=["clean", "invalid-rows"])
@pytest.mark.parametrize("scale", GAUSS_SCALES)
@pytest.mark.parametrize("n", GAUSS_SIZES)
def test_gauss_calibration_against_the_restatement(n, scale, invalid, parity_log):
    mean, std, target = CR.gauss_rows(n, n)
    bad = 0
    if invalid:
        mean, std, target, bad = CR.inject_invalid(mean, std, target)
    worst = np.zeros(CR.GAUSS_NSUMS)
    failures = []
    for bins in GAUSS_BINS:
        ref = CR.gauss_calibration(mean, std, target, scale, bins)
        got = raw_gauss(mean, std, target, scale, bins)
        assert np.array_equal(raw_gauss(mean, std, target, scale, bins, fill=3.0), got)      # a second call: the same bits
        assert got[0] == ref["sums"][0] == n - bad and got[1] == ref["sums"][1] == bad     # the counts: exactly
        for k in range(2, CR.GAUSS_NSUMS):
            err, bound = abs(got[k] - ref["sums"][k]), n * EPS * ref["mags"][k]
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
            worst[k] = max(worst[k], ratio)
            Hh.record(f"{CR.SUM_NAMES[k]} / bound", ratio, 1.0)
            if err > bound:
                failures.append((bins, CR.SUM_NAMES[k], got[k], ref["sums"][k], err, bound))
        hist = got[CR.GAUSS_NSUMS:]
        assert hist.sum() == n - bad and np.array_equal(hist, np.round(hist))
        moved = int(np.abs(hist - ref["hist"]).sum())
        assert ref["edge"] <= 1e-3 * n and moved <= 2 * ref["edge"], (bins, moved, ref["edge"])   # no edge rows: exact
    parity_log(f"n {n} scale {scale} {'with' if bad else 'no'} invalid rows: err / (n 2^-52 sum |term|) "
               + ", ".join(f"{CR.SUM_NAMES[k]} {worst[k]:.3f}" for k in range(2, CR.GAUSS_NSUMS)) + "; counts and histogram exact")
    assert not failures, failures


def test_probabilistic_calibration_and_the_fitted_scale(parity_log):
    mean, std, target = CR.gauss_rows(99, 5000, spread=1.5)
    mean, std, target, bad = CR.inject_invalid(mean, std, target)
    got = U.probabilistic_calibration(mean, torch.tensor(target), dev(std), n_bins=20, sigma_scale=1.0)
    ref = CR.gauss_calibration(mean, std, target, 1.0, 20)
    want = CR.probabilistic(ref)
    assert got["n_valid"] == 5000 - bad and got["n_invalid"] == bad and ref["edge"] == 0
    assert np.array_equal(got["pit_hist"], ref["hist"]) and np.array_equal(got["observed"], want["observed"])
    assert got["miscalibration_area"] == want["miscalibration_area"]
    for k in ("nll", "crps", "z_mean", "z2_mean", "sharpness", "rmse"):                # means of sums within the bound above
        assert abs(got[k] - want[k]) <= 5000 * EPS * max(1.0, abs(want[k])) * 4, k
    half = ref["hist"][10 - 3:10 + 3].sum() / (5000 - bad)
    assert list(got["interval_levels"][:3]) == [0.1, 0.2, 0.3] and got["interval_coverage"][2] == half
    assert got["interval_coverage"][-1] == 1.0 and "interval_levels" not in U.probabilistic_calibration(mean, target, std, n_bins=5)
    scale = U.fit_sigma_scale(mean, target, std)
    assert abs(scale - 1.5) <= 3 * 1.5 / np.sqrt(2 * 5000)                            # (the standard error of a std estimate)
    after = U.probabilistic_calibration(mean, target, std, 20, scale)
    assert abs(after["z2_mean"] - 1.0) <= 1e-9 and after["nll"] < got["nll"]
    assert after["miscalibration_area"] < got["miscalibration_area"]
    parity_log(f"spread 1.5: fitted scale {scale:.4f}; miscalibration area {got['miscalibration_area']:.4f} -> "
               f"{after['miscalibration_area']:.4f}, nll {got['nll']:.4f} -> {after['nll']:.4f}")
    with pytest.raises(ValueError):
        U.probabilistic_calibration(mean[:3], target[:3], np.zeros(3, np.float32))   # no valid row
    for kw in (dict(n_bins=0), dict(n_bins=65), dict(sigma_scale=0.0), dict(sigma_scale=float("nan"))):
        with pytest.raises(ValueError):
            U.probabilistic_calibration(mean, target, std, **kw)


# ------------------------------------------------------------------------------------------------ 2. top-1 sets
@functools.lru_cache(maxsize=None)
def case(window, kind):
    """(p, targets, cores) of one window: the inputs and everything of the restatement that does not depend on tau"""
    scope = WINDOWS[window]
    seed = sorted(WINDOWS).index(window) + 10 * KINDS.index(kind)
    p, t = (CR.sample_share_window if kind == "shares" else CR.softmax_window)(seed, scope, ties=True)
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t, CR.window_core(p, scope, t)


def raw_sets(p, scope, targets, tau, fill=-7):
    """rr_top1_sets_f32 called directly: (rank, before, in_set, stats) on the host, every entry pre-filled with `fill`"""
    x = p if torch.is_tensor(p) else dev(p)
    t, seg, Q, M = dev(targets), seg_of(scope), len(scope), int(sum(scope))
    rank = torch.full((max(M, 1),), fill, dtype=torch.int32, device="cuda")
    before = torch.full((max(M, 1),), float(fill), dtype=torch.float64, device="cuda")
    inside = torch.full((max(M, 1),), 7, dtype=torch.uint8, device="cuda")
    stats = torch.full((max(Q, 1), CR.TOP1_NSTATS), float(fill), dtype=torch.float64, device="cuda")
    ptr = _lib.ptr
    _lib.check(_lib.lib().rr_top1_sets_f32(ptr(x), x.stride(0), ptr(t), ptr(seg), Q, max(list(scope) + [0]), float(tau), ptr(rank),
                                           ptr(before), ptr(inside), ptr(stats), _lib.stream()), "rr_top1_sets_f32")
    return rank[:M].cpu().numpy(), before[:M].cpu().numpy(), inside[:M].cpu().numpy(), stats[:Q].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_outputs(a, b):
    """two results of raw_sets, bit for bit (NaNs by their bits too: the same code wrote them)"""
    return all(np.array_equal(x, y) for x, y in zip(a[:1] + a[2:3], b[:1] + b[2:3])) and \
        np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[3]), bits(b[3]))


def compare_sets(got, ref, what):
    rank, before, inside, stats = got
    r_rank, r_before, r_inside, r_stats = ref
    assert np.array_equal(rank, r_rank), what
    assert np.array_equal(bits(before), bits(r_before)), what                          # the ordered sum: bit for bit
    assert np.array_equal(inside.astype(bool), r_inside) and set(np.unique(inside)) <= {0, 1}, what
    live = ~np.isnan(r_stats[:, 0])
    assert np.isnan(stats[~live, :6]).all() and not stats[~live, 6:].any(), what      # an empty list
    assert np.array_equal(stats[live][:, EXACT_STATS], r_stats[live][:, EXACT_STATS]), what
    assert np.array_equal(bits(stats[live][:, BIT_STATS]), bits(r_stats[live][:, BIT_STATS])), what
    assert np.array_equal(stats[live, 7] == 1, stats[live, 5] <= what[-1]), what       # covered <=> E <= tau


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("window", list(WINDOWS))
def test_top1_sets_against_the_restatement(window, kind, parity_log):
    scope = WINDOWS[window]
    p, t, cores = case(window, kind)
    sizes = []
    for tau in TAUS:
        ref = CR.window_sets(p, scope, t, tau, cores)
        got = raw_sets(p, scope, t, tau)
        compare_sets(got, ref, (window, kind, tau))
        sizes.append(got[3][:, 6].sum())
    assert sizes == sorted(sizes) and sizes[-1] == sum(scope)                          # grows with tau; inf: every candidate
    if kind == "shares":
        assert (CR.window_sets(p, scope, t, 0.0, cores)[1] == 0.9375).any()            # tau = 0.9375 sits ON a value of before
    # both forms of the kernel, a second call and the Python entry point: the same bits
    tau = 0.9375
    got = raw_sets(p, scope, t, tau)
    assert same_outputs(raw_sets(p, scope, t, tau, fill=5), got)
    l = _lib.lib()
    try:
        for w in (1, 4):
            assert l.rr_top1_sets_set_waves(w) == 0 and l.rr_top1_sets_waves() == w
            assert same_outputs(raw_sets(p, scope, t, tau), got), w
    finally:
        assert l.rr_top1_sets_set_waves(0) == 0
    via = U.top1_sets(dev(p), scope, torch.tensor(np.array(t)), tau, 0)
    assert via["rank"].dtype == torch.int32 and via["in_set"].dtype == torch.bool and via["stats"].shape == (len(scope), 9)
    assert same_outputs((via["rank"].cpu().numpy(), via["before"].cpu().numpy(), via["in_set"].cpu().numpy().astype(np.uint8),
                         via["stats"].cpu().numpy()), got)
    s = got[3][~np.isnan(got[3][:, 0])]
    parity_log(f"{window} {kind}: rank, in_set, hit, rank of the true top, set size, covered exact and before, confidence, p of the "
               f"true top, Brier, E, mass bit-equal at tau {list(TAUS)}; one wave = four waves = a second call; at tau {tau}: "
               f"coverage {s[:, 7].mean():.3f}, mean set size {s[:, 6].mean():.2f}, worst |mass - 1| {np.abs(s[:, 8] - 1).max():.1e}")


def test_known_answers_on_the_device():
    p, t = [0.25, 0.5, 0.0, 0.25] + [1.0] + [0.5, 0.5], [1, 0, 3, 3] + [2] + [4, 4]
    rank, before, inside, stats = raw_sets(p, [4, 0, 1, 2], t, 0.75)
    assert list(rank) == [2, 1, 4, 3, 1, 1, 2] and list(before) == [0.5, 0.0, 1.0, 0.75, 0.0, 0.0, 0.5]
    assert list(inside) == [1, 1, 0, 1, 1, 1, 1]
    brier = 0.25 ** 2 + 0.5 ** 2 + 1.0 + 0.25 ** 2
    assert list(stats[0]) == [0.0, 0.5, 0.0, 4.0, brier, 1.0, 3.0, 0.0, 1.0]            # the true top: the FIRST maximum, p = 0
    assert np.isnan(stats[1, :6]).all() and list(stats[1, 6:]) == [0, 0, 0]
    assert list(stats[2]) == [1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0]              # a list of one
    assert list(stats[3]) == [1.0, 0.5, 0.5, 1.0, 0.5, 0.0, 2.0, 1.0, 1.0]              # ties in p and in the targets: position


def test_a_strided_probability_column_gives_the_bits_of_the_contiguous_call():
    scope = [5, 64, 65, 300, 2]
    p, t = CR.softmax_window(77, scope, ties=True)
    two = torch.stack([dev(p), dev(p[::-1].copy())], 1)
    assert two[:, 0].stride(0) == 2
    want = raw_sets(p, scope, t, 0.5)
    assert same_outputs(raw_sets(two[:, 0], scope, t, 0.5), want)                      # at the C ABI
    via = U.top1_sets(two[:, 0], scope, torch.tensor(t), 0.5, 0)                                     # and through the Python layer, in place
    assert np.array_equal(bits(via["before"].cpu().numpy()), bits(want[1])) and np.array_equal(bits(via["stats"].cpu().numpy()), bits(want[3]))


def test_status_codes_and_rejected_input():
    fn = _lib.lib().rr_top1_sets_f32
    scope = [4, 4]
    p, t = CR.sample_share_window(3, scope)
    x, tt, seg = dev(p), dev(t), seg_of(scope)
    rank = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    before = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    inside = torch.full((8,), 7, dtype=torch.uint8, device="cuda")
    stats = torch.full((2, 9), -7.0, dtype=torch.float64, device="cuda")
    ptr = _lib.ptr

    def call(tau, max_len=4, Q=2):
        return fn(ptr(x), 1, ptr(tt), ptr(seg), Q, max_len, tau, ptr(rank), ptr(before), ptr(inside), ptr(stats), _lib.stream())

    def untouched():
        torch.cuda.synchronize()
        return bool((rank == -7).all() and (before == -7).all() and (inside == 7).all() and (stats == -7).all())

    for tau in (-1e-300, -1.0, float("nan"), float("-inf")):
        assert call(tau) == -1                                                        # RR_ERR_ARG
    assert call(0.5, max_len=8193) == -4 and untouched()                              # RR_ERR_UNSUPPORTED, nothing launched
    assert call(0.5, Q=0) == 0 and untouched()                                        # RR_OK, nothing launched
    assert call(float("inf")) == 0
    torch.cuda.synchronize()
    assert bool((inside == 1).all()) and stats[:, 6].tolist() == [4.0, 4.0] and stats[:, 7].tolist() == [1.0, 1.0]
    ok = torch.tensor(np.array(t))
    for bad in (np.array([0.5, np.nan, 0.5, 0, 1, 0, 0, 0]), np.array([0.5, -0.25, 0.75, 0, 1, 0, 0, 0])):
        with pytest.raises(ValueError):
            U.top1_sets(dev(bad), scope, ok, 0.5, 0)
    with pytest.raises(ValueError):
        U.top1_sets(x, scope, torch.tensor([0, np.nan, 0, 0, 0, 0, 0, 0.0]), 0.5, 0)
    # a NaN or a negative p at the C ABI changes values and no address: the other list keeps its bits, every rank is in range
    clean = raw_sets(p, scope, t, 0.5)
    q = p.copy()
    q[1], q[2] = np.nan, -0.5
    dirty = raw_sets(q, scope, t, 0.5)
    assert np.array_equal(dirty[0][4:], clean[0][4:]) and np.array_equal(bits(dirty[3][1]), bits(clean[3][1]))
    assert dirty[0][:4].min() >= 1 and dirty[0][:4].max() <= 4


# ------------------------------------------------------------------------------------------------ 3. end to end
TRAIN_SCOPES = [[4, 3, 5], [2, 6, 9, 3], [5, 5, 2, 7, 3], [8, 2, 4]]
CALIB_SCOPES = [[4, 3, 6, 2], [5, 2, 7]]
TEST_SCOPES = [[3, 5, 4], [6, 2, 2, 8]]
HEADS = {"MC_dropout": (dict(task_num=1, ffn_last_layer="with_softplus", task_type=None), "mle", dict(n_samples=8, seed=1)),
         "distribution": (dict(task_num=2, ffn_last_layer="no_softplus", task_type="evidential_ranking"), "evidential_ranking", {})}


@pytest.mark.parametrize("method", list(HEADS))
def test_evaluate_calibration_end_to_end(method, tmp_path, parity_log):
    head, task_type, kw = HEADS[method]
    torch.manual_seed(0)
    model = build_model(hidden_size=32, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.1,
                        add_features_dim=1, **head).cuda()
    opt = TU.build_optimizer(model)
    sch = TU.build_lr_scheduler(opt, warmup_epochs=1.0, total_epochs=2, train_data_size=16, batch_size=4, init_lr=1e-4,
                                max_lr=5e-4, final_lr=1e-4)
    hist = TL.train(model, sch, windows(700, TRAIN_SCOPES), windows(800, CALIB_SCOPES), None, opt, 2, seed=0, gpu=0,
                    task_type=task_type, target_name=None)
    assert len(hist) == 2
    path = str(tmp_path / "model.pt")
    save_checkpoint(path, model)
    calib, test = windows(800, CALIB_SCOPES), windows(900, TEST_SCOPES)
    alpha = 0.25
    res = U.evaluate_calibration(model, calib, test, path, 0, method=method, alpha=alpha, n_bins=20, target_name=None, **kw)
    scope = [c for s in TEST_SCOPES for c in s]
    assert res["scope"] == scope and res["in_set"].shape == res["rank"].shape == (sum(scope),) and res["alpha"] == alpha
    # the threshold from the calibration set's scores, the sets and the coverage from the test set: the restatement's
    cs = res["calibration_set"]
    cal_p, cal_t = cs["p_top1"].cpu().numpy(), cs["targets"].cpu().numpy()
    tau = CR.conformal_threshold(CR.window_sets(cal_p, cs["scope"], cal_t, 0.0)[3][:, 5], alpha)
    assert res["tau"] == tau and cs["scope"] == [c for s in CALIB_SCOPES for c in s]
    p, t = res["p_top1"].cpu().numpy(), res["targets"].cpu().numpy()
    rank, before, inside, stats = CR.window_sets(p, scope, t, tau)
    assert np.array_equal(res["rank"].cpu().numpy(), rank) and np.array_equal(res["in_set"].cpu().numpy(), inside)
    assert res["coverage"] == stats[:, 7].mean() and res["mean_set_size"] == stats[:, 6].mean()
    assert np.array_equal(bits(res["stats"].cpu().numpy()), bits(stats))
    assert abs(res["top1"]["ece"] - CR.ece(stats, 10)) <= 1e-12 and res["top1"]["accuracy"] == stats[:, 0].mean()
    # the sigma scale: fitted on the calibration set, where it makes mean z^2 one; it leaves p_top1 and the sets alone
    assert abs(cs["probabilistic"]["after"]["z2_mean"] - 1.0) <= 1e-9
    assert res["probabilistic"]["after"]["sigma_scale"] == res["sigma_scale"] == cs["probabilistic"]["after"]["sigma_scale"]
    assert res["probabilistic"]["before"]["sigma_scale"] == 1.0
    mean, std = res["mean"].cpu().numpy(), res["std"].cpu().numpy()
    ref = CR.gauss_calibration(mean, std, t, res["sigma_scale"], 20)
    assert ref["edge"] > 0 or np.array_equal(res["probabilistic"]["after"]["pit_hist"], ref["hist"])
    nll = CR.probabilistic(ref)["nll"]
    assert abs(res["probabilistic"]["after"]["nll"] - nll) <= 1e-12 * max(1.0, abs(nll))
    parity_log(f"{method}: sigma scale {res['sigma_scale']:.3f}, tau {tau:.4f}, test coverage {res['coverage']:.3f} at alpha {alpha}, "
               f"mean set size {res['mean_set_size']:.2f} of {np.mean(scope):.2f}, top-1 accuracy {res['top1']['accuracy']:.3f}, "
               f"ECE {res['top1']['ece']:.3f}")
