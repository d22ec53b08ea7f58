"""GPU tests of the per-query rank correlation (csrc/rank_corr.hip, rr_rank_correlation_f32) and of what is built on it: the
eight statistics against the numpy restatement of tests/rank_correlation_ref.py, the bit-level contracts (one wave against
four, repeated calls, strided input), NaN scores, the status codes, shard additivity of eval.rank_correlation_from_scores and
two epochs of both trainers selecting their checkpoint by a rank correlation.

Bounds.  The pair counts P, D, X, Y are integers: EXACTLY the reference's.  tau-b, rho and the reciprocal rank are exact
integers followed by at most four correctly rounded float64 operations (a product, a square root, a quotient; a sum and a
quotient) on magnitudes <= 1: 1e-14 absolute, some fifty half-ulps of 1.  The regret is a difference of two float32 values
formed in float64: exact.  NaNs (a constant key, a list shorter than two, an empty list) sit in the same places."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import rank_correlation_ref as RC
from tests.test_gpu_lambdarank import seg_of, windows

from reactranker_amd import _lib
from reactranker_amd import eval as RE
from reactranker_amd import run_train_pairwise as RT
from reactranker_amd import train_listwise as TL
from reactranker_amd import train_utils as TU
from reactranker_amd.base_model import build_model

pytestmark = pytest.mark.gpu

BOUND = 1e-14
RAGGED = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 300]   # crosses the wave (64) and workgroup (256) boundaries
WINDOWS = {   # seed -> scope
    0: RAGGED,
    1: [64] * 64,                             # the workload's shape
    2: [5, 1, 1, 7, 70],                      # every score 0.5: tau and rho are undefined, the tie rule decides the ranks
    3: [1000],                                # one long list
    4: [8192],                                # the LDS limit
}
CASES = [(seed, ties) for seed in WINDOWS for ties in RC.TIE_LEVELS if seed != 4 or ties == 1]
NAMES = ("tau", "rho", "reciprocal rank")


@functools.lru_cache(maxsize=None)
def case_window(seed, ties):
    score, targets = RC.window(seed, WINDOWS[seed], ties)
    if seed == 2:
        score[:] = 0.5
    score.setflags(write=False)
    targets.setflags(write=False)
    return score, targets


@functools.lru_cache(maxsize=None)
def reference(seed, ties):
    score, targets = case_window(seed, ties)
    ref = RC.window_stats(score, WINDOWS[seed], targets)
    ref.setflags(write=False)
    return ref


def raw_stats(score, scope, targets, fill=float("nan")):
    """rr_rank_correlation_f32 called directly: [Q, 8] float64 on the device, every entry pre-filled with `fill`"""
    s = score if torch.is_tensor(score) else torch.tensor(np.asarray(score, np.float32)).cuda()
    t = torch.tensor(np.asarray(targets, np.float32)).cuda()
    seg, Q = seg_of(scope), len(scope)
    out = torch.full((max(Q, 1), RE.RANK_CORR_NSTATS), fill, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().rr_rank_correlation_f32(_lib.ptr(s), s.stride(0), _lib.ptr(t), _lib.ptr(seg), Q, max(list(scope) + [0]),
                                                  _lib.ptr(out), _lib.stream()), "rr_rank_correlation_f32")
    return out[:Q]


def bits64(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def compare(log, what, got, ref):
    """records and asserts the measures of one window; got: a [Q, 8] device tensor, ref: the restatement's array"""
    got = got.cpu().numpy()
    assert got.shape == ref.shape
    assert np.array_equal(got[:, 4:], ref[:, 4:]), what                               # the pair counts: exactly
    assert np.array_equal(np.isnan(got), np.isnan(ref), equal_nan=True), what         # NaNs in the same places
    errs = []
    for k, name in enumerate(NAMES):
        ok = ~np.isnan(ref[:, k])
        e = float(np.max(np.abs(got[ok, k] - ref[ok, k]))) if ok.any() else 0.0
        Hh.record(f"{what} {name}", e, BOUND)
        errs.append(e)
    ok = ~np.isnan(ref[:, 3])
    regret_equal = bool(np.array_equal(got[ok, 3], ref[ok, 3]))
    log(f"{what}: tau err {errs[0]:.3e}, rho err {errs[1]:.3e}, reciprocal rank err {errs[2]:.3e} abs (bound {BOUND:g}); "
        f"P, D, X, Y exact; regret {'exact' if regret_equal else 'DIFFERS'}; "
        f"{int(np.isnan(ref[:, 0]).sum())} of {len(ref)} queries without a tau")
    assert max(errs) <= BOUND, (what, errs)
    assert regret_equal, what
    return errs


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("seed,ties", CASES)
def test_statistics_against_the_numpy_restatement(seed, ties, parity_log):
    scope = WINDOWS[seed]
    score, targets = case_window(seed, ties)
    ref = reference(seed, ties)
    got = raw_stats(score, scope, targets)
    compare(parity_log, f"seed {seed} ties {ties}", got, ref)
    assert bits64(raw_stats(score, scope, targets, fill=-7.0), got)                   # a second call: the same bits, all written
    via = RE.rank_correlation_stats(torch.tensor(np.array(score)).cuda(), scope, torch.tensor(np.array(targets)), 0)
    assert via.dtype == torch.float64 and bits64(via, got)                            # the Python entry point
    l = _lib.lib()
    forms = {}
    try:                                                                              # both forms of the kernel on every window
        for w in (1, 4):
            assert l.rr_rank_correlation_set_waves(w) == 0 and l.rr_rank_correlation_waves() == w
            forms[w] = raw_stats(score, scope, targets)
    finally:
        assert l.rr_rank_correlation_set_waves(0) == 0
    assert bits64(forms[1], got) and bits64(forms[4], got)
    if seed == 2:
        assert torch.isnan(got[:, :2]).all()                                          # every score tied
        g = got.cpu().numpy()
        assert not g[:, [4, 5, 7]].any() and g[4, 6] > 0                              # no pair is ordered in the score


def test_known_answers_on_the_device():
    s = [1, 2, 3, 4] + [1, 2] + [1, 1, 1] + [0.25]
    t = [1, 2, 2, 5] + [2, 1] + [1, 2, 3] + [7.0]
    got = raw_stats(s, [4, 2, 3, 1, 0], t).cpu().numpy()
    assert abs(got[0, 0] - 0.9128709291752769) <= BOUND and abs(got[0, 1] - 0.9486832980505138) <= BOUND
    assert list(got[0, 2:]) == [1.0, 0.0, 5, 0, 0, 1]
    assert list(got[1]) == [-1.0, -1.0, 0.5, 1.0, 0, 1, 0, 0]
    assert np.isnan(got[2, :2]).all() and abs(got[2, 2] - 1.0 / 3.0) <= BOUND and list(got[2, 3:]) == [2.0, 0, 0, 3, 0]
    assert np.isnan(got[3, :2]).all() and list(got[3, 2:]) == [1.0, 0.0, 0, 0, 0, 0]          # a list of one
    assert np.isnan(got[4, :4]).all() and list(got[4, 4:]) == [0, 0, 0, 0]                    # an empty list


# ------------------------------------------------------------------------------------------------ 2. bits
def test_column_of_a_two_column_output_gives_the_bits_of_the_contiguous_call():
    scope = [5, 64, 65, 300, 2]
    score, targets = RC.window(13, scope, 2)
    out = torch.stack([torch.tensor(score), torch.tensor(score[::-1].copy())], 1).cuda()
    assert out[:, 0].stride(0) == 2
    want = raw_stats(score, scope, targets)
    assert bits64(raw_stats(out[:, 0], scope, targets), want)                         # at the C ABI
    tt = torch.tensor(targets)
    assert bits64(RE.rank_correlation_stats(out, scope, tt, 0), want)                 # [M, 2]: the first column, read in place
    assert same_dict(RE.rank_correlation_from_scores(out, scope, tt, 0), RE.rank_correlation_from_scores(out[:, 0].contiguous(), scope, tt, 0))


def test_nan_scores_are_tied_with_everything_and_touch_no_other_list(parity_log):
    scope = [7, 65, 70]
    score, targets = RC.window(21, scope, 1)
    clean = raw_stats(score, scope, targets)
    score = score.copy()
    score[7 + np.array([0, 13, 63, 64])] = np.nan                                     # first, inside, and both sides of the wave edge
    ref = RC.window_stats(score, scope, targets)
    got = raw_stats(score, scope, targets)
    compare(parity_log, "NaN scores in a list of 65", got, ref)
    assert bits64(got[0], clean[0]) and bits64(got[2], clean[2])                      # the lists before and after
    g = got.cpu().numpy()
    assert g[1, 6] > float(clean[1, 6]) and not np.isnan(g[1, :4]).any()             # more pairs tied in the score only
    score[7:7 + 65] = np.nan                                                          # a list of NaNs only: a constant key
    got = raw_stats(score, scope, targets).cpu().numpy()
    ref = RC.window_stats(score, scope, targets)
    assert np.isnan(got[1, :2]).all() and np.array_equal(got, ref, equal_nan=True)


def test_status_codes():
    fn = _lib.lib().rr_rank_correlation_f32
    score, targets = RC.window(3, [4, 4])
    s, t, seg = torch.tensor(score).cuda(), torch.tensor(targets).cuda(), seg_of([4, 4])
    out = torch.full((2, 8), -7.0, dtype=torch.float64, device="cuda")
    p = _lib.ptr
    assert fn(p(s), 1, p(t), p(seg), 2, 8193, p(out), _lib.stream()) == -4            # RR_ERR_UNSUPPORTED, nothing launched
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, -7.0))
    for args in ((None, 1, p(t), p(seg)), (p(s), 1, None, p(seg)), (p(s), 1, p(t), None), (p(s), 0, p(t), p(seg))):
        assert fn(*args, 2, 4, p(out), _lib.stream()) == -1                           # RR_ERR_ARG: null pointers, stride 0
    assert fn(p(s), 1, p(t), p(seg), 2, 4, None, _lib.stream()) == -1
    assert fn(p(s), 1, p(t), p(seg), -1, 4, p(out), _lib.stream()) == -1
    assert fn(p(s), 1, p(t), p(seg), 0, 4, p(out), _lib.stream()) == 0                # RR_OK, nothing launched
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, -7.0))
    assert fn(p(s), 1, p(t), p(seg), 2, 4, p(out), _lib.stream()) == 0
    ref = RC.window_stats(score, [4, 4], targets)
    assert np.array_equal(out.cpu().numpy()[:, 3:], ref[:, 3:]) and np.max(np.abs(out.cpu().numpy() - ref)) <= BOUND


# ------------------------------------------------------------------------------------------------ 3. the Python layer
def same_dict(a, b):
    def eq(x, y):
        return x == y or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))
    return a.keys() == b.keys() and all(eq(a[k], b[k]) for k in a)


def test_from_scores_matches_the_restatement_and_shards_add_up():
    scope = [3, 70, 1, 2, 9, 0, 130, 4]
    score, targets = RC.window(15, scope)
    targets[3 + 70 + 1:3 + 70 + 1 + 2] = 0.5                                          # query 3: a constant key, as is query 2
    s, tt = torch.tensor(score).cuda(), torch.tensor(targets)
    whole = RE.rank_correlation_from_scores(s, scope, tt, 0)
    ref = RC.summary(*RC.nanmean_stats(RC.window_stats(score, scope, targets)))
    assert whole["pairs"] == ref["pairs"] and whole["n_defined"] == ref["n_defined"] == 5
    assert whole["kendall_tau_pooled"] == ref["kendall_tau_pooled"]
    for k in ("kendall_tau", "spearman", "mrr", "regret"):
        assert abs(whole[k] - ref[k]) <= BOUND, k
    # the data-parallel contract without a process group: each shard's sums and counts, added by hand
    lo = sum(scope[:3])
    a = RE._nanmean_stats(RE.rank_correlation_stats(s[:lo], scope[:3], tt[:lo], 0))
    b = RE._nanmean_stats(RE.rank_correlation_stats(s[lo:], scope[3:], tt[lo:], 0))
    both = RE._rank_correlation_dict(a[0] + b[0], a[1] + b[1])
    assert both["pairs"] == whole["pairs"] and both["n_defined"] == whole["n_defined"]
    assert both["kendall_tau_pooled"] == whole["kendall_tau_pooled"]
    for k in ("kendall_tau", "spearman", "mrr", "regret"):                            # (two float64 sums added in another order)
        assert abs(both[k] - whole[k]) <= BOUND, k
    none = RE.rank_correlation_from_scores(s[:1], [1, 0], tt[:1], 0)                  # no tau defined: NaN means, no error
    assert math.isnan(none["kendall_tau"]) and math.isnan(none["spearman"]) and math.isnan(none["kendall_tau_pooled"])
    assert none["mrr"] == 1.0 and none["regret"] == 0.0 and none["n_defined"] == 0 and none["pairs"] == [0.0] * 4


def small_model():
    torch.manual_seed(0)
    model = build_model(task_num=1, ffn_last_layer="no_softplus", add_features_dim=1, hidden_size=32, mpnn_depth=2,
                        mpnn_diff_depth=2, ffn_depth=2, use_bias=True, dropout=0.0).cuda()
    opt = TU.build_optimizer(model)
    sch = TU.build_lr_scheduler(opt, warmup_epochs=1.0, total_epochs=2, train_data_size=16, batch_size=4, init_lr=1e-4,
                                max_lr=5e-4, final_lr=1e-4)
    return model, opt, sch


TRAIN_SCOPES = [[4, 3, 5], [2, 6, 9, 3], [5, 5, 2, 7, 3], [8, 2, 4]]
VAL_SCOPES = [[4, 3], [5, 2]]


@pytest.mark.parametrize("trainer,metric", [("listwise", "kendall_tau"), ("pairwise", "spearman")])
def test_two_epochs_selecting_the_checkpoint_by_a_rank_correlation(trainer, metric, tmp_path):
    import os
    model, opt, sch = small_model()
    train_w, val_w = windows(500, TRAIN_SCOPES), windows(600, VAL_SCOPES)
    val = [(b["r"], b["p"], b["scope"], b["targets"], b.get("add")) for b in val_w]
    seen = []

    def hook(epoch, m, rec):
        was = m.training
        seen.append((rec.get("rank_correlation"), RE.rank_correlation(m, 0, val), rec["checkpoint"]))
        assert m.training == was                                                      # the caller's mode is restored

    path = str(tmp_path / "ck" / "model.pt")
    if trainer == "listwise":
        hist = TL.train(model, sch, train_w, val_w, path, opt, 2, seed=0, gpu=0, task_type="mle", save_metric=metric,
                        target_name=None, epoch_hook=hook)
    else:
        hist = RT.run_train(model, sch, train_w, val_w, path, opt, 2, 0, 0, train_strategy="sum_session", task_type="baseline",
                            target_name=None, save_metric=metric, epoch_hook=hook)
    assert len(hist) == len(seen) == 2
    for h, (recorded, again, _) in zip(hist, seen):
        assert "rank_correlation" in h and same_dict(h["rank_correlation"], recorded) and same_dict(recorded, again)
        assert -1.0 <= h["rank_correlation"][metric] <= 1.0 and 1 <= h["rank_correlation"]["n_defined"] <= 4
    assert hist[0]["checkpoint"] and os.path.exists(path)                             # any defined value beats -inf
    best = hist[0]["rank_correlation"][metric]
    assert hist[1]["checkpoint"] == (hist[1]["rank_correlation"][metric] >= best)


def test_other_save_metrics_record_no_rank_correlation():
    model, opt, sch = small_model()
    hist = TL.train(model, sch, windows(500, TRAIN_SCOPES), windows(600, VAL_SCOPES), None, opt, 1, seed=0, gpu=0, task_type="mle",
                    save_metric="all", target_name=None)
    assert len(hist) == 1 and "rank_correlation" not in hist[0]
    model, opt, sch = small_model()
    hist = RT.run_train(model, sch, windows(500, TRAIN_SCOPES), windows(600, VAL_SCOPES), None, opt, 1, 0, 0,
                        train_strategy="sum_session", task_type="baseline", target_name=None, save_metric="all")
    assert len(hist) == 1 and "rank_correlation" not in hist[0]
    assert set(hist[0]) == {"epoch", "train_loss", "top1", "pred_top25_in_targ_top25", "top1_in_pred_top25", "checkpoint",
                            "checkpoint_all"}
