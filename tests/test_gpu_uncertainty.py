"""MC-dropout / ensemble uncertainty on the GPU (reactranker_amd.uncertainty): rr_mc_sample_stats_f32 and
rr_uq_calibration_f64 against the numpy restatements of tests/test_uq_cpu.py (the Spearman one pinned to scipy there and
here), the MC samples against explicit train-mode forwards with the same dropout seeds, the ensemble against stacked
eval-mode forwards, and evaluate_uncertainty end to end on a saved checkpoint."""
import math

import numpy as np
import pytest
import torch

from reactranker_amd import eval as E
from reactranker_amd import featurization, synth
from reactranker_amd import uncertainty as U
from reactranker_amd.base_model import build_model
from reactranker_amd.utils import save_checkpoint
from oracle import ref_cpu as O
from tests.test_uq_cpu import curve_ref, spearman_ref, stats_ref

pytestmark = pytest.mark.gpu

CFG = dict(hidden_size=64, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, task_num=1,
           ffn_last_layer="with_softplus", add_features_dim=1)
SCOPE = [0, 1, 2, 63, 64, 65, 300, 8192]


def _quantised(rng, shape, step=0.25):
    """Scores on a coarse grid (many ties); + 0.0 turns the -0.0 of rounding into 0.0."""
    return (np.round(rng.standard_normal(shape) / step) * step + 0.0).astype(np.float32)


def _model(dropout, wseed):
    shapes = O.model_shapes(64, 3, 3, 3, 1, 1, True)
    m = build_model(dropout=dropout, **CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in synth.seeded_weights(shapes, wseed).items()})
    return m.cuda()


def _batch(seed, nq=16):
    rng = np.random.default_rng(seed)
    scope = [int(c) for c in rng.integers(3, 13, nq)]
    qb = synth.make_queries(seed, nq, scope, atoms_lo=5, atoms_hi=12)
    return (featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs), qb.scope,
            torch.tensor(qb.targets), qb.add_features)


def _forward(model, b, train, seed=None):
    was = model.training
    model.train(train)
    model.dropout_seed = seed
    with torch.no_grad():
        out = model(b[0], b[1], gpu=0, add_features=b[4])
    model.train(was)
    model.dropout_seed = None
    return out[:, 0] if out.dim() > 1 else out


def _check_stats(got, want, parity_log=None, what=""):
    for k in ("mean", "std"):
        g, w = got[k].cpu().numpy().astype(np.float64), want[k].astype(np.float64)
        err = float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-30))) if len(w) else 0.0
        if parity_log is not None:
            parity_log(f"{what} {k}: max rel err {err:.3e}")
        assert err <= 1e-12, (what, k, err)
    for k in ("p_top1", "mean_rank"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), (what, k)
    q = got["qstats"].cpu().numpy()
    qerr = float(np.max(np.abs(q - want["qstats"]) / np.maximum(1.0, np.abs(want["qstats"])))) if q.size else 0.0
    if parity_log is not None:
        parity_log(f"{what} qstats: max err {qerr:.3e}")
    assert q.shape == want["qstats"].shape and qerr <= 1e-12, (what, qerr)


@pytest.mark.parametrize("T", [2, 7, 64])
def test_sample_stats_kernel_against_numpy(T, parity_log):
    rng = np.random.default_rng(100 + T)
    M = sum(SCOPE)
    s = _quantised(rng, (T, M))
    tg = _quantised(rng, M, 0.5)
    dev = torch.device("cuda", 0)
    x, t = torch.from_numpy(s).to(dev), torch.from_numpy(tg).to(dev)
    got = U.sample_stats(x, SCOPE, t, 0)
    _check_stats(got, stats_ref(s, SCOPE, tg), parity_log, f"T={T}")
    again = U.sample_stats(x, SCOPE, t, 0)
    for k in ("mean", "std", "p_top1", "mean_rank", "qstats"):
        assert torch.equal(got[k], again[k]), k
    assert torch.all(got["qstats"][0] == 0)                       # the empty list
    # a strided view of a wider buffer is read in place
    wide = torch.zeros(T, M + 37, device=dev)
    wide[:, :M] = x
    v = U.sample_stats(wide[:, :M], SCOPE, t, 0)
    assert torch.equal(v["mean"], got["mean"]) and torch.equal(v["qstats"], got["qstats"])


def test_sample_stats_status_codes():
    dev = torch.device("cuda", 0)
    with pytest.raises(RuntimeError, match="size outside"):
        U.sample_stats(torch.zeros(3, 8193, device=dev), [8193], torch.zeros(8193, device=dev), 0)
    with pytest.raises(RuntimeError, match="invalid argument"):
        U.sample_stats(torch.zeros(1, 10, device=dev), [4, 6], torch.zeros(10, device=dev), 0)
    torch.cuda.synchronize()


def test_mc_samples_match_explicit_forwards():
    model = _model(0.1, 11)
    model.train(False)
    model.dropout_seed = 1234
    b = _batch(21)
    rng_before = torch.get_rng_state()
    res = U.mc_dropout_predict(model, [b], 6, seed=9, gpu=0)
    assert torch.equal(torch.get_rng_state(), rng_before)
    assert model.training is False and model.dropout_seed == 1234
    assert len(res) == 1
    r = res[0]
    assert r["samples"].shape == (6, sum(b[2]))
    for t in range(6):
        assert torch.equal(r["samples"][t], _forward(model, b, True, U.sample_seed(9, t))), t
    assert not torch.equal(r["samples"][0], r["samples"][1])        # dropout 0.1 does move the scores
    _check_stats(r, stats_ref(r["samples"].cpu().numpy(), b[2], b[3].numpy()))
    assert torch.equal(torch.get_rng_state(), rng_before)


def _check_degenerate(r, eval_scores, scope):
    assert torch.all(r["std"] == 0)
    assert torch.equal(r["mean"], eval_scores)
    p, s, off = r["p_top1"].cpu().numpy(), eval_scores.cpu().numpy(), 0
    for c in scope:
        want = np.zeros(c, np.float32)
        want[int(np.argmax(s[off:off + c]))] = 1.0
        assert np.array_equal(p[off:off + c], want)
        off += c
    assert torch.all(r["qstats"][:, 0] == 0)
    assert torch.all(r["qstats"][:, 3] == 0)


def test_dropout_zero_and_a_repeated_checkpoint_have_no_spread(tmp_path):
    model = _model(0.0, 12)
    b = _batch(22)
    ev = _forward(model, b, False)
    r = U.mc_dropout_predict(model, [b], 3, seed=0, gpu=0)[0]
    _check_degenerate(r, ev, b[2])
    path = str(tmp_path / "0.pt")
    save_checkpoint(path, model)
    other = _model(0.0, 99)                                       # its own weights are replaced by the checkpoint's
    other.train(True)
    r = U.ensemble_predict(other, [path] * 3, [b], gpu=0)[0]
    assert other.training is True
    _check_degenerate(r, ev, b[2])


def test_ensemble_of_three_models_matches_stacked_forwards(tmp_path, parity_log):
    b1, b2 = _batch(23), _batch(24, nq=5)
    paths, cols = [], [[], []]
    for i, ws in enumerate((31, 32, 33)):
        m = _model(0.1, ws)
        paths.append(str(tmp_path / f"{i}.pt"))
        save_checkpoint(paths[-1], m)
        cols[0].append(_forward(m, b1, False))
        cols[1].append(_forward(m, b2, False))
    res = U.ensemble_predict(_model(0.1, 1), paths, [b1, b2], gpu=0)
    for r, c, b in zip(res, cols, (b1, b2)):
        stacked = torch.stack(c)
        assert torch.equal(r["samples"], stacked)
        _check_stats(r, stats_ref(stacked.cpu().numpy(), b[2], b[3].numpy()), parity_log, "ensemble")


def _calibration_case(rng, n, kind):
    pred = _quantised(rng, n, 0.5)
    target = np.zeros(n, np.float32) if kind != "plain" else rng.standard_normal(n).astype(np.float32)
    if kind == "constant":
        unc = np.full(n, 0.25, np.float32)
    else:
        unc = (np.round(np.abs(pred) * 2 + rng.random(n) * 3) * 0.5).astype(np.float32)    # correlated, with ties
    return pred, target, unc


@pytest.mark.parametrize("n", [2, 1000, 1_000_003])
@pytest.mark.parametrize("kind", ["ties", "constant", "plain"])
def test_calibration_against_numpy_and_scipy(n, kind, parity_log):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(n + len(kind))
    pred, target, unc = _calibration_case(rng, n, kind)
    fr = U.DEFAULT_FRACTIONS + (0.999,)
    dev = torch.device("cuda", 0)
    args = [torch.from_numpy(a).to(dev) for a in (pred, target, unc)]
    got = U.uncertainty_calibration(*args, fractions=fr)
    err = np.abs(pred - target)                                    # float32, as the library forms it
    want_rho = spearman_ref(err, unc)
    if kind == "constant":
        assert math.isnan(want_rho)
    if math.isnan(want_rho):                                       # a constant error or uncertainty
        assert math.isnan(got["spearman"])
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sp = stats.spearmanr(err, unc).statistic
        assert abs(got["spearman"] - want_rho) <= 1e-9 and abs(got["spearman"] - sp) <= 1e-9, (got["spearman"], want_rho, sp)
        parity_log(f"n={n} {kind}: |rho - scipy| {abs(got['spearman'] - sp):.3e}")
    kept, mae, rmse = curve_ref(err, unc, fr)
    assert np.array_equal(got["kept"], kept)
    assert np.array_equal(got["fractions"], np.asarray(fr))
    for name, g, w in (("mae", got["mae"], mae), ("rmse", got["rmse"], rmse)):
        rel = float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300)))
        parity_log(f"n={n} {kind}: {name} max rel err {rel:.3e}")
        assert rel <= 1e-9, (name, rel)
    again = U.uncertainty_calibration(*args, fractions=fr)
    for k in ("kept", "mae", "rmse"):
        assert got[k].tobytes() == again[k].tobytes(), k
    assert np.float64(got["spearman"]).tobytes() == np.float64(again["spearman"]).tobytes()


def test_calibration_moves_host_tensors_to_the_gpu():
    pred = torch.tensor([0.0, 1.0, 2.0, 3.0])
    out = U.uncertainty_calibration(pred, torch.zeros(4), pred * 2, fractions=(0.0, 0.5))
    assert out["spearman"] == 1.0
    assert out["kept"].tolist() == [4, 2] and out["mae"].tolist() == [1.5, 0.5]


def test_evaluate_uncertainty_on_a_saved_checkpoint(tmp_path):
    model = _model(0.1, 41)
    path = str(tmp_path / "ck" / "0.pt")
    mean, std = 1.7, 0.6
    save_checkpoint(path, model, mean, std)
    bs = [_batch(51), _batch(52, nq=4)]
    test_b = [dict(r=b[0], p=b[1], scope=b[2], targets=b[3], add=b[4]) for b in bs]
    res = U.evaluate_uncertainty(_model(0.1, 7), test_b, path, 0, method="MC_dropout", n_samples=5, seed=3)
    scope = [c for b in bs for c in b[2]]
    assert res["scope"] == scope
    want_t = np.concatenate([(-(b[3].double().numpy() - mean) / std).astype(np.float32) for b in bs])   # 'ea': sign flipped
    assert np.array_equal(res["targets"].cpu().numpy(), want_t)
    assert res["top_scores"] == E.top_scores_from_scores(res["mean"], scope, res["targets"], 0, 0.25)
    # the same numbers as mc_dropout_predict on the standardised batches
    m2 = _model(0.1, 41)
    direct = U.mc_dropout_predict(m2, [(b[0], b[1], b[2], torch.from_numpy(want_t[o:o + len(b[3])]), b[4])
                                       for b, o in zip(bs, (0, len(bs[0][3])))], 5, seed=3, gpu=0)
    assert torch.equal(res["mean"], torch.cat([d["mean"] for d in direct]))
    assert torch.equal(res["std"], torch.cat([d["std"] for d in direct]))
    q = torch.cat([d["qstats"] for d in direct]).mean(dim=0).cpu().numpy()
    assert np.array_equal(res["qstats"], q)
    cal = U.uncertainty_calibration(res["mean"], res["targets"], res["std"])
    assert res["calibration"]["spearman"] == cal["spearman"] or (math.isnan(cal["spearman"])
                                                                and math.isnan(res["calibration"]["spearman"]))
    assert np.array_equal(res["calibration"]["mae"], cal["mae"])
    # the ensemble path over three checkpoints with the same scaler
    paths = []
    for i in range(3):
        paths.append(str(tmp_path / f"e{i}.pt"))
        save_checkpoint(paths[-1], _model(0.1, 60 + i), mean, std)
    ens = U.evaluate_uncertainty(_model(0.1, 7), test_b, paths, 0, method="ensemble")
    assert ens["top_scores"] == E.top_scores_from_scores(ens["mean"], scope, ens["targets"], 0, 0.25)
    assert torch.all(ens["std"] > 0)
