"""GPU parity of the pairwise trainer's remaining strategies: the two C x C losses (BetaNet, BetaNet_envidential) against a
float64 evaluation of the reference's formula, no worse than the reference's own float32 result; pairwise_acc /
eval_cross_entropy_loss and the baseline pair model against vectors produced by the reference itself
(tests/golden/pairwise_variants.npz, written by tools/make_golden_pairwise_variants.py); the three new training loops.

Why float64 is the yardstick for the two losses: BetaNet cancels lgamma values near 360 (alpha0 = 100), and the reference's
own float32 evaluation sits up to a few 1e-5 (relative to 1 + |value|) from a float64 evaluation of the same formula.  For
every case, with dist(x) = max |x - f64| / (1 + |f64|) over the loss and EVERY gradient element, the kernel must satisfy
dist(kernel) <= max(1e-5, dist(reference golden)): no worse than the reference, with no margin on top."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import pairwise_variants_ref as R

from reactranker_amd import eval as RE
from reactranker_amd import featurization, pairs, ranknet_baseline, synth
from reactranker_amd import loss as RL
from reactranker_amd import run_train_pairwise as RT
from reactranker_amd import train_pairwise as TP
from reactranker_amd import train_utils as TU
from reactranker_amd.base_model import build_model
from reactranker_amd.utils import load_checkpoint

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQ_CASES = ["c1_c2", "c2_c5", "c64", "c64_s3", "c300", "c300_s3", "c2000", "tied"]


def _parity_file():
    """$RR_PAIRWISE_PARITY, or pairwise_variants_parity.txt next to the parity log tests/conftest.py keeps."""
    from tests.conftest import _parity_path
    return os.environ.get("RR_PAIRWISE_PARITY", os.path.join(os.path.dirname(_parity_path()), "pairwise_variants_parity.txt"))


@pytest.fixture(scope="module")
def V(golden_dir):
    return np.load(os.path.join(golden_dir, "pairwise_variants.npz"))


def dist(x, f64):
    x = x.detach().cpu().double().numpy().reshape(-1) if torch.is_tensor(x) else np.asarray(x, np.float64).reshape(-1)
    f64 = f64.detach().cpu().double().numpy().reshape(-1) if torch.is_tensor(f64) else np.asarray(f64, np.float64).reshape(-1)
    assert x.shape == f64.shape, (x.shape, f64.shape)
    assert np.isfinite(x).all()
    return float(np.max(np.abs(x - f64) / (1 + np.abs(f64)))) if x.size else 0.0


def close(got, ref, tol=1e-5, what=""):
    err = dist(got, ref)
    Hh.record(what, err, tol)
    assert err <= tol, f"{what}: err {err:.3e} > {tol}"


def leaf(a):
    return torch.tensor(np.asarray(a, np.float32)).cuda().requires_grad_(True)


def sq_params(V):
    mc, ep, eps = V["evi_args"].tolist()
    return {"betanet": float(V["alpha0"]), "beta_evidential": mc * (ep / (eps - 1)) ** 3}


def sq_call(key, x, scope, t, param):
    if key == "betanet":
        return RL.betanet_loss(x, scope, t, param, 0)
    return RL.beta_evidential_loss(x, scope, t, param, 0)


def _note(line):
    path = _parity_file()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


@pytest.mark.parametrize("name", SQ_CASES)
def test_sq_losses_no_worse_than_the_reference_against_float64(name, V, parity_log):
    P = f"sq.{name}."
    scope, t = V[P + "scope"].tolist(), V[P + "targets"]
    for key, xkey in (("betanet", "score"), ("beta_evidential", "pos")):
        param = sq_params(V)[key]
        f_loss, npairs, f_g = R.sq_loss(key, V[P + xkey], scope, t, param)
        f_loss, f_g = f_loss / npairs, f_g / npairs                       # what one step of the reference's loop forms
        x = leaf(V[P + xkey])
        loss_sum, pairs_dev = sq_call(key, x, scope, torch.tensor(t), param)
        assert loss_sum.shape == () and int(pairs_dev) == npairs
        loss = loss_sum / npairs
        RL.backward(loss)
        d_ref = max(dist(V[P + key], f_loss), dist(V[P + key + "_g"], f_g))
        d_loss, d_grad = dist(loss, f_loss), dist(x.grad, f_g)
        bound = max(1e-5, d_ref)
        line = (f"{key} {name} scope={scope}: kernel vs f64 loss {d_loss:.3e} grad {d_grad:.3e} | reference float32 vs f64 "
                f"loss {dist(V[P + key], f_loss):.3e} grad {dist(V[P + key + '_g'], f_g):.3e} | bound {bound:.3e}")
        parity_log(line)
        _note(line)
        Hh.record(f"{key} loss vs f64", d_loss, bound)
        Hh.record(f"{key} grad vs f64", d_grad, bound)
        assert d_loss <= bound and d_grad <= bound, line
        # two runs give the same bits
        x2 = leaf(V[P + xkey])
        l2, _ = sq_call(key, x2, scope, torch.tensor(t), param)
        RL.backward(l2 / npairs)
        assert torch.equal(l2, loss_sum) and torch.equal(x2.grad, x.grad)


def test_sq_losses_ragged_window_strided_view_and_empty_query(V, parity_log):
    """One window of ragged queries including C = 1, C = 2, an EMPTY query, C = 64 and C = 300, scored through column 0 of a
    strided [M, 2] view: against float64 at 1e-5 * (1 + |f64|) (the reference has no multi-query window to compare with)."""
    rng = np.random.default_rng(5)
    scope = [1, 2, 0, 64, 7, 300, 33]
    m = sum(scope)
    t = rng.standard_normal(m).astype(np.float32)
    t[70:74] = t[70]                                                       # tied targets
    for key, col, param in (("betanet", (rng.standard_normal(m) * 1.5).astype(np.float32), 100.0),
                            ("beta_evidential", (np.log1p(np.exp(rng.standard_normal(m))) + 1).astype(np.float32), 0.004)):
        f_loss, npairs, f_g = R.sq_loss(key, col, scope, t, param)
        two = torch.zeros(m, 2)
        two[:, 0] = torch.tensor(col)
        two[:, 1] = 123.0
        x = two.cuda().requires_grad_(True)
        loss_sum, pairs_dev = sq_call(key, x, scope, torch.tensor(t), param)
        assert int(pairs_dev) == npairs == RL.sq_pairs(scope)
        (loss_sum / npairs).backward()
        close(loss_sum / npairs, f_loss / npairs, what=key + " window loss")
        close(x.grad[:, 0], f_g / npairs, what=key + " window grad")
        assert float(x.grad[:, 1].abs().max()) == 0.0
        y = leaf(col)
        l2, _ = sq_call(key, y, scope, torch.tensor(t), param)
        (l2 / npairs).backward()
        assert torch.equal(l2, loss_sum) and torch.equal(y.grad, x.grad[:, 0])
    # a too-long list
    big = torch.zeros(8193).cuda()
    for fn in (lambda: RL.betanet_loss(big, [8193], torch.zeros(8193)), lambda: RL.beta_evidential_loss(big + 1, [8193], torch.zeros(8193), 0.1)):
        with pytest.raises(RuntimeError, match="unsupported|range"):
            fn()
    with pytest.raises(RuntimeError, match="unsupported|range"):            # the same error as the other loss entries
        RL.ranknet_loss(big, [8193], torch.zeros(8193))


def test_pairwise_eval_kernel_against_the_reference(V):
    scope, t, s = V["eval.scope"].tolist(), V["eval.targets"], V["eval.scores"]
    sums, per_query = RE.pairwise_stats_from_scores(torch.tensor(s).cuda(), scope, torch.tensor(t), float(V["eval.sigma"]))
    sums = sums.cpu().numpy()
    acc, ce = sums[0] / sums[1], sums[2] / sums[3]
    assert abs(acc - float(V["eval.pairwise_acc"])) <= 1e-6
    close(ce, V["eval.cross_entropy"], what="eval_cross_entropy_loss")
    assert (per_query[:, 0].cpu().numpy() > 0).tolist() == V["eval.used"].tolist()       # pair-less queries are skipped
    assert int(sums[1]) == int(V["eval.used"].sum()) < len(scope)
    _, _, rows = R.pairwise_stats(s, scope, t, float(V["eval.sigma"]))
    assert np.array_equal(per_query[:, :2].cpu().numpy(), rows[:, :2])                   # counts are exact
    # [M, 2] outputs: first column; run to run the same bits
    two = torch.stack([torch.tensor(s), torch.zeros(len(s))], dim=1).cuda()
    sums2, pq2 = RE.pairwise_stats_from_scores(two, scope, torch.tensor(t), float(V["eval.sigma"]))
    assert torch.equal(sums2.cpu(), torch.tensor(sums)) and torch.equal(pq2, per_query)

    class Preset(torch.nn.Module):
        def forward(self, r, p, gpu=None, add_features=None):
            return r
    off, batches = 0, []
    for lo, hi in ((0, 3), (3, len(scope))):                                             # two batches of whole queries
        n = sum(scope[lo:hi])
        batches.append((torch.tensor(s[off:off + n]).cuda(), None, scope[lo:hi], torch.tensor(t[off:off + n]), None))
        off += n
    assert abs(RE.pairwise_acc(Preset(), 0, batches) - float(V["eval.pairwise_acc"])) <= 1e-6
    close(RE.eval_cross_entropy_loss(Preset(), 0, batches, sigma=float(V["eval.sigma"])), V["eval.cross_entropy"],
          what="eval_cross_entropy_loss over batches")


def test_pairwise_eval_kernel_1e5_candidates_against_numpy():
    rng = np.random.default_rng(11)
    scope = [50] * 2000
    t = (np.round(rng.standard_normal(10 ** 5) * 4) / 4).astype(np.float32)
    s = (np.round(rng.standard_normal(10 ** 5) * 16) / 16).astype(np.float32)
    sums, _ = RE.pairwise_stats_from_scores(torch.tensor(s).cuda(), scope, torch.tensor(t), 0.7)
    sums = sums.cpu().numpy()
    acc, ce, rows = R.pairwise_stats(s, scope, t, 0.7)
    assert abs(sums[0] / sums[1] - acc) <= 1e-6
    close(sums[2] / sums[3], ce, what="cross entropy, 1e5 candidates")
    assert sums[3] == 2 * rows[:, 0].sum()


def test_pair_loss_and_accuracy_kernels(V):
    off = 0
    accs = []
    for b in V["pairacc.sizes"].tolist():
        y, t = V["pairacc.y"][off:off + b], V["pairacc.t"][off:off + b]
        accs.append(float(RE.pair_acc_from_outputs(torch.tensor(y).cuda(), t)))
        f_loss, f_g = R.pair_softmax_mse(y, t)
        x = leaf(y)
        l = RL.pair_softmax_mse(x, t)
        assert l.shape == ()
        RL.backward(l)
        close(l, f_loss, what="pair_softmax_mse")
        close(x.grad, f_g, what="pair_softmax_mse grad")
        # a strided [B, 4] view
        wide = torch.zeros(b, 4).cuda()
        wide[:, :2] = torch.tensor(y).cuda()
        xv = wide.requires_grad_(True)
        lv = RL.pair_softmax_mse(xv[:, :2], t)
        lv.backward()
        assert torch.equal(lv, l) and torch.equal(xv.grad[:, :2], x.grad)
        off += b
    assert abs(np.mean(accs) - float(V["pairacc.acc"])) <= 1e-6


def pair_case(V, dropout=0.0):
    hidden, d, dd, fd, tn, seed, wseed, B = V["pair.cfg"].tolist()
    model = ranknet_baseline.build_model(hidden_size=hidden, mpnn_depth=d, mpnn_diff_depth=dd, ffn_depth=fd, use_bias=True,
                                         dropout=dropout, task_num=tn, ffn_last_layer="evidential")
    w = {k[len("pair.w."):]: V[k] for k in V.files if k.startswith("pair.w.")}
    missing = model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    assert not missing.missing_keys and not missing.unexpected_keys
    scope = V["pair.scope"].tolist()
    qb = synth.make_queries(seed, len(scope), scope, atoms_lo=5, atoms_hi=10)
    batches = list(pairs.pair_windows(qb.r_specs, qb.p_specs, scope, V["pair.targets"], B))
    return model.cuda(), batches, B


def test_pair_model_against_reference_vectors(V):
    """Outputs and every parameter gradient against the reference's ranknet_baseline model, at the tolerances
    tests/test_gpu_model.py uses for the model_* fixtures (scores / loss 1e-5 * (1 + |ref|), gradients 5e-5 of the tensor's
    max-abs + 1e-6), in the library's default arithmetic."""
    model, batches, B = pair_case(V)
    model.eval()
    model.dedup_molecules = False
    with torch.no_grad():
        out = torch.cat([model(b["r"], b["p1"], b["p2"], gpu=0) for b in batches])
    assert tuple(out.shape) == tuple(V["pair.out_eval"].shape)
    close(out, V["pair.out_eval"], what="pair model out (eval, three passes)")
    # train mode, dropout 0: one step of the baseline loop's loss on the whole batch
    model.train()
    model.zero_grad()
    b = batches[0]
    y = model(b["r"], b["p1"], b["p2"], gpu=0)
    close(y, V["pair.out_eval"][:B], what="pair model out (train, p = 0)")
    loss = RL.pair_softmax_mse(y, b["targets"])
    close(loss, V["pair.loss"], what="pair loss")
    RL.backward(loss)
    seen = 0
    for k, p in model.named_parameters():
        key = "pair.g." + k
        if key not in V.files:
            continue
        seen += 1
        ref = V[key]
        g = torch.zeros_like(p) if p.grad is None else p.grad
        err = float(np.max(np.abs(g.detach().cpu().numpy().astype(np.float64) - ref)))
        bound = 5e-5 * float(np.abs(ref).max()) + 1e-6
        Hh.record("pair model grad (worst tensor, |err| / (max|g| + 2e-2))", err / (float(np.abs(ref).max()) + 2e-2), None)
        assert err <= bound, f"{key}: |err| {err:.3e} > {bound:.3e}"
    assert seen == len([k for k in V.files if k.startswith("pair.g.")]) > 0


def test_pair_model_dedup_path_agrees_with_three_passes(V):
    model, batches, B = pair_case(V)
    model.eval()
    res = {}
    for mode in (False, "auto"):
        model.dedup_molecules = mode
        with torch.no_grad():
            res[mode] = torch.cat([model(b["r"], b["p1"], b["p2"], gpu=0, pair_index=b["index"]) for b in batches])
    close(res["auto"], res[False], tol=2e-6, what="pair model: distinct molecules once vs three passes")
    close(res["auto"], V["pair.out_eval"], what="pair model (de-duplicated) vs reference vectors")
    with torch.no_grad():
        again = torch.cat([model(b["r"], b["p1"], b["p2"], gpu=0, pair_index=b["index"]) for b in batches])
    assert torch.equal(again, res["auto"])
    acc = RE.pairwise_baseline_acc(model, 0, batches)
    accs = [R.pair_acc(res["auto"][lo:lo + len(b["targets"])].cpu().numpy(), b["targets"])
            for lo, b in zip(np.cumsum([0] + [len(b["targets"]) for b in batches[:-1]]), batches)]
    assert abs(acc - float(np.mean(accs))) <= 1e-6
    # with gradients wanted (train mode, p = 0) the indices are ignored: three passes, same bits as without them
    model.train()
    b = batches[0]
    y1 = model(b["r"], b["p1"], b["p2"], gpu=0, pair_index=b["index"])
    y2 = model(b["r"], b["p1"], b["p2"], gpu=0)
    assert y1.requires_grad and torch.equal(y1, y2)


def test_pair_model_rejects_mismatched_atom_counts(V):
    model, batches, B = pair_case(V)
    model.eval()
    b0, b1 = batches[0], batches[1]
    assert b0["r"].n_atoms != b1["p2"].n_atoms
    with pytest.raises(RuntimeError, match="same atoms in the same order"):
        model(b0["r"], b0["p1"], b1["p2"], gpu=0)


# ------------------------------------------------------------------------------------------------ trainers
def windows(seed0, scopes, positive_targets=False):
    out = []
    for i, scope in enumerate(scopes):
        qb = synth.make_queries(seed0 + i, len(scope), scope, atoms_lo=6, atoms_hi=12)
        tg = np.array([s.edges.shape[0] for s in qb.p_specs], np.float32) * 0.7 + 3.0 * qb.add_features[:, 0]
        tg = (tg + 0.05 * np.arange(len(tg), dtype=np.float32)).astype(np.float32)
        out.append(dict(r=featurization.BatchMolGraph(qb.r_specs, K=4), p=featurization.BatchMolGraph(qb.p_specs, K=4),
                        scope=qb.scope, targets=torch.tensor(tg), add=qb.add_features, mols_r=qb.r_specs, mols_p=qb.p_specs))
    return out


def trainer_model(selector):
    kw = dict(hidden_size=32, mpnn_depth=2, mpnn_diff_depth=2, ffn_depth=2, use_bias=True, dropout=0.1)
    if selector == "pair_baseline":
        return ranknet_baseline.build_model(task_num=2, ffn_last_layer="evidential", **kw)
    last = "evidential" if selector == "BetaNet_envidential" else "no_softplus"
    return build_model(task_num=1, ffn_last_layer=last, add_features_dim=1, **kw)


SELECTORS = {"pair_baseline": ("baseline", "baseline"), "BetaNet": ("sum_session", "BetaNet"),
             "BetaNet_envidential": ("sum_session", "BetaNet_envidential")}


@pytest.mark.parametrize("selector", list(SELECTORS))
def test_two_epochs_of_each_new_selector(selector, tmp_path):
    torch.manual_seed(0)
    strategy, task = SELECTORS[selector]
    model = trainer_model(selector).cuda()
    opt = TU.build_optimizer(model)
    sch = TU.build_lr_scheduler(opt, warmup_epochs=1.0, total_epochs=2, train_data_size=16, batch_size=4, init_lr=1e-4,
                                max_lr=5e-4, final_lr=1e-4)
    ck = str(tmp_path / "m.pt")
    before = {k: v.clone() for k, v in model.state_dict().items()}
    hist = RT.run_train(model, sch, windows(100, [[4, 3, 5], [2, 6, 1, 3], [5, 5]]), windows(200, [[4, 3], [5, 2]]), ck, opt, 2, 0, 0,
                        train_strategy=strategy, task_type=task, target_name="ea", batch_size=16, val_batch_size=10)
    assert len(hist) == 2 and all(np.isfinite(h["train_loss"]) for h in hist)
    assert any(h["checkpoint"] for h in hist) and os.path.exists(ck)
    if selector == "pair_baseline":
        assert all(0.0 <= h["acc"] <= 1.0 for h in hist)
    else:
        assert all(0.0 <= h["top1"] <= 1.0 for h in hist)
    assert any(not torch.equal(before[k], v) for k, v in model.state_dict().items() if v.dtype.is_floating_point)
    fresh = trainer_model(selector)
    scaler = load_checkpoint(ck, fresh, map_location="cpu")
    assert scaler is not None and np.isfinite(scaler["means"]) and scaler["stds"] > 0


class _SGD1:
    """Records nothing and changes nothing: the loops' first step is then comparable with a hand-made one."""
    param_groups = [dict(lr=0.0)]

    def step(self):
        pass


@pytest.mark.parametrize("selector", list(SELECTORS))
def test_first_step_of_each_loop_equals_loss_plus_backward_by_hand(selector):
    torch.manual_seed(0)
    model = trainer_model(selector).cuda()
    for m in model.modules():
        if hasattr(m, "dropout") and isinstance(getattr(m, "dropout"), float):
            m.dropout = 0.0
    model.train()
    grads = {}

    class Opt(_SGD1):
        def step(self):
            if not grads:
                grads.update({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    w = windows(300, [[4, 3, 5, 1]])
    b = w[0]
    b["targets"] = (b["targets"] - b["targets"].mean()) / b["targets"].std()
    if selector == "pair_baseline":
        pb = list(pairs.pair_windows(b["mols_r"], b["mols_p"], b["scope"], b["targets"].numpy(), 12))
        assert pb[0]["full"] and not pb[-1]["full"]
        got = TP.baseline_pairwise_training_loop(0, 3, model, Opt(), _SGD1(), pb, batch_size=12, gpu=0)
        model.zero_grad()
        loss = RL.pair_softmax_mse(model(pb[0]["r"], pb[0]["p1"], pb[0]["p2"], gpu=0), pb[0]["targets"])
        n_steps = sum(1 for x in pb if x["full"])
    else:
        n = RL.sq_pairs(b["scope"])
        if selector == "BetaNet":
            got = TP.beta_dis_train_loop(0, model, Opt(), _SGD1(), w, alpha0=100, gpu=0)
            model.zero_grad()
            loss = RL.betanet_loss(model(b["r"], b["p"], gpu=0, add_features=b["add"]), b["scope"], b["targets"], 100.0, 0)[0] / n
        else:
            got = TP.beta_evi_train_loop(1, model, Opt(), _SGD1(), w, max_coeff=0.01, epochs=3, gpu=0)
            model.zero_grad()
            coef = RL.annealing_coef(0.01, 1, 3)
            loss = RL.beta_evidential_loss(model(b["r"], b["p"], gpu=0, add_features=b["add"]), b["scope"], b["targets"], coef, 0)[0] / n
        n_steps = 1
    RL.backward(loss)
    if n_steps == 1:
        assert abs(got - float(loss.detach())) <= 1e-6 * (1 + abs(float(loss.detach())))
    assert grads
    for k, p in model.named_parameters():
        if p.grad is not None:
            err = float((grads[k] - p.grad).abs().max())                  # the same launches in the same order: rounding at most
            assert err <= 1e-6 * float(p.grad.abs().max()) + 1e-9, (k, err)
    if selector == "BetaNet_envidential":
        with pytest.raises(ValueError, match="epochs == 1"):
            TP.beta_evi_train_loop(0, model, Opt(), _SGD1(), w, epochs=1, gpu=0)
    if selector == "BetaNet":                               # a window of one-candidate queries has no pair: skipped
        assert np.isnan(TP.beta_dis_train_loop(0, model, Opt(), _SGD1(), windows(400, [[1, 1]]), gpu=0))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_process_betanet_loop_reproduces_the_one_process_loop(tmp_path, parity_log):
    job = os.path.join(REPO, "tests", "pairwise_dp_job.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("RR_F16X2", None)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    one, two = str(tmp_path / "one.json"), str(tmp_path / "two.json")
    subprocess.run([sys.executable, job, "--out", one, "--ckpt", str(tmp_path / "ck1.pt")], check=True, env=env, timeout=600)
    env2 = dict(env)
    if torch.cuda.device_count() >= 2:
        env2.setdefault("RR_DIST_BACKEND", "nccl")
    else:
        env2.update(RR_SINGLE_DEVICE="1", RR_DIST_BACKEND="gloo")
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                    "127.0.0.1", "--master-port", str(_free_port()), job, "--out", two, "--ckpt", str(tmp_path / "ck2.pt")],
                   check=True, env=env2, timeout=600)
    with open(one) as f:
        a = json.load(f)
    with open(two) as f:
        b = json.load(f)
    assert a["world"] == 1 and b["world"] == 2
    h1, h2 = a["history"], b["history"]
    assert len(h1) == len(h2) == 3
    worst = max(abs(e1["train_loss"] - e2["train_loss"]) / max(1e-6, abs(e1["train_loss"])) for e1, e2 in zip(h1, h2))
    parity_log(f"BetaNet backend={b['backend']}: max rel |loss_2proc - loss_1proc| {worst:.2e}")
    assert worst <= 1e-5, worst
    assert all(np.isfinite(e["train_loss"]) for e in h1)
    assert os.path.exists(str(tmp_path / "ck2.pt"))
