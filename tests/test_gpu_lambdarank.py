"""GPU tests of the LambdaRank loss (csrc/lambdarank.hip) and strategy: parity of the forward value and the gradient with
the float64 restatement of tests/lambdarank_ref.py, the bit-level contracts of the entry points (truncation beyond the list,
pair-less queries, strided input, the one-launch step against the two-kernel path, shard additivity) and two epochs of the
trainer with the fused step on and off.

Parity measure and bound.  |loss_sum - ref| / |ref| for the loss and max |dscore - ref| / max |ref| over the window for the
gradient - scaled to its largest entry because the project's usual 1e-5 * (1 + |ref|) is vacuous for gradient entries that
are ~1e-5 themselves once divided by the pair count.  Bound 1e-5, the project's parity bound: the same formulas in plain
float32 torch arithmetic stay below 2e-7 on both measures for these windows, so the bound leaves ~50x for the device's
expf / logf and its summation order."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import lambdarank_ref as LR

from reactranker_amd import _lib, featurization, synth
from reactranker_amd import loss as RL
from reactranker_amd import run_train_pairwise as RT
from reactranker_amd import train_utils as TU
from reactranker_amd.base_model import build_model

pytestmark = pytest.mark.gpu
BOUND = 1e-5

WINDOWS = {   # seed -> scope
    0: [1, 2, 3, 32, 64, 65, 129, 300],       # mixed list lengths
    1: [64] * 64,                             # the workload's shape
    2: [5, 1, 1, 7],                          # every score 0.5: the tie rule decides every rank
    3: [1000],                                # one long list
    4: [8192],                                # the LDS limit
}
SETTINGS = [(1.0, 0), (0.5, 1), (1.0, 10)]
CASES = [(seed, sigma, k) for seed in WINDOWS for sigma, k in SETTINGS if seed != 4 or (sigma, k) == (1.0, 0)]


@functools.lru_cache(maxsize=None)
def case_window(seed):
    score, targets = LR.window(seed, WINDOWS[seed])
    if seed == 2:
        score[:] = 0.5
    score.setflags(write=False)
    targets.setflags(write=False)
    return score, targets


@functools.lru_cache(maxsize=None)
def reference(seed, sigma, k):
    score, targets = case_window(seed)
    loss, pairs, grad = LR.lambdarank(score, WINDOWS[seed], targets, sigma, k)
    grad.setflags(write=False)
    return loss, pairs, grad


def measure(what, loss, grad, ref_loss, ref_grad):
    """records and returns the two parity measures"""
    e_loss = abs(float(loss.detach()) - ref_loss) / abs(ref_loss)
    g = grad.detach().double().cpu().numpy().reshape(-1)
    e_grad = float(np.max(np.abs(g - ref_grad)) / np.max(np.abs(ref_grad)))
    Hh.record(what + " loss", e_loss, BOUND)
    Hh.record(what + " grad", e_grad, BOUND)
    print(f"[lambdarank] {what}: loss err {e_loss:.3e}, grad err {e_grad:.3e} (bound {BOUND:g})")
    return e_loss, e_grad


def seg_of(scope):
    return torch.tensor(np.concatenate([[0], np.cumsum(scope)]).astype(np.int32)).cuda()


class Raw:
    """the three entry points called directly on device tensors"""

    def __init__(self, score, scope, targets, sigma=1.0, k=0):
        self.s = score if torch.is_tensor(score) else torch.tensor(score).cuda()
        self.t = torch.tensor(np.asarray(targets, np.float32)).cuda()
        self.seg, self.Q, self.L = seg_of(scope), len(scope), max(list(scope) + [0])
        self.n = int(sum(scope))
        self.head = [_lib.ptr(self.s), self.s.stride(0), _lib.ptr(self.t), _lib.ptr(self.seg), self.Q, self.L, float(sigma), int(k)]
        self.part = torch.empty(max(2 * self.Q, 2), dtype=torch.float32, device="cuda")

    def fwd(self):
        loss = torch.full((1,), float("nan"), device="cuda")
        pairs = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        _lib.check(_lib.lib().rr_lambdarank_fwd_f32(*self.head, _lib.ptr(loss), _lib.ptr(pairs), _lib.ptr(self.part), _lib.stream()))
        return loss, pairs

    def bwd(self, gloss):
        d = torch.full((max(self.n, 1),), float("nan"), device="cuda")      # every entry must be WRITTEN
        g = torch.tensor([gloss], dtype=torch.float32).cuda()
        _lib.check(_lib.lib().rr_lambdarank_bwd_f32(*self.head, _lib.ptr(g), _lib.ptr(d), 1, _lib.stream()))
        return d[:self.n]

    def step(self, scale, counter):
        loss = torch.full((1,), float("nan"), device="cuda")
        pairs = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        d = torch.full((max(self.n, 1),), float("nan"), device="cuda")
        _lib.check(_lib.lib().rr_lambdarank_step_f32(*self.head, float(scale), _lib.ptr(loss), _lib.ptr(pairs), _lib.ptr(self.part),
                                                     _lib.ptr(counter), _lib.ptr(d), 1, _lib.stream()))
        return loss, pairs, d[:self.n]


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("seed,sigma,k", CASES)
def test_forward_and_gradient_against_the_float64_restatement(seed, sigma, k):
    scope = WINDOWS[seed]
    score, targets = case_window(seed)
    ref_loss, ref_pairs, ref_grad = reference(seed, sigma, k)
    tt = torch.tensor(np.array(targets))
    score = np.array(score)
    s = torch.tensor(score).cuda().requires_grad_(True)
    loss, pairs = RL.lambdarank_loss(s, scope, tt, sigma, k, 0)          # (the step launch; autograd's own ones -> bwd kernel)
    assert loss.dim() == 0 and pairs.dtype == torch.int64
    loss.backward()
    assert int(pairs) == ref_pairs                                       # exactly
    e_loss, e_grad = measure(f"seed {seed} sigma {sigma} k {k}", loss, s.grad, ref_loss, ref_grad)
    assert e_loss <= BOUND and e_grad <= BOUND, (e_loss, e_grad)
    with torch.no_grad():                                                # the forward entry point alone: the same bits
        loss_f, pairs_f = RL.lambdarank_loss(torch.tensor(score).cuda(), scope, tt, sigma, k, 0)
    assert bits(loss_f.reshape(1), loss.detach().reshape(1)) and int(pairs_f) == ref_pairs
    if seed == 0 and k == 0:                                             # normalised by a host pair count, fused hand-out
        s2 = torch.tensor(score).cuda().requires_grad_(True)
        l2, _ = RL.lambdarank_loss(s2, scope, tt, sigma, k, 0, pairs=ref_pairs)
        hits = RL.FusedStep.hits
        RL.backward(l2)
        assert RL.FusedStep.hits == hits + 1
        e_loss, e_grad = measure("seed 0 over pairs", l2, s2.grad, ref_loss / ref_pairs, ref_grad / ref_pairs)
        assert e_loss <= BOUND and e_grad <= BOUND, (e_loss, e_grad)


# ------------------------------------------------------------------------------------------------ 2. truncation beyond the list
def test_ndcg_k_at_or_beyond_the_list_length_gives_the_bits_of_zero():
    scope = [5, 64, 65]
    score, targets = LR.window(11, scope)
    base = Raw(score, scope, targets, 1.0, 0)
    l0, p0 = base.fwd()
    d0 = base.bwd(1.0)
    assert torch.isfinite(d0).all() and float(l0) > 0
    for k in (65, 66, 1000, 2 ** 31 - 1):
        r = Raw(score, scope, targets, 1.0, k)
        l, p = r.fwd()
        assert bits(l, l0) and int(p) == int(p0), k
        assert bits(r.bwd(1.0), d0), k
    l64, _ = Raw(score, scope, targets, 1.0, 64).fwd()                   # (64 does truncate the list of 65)
    assert not bits(l64, l0)


# ------------------------------------------------------------------------------------------------ 3. pair-less queries
def test_pairless_queries_add_nothing_and_their_gradient_is_written_as_zero():
    scope = [4, 3, 1, 0, 5]
    score, targets = LR.window(12, scope)
    targets[0:4] = 0.25                                                   # query 0: all targets equal; query 2 has one candidate
    r = Raw(score, scope, targets, 1.0, 0)
    loss, pairs = r.fwd()
    d = r.bwd(1.0)                                                        # into a NaN-filled buffer
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    loss_s, pairs_s, d_s = r.step(1.0, ctr)                               # likewise
    refs = [LR.lambdarank(score[a:b], [b - a], targets[a:b], 1.0, 0) for a, b in ((4, 7), (8, 13))]
    for dd in (d, d_s):
        assert torch.isfinite(dd).all()
        assert torch.equal(dd[0:4], torch.zeros(4, device="cuda")) and float(dd[7]) == 0.0
    assert int(pairs) == int(pairs_s) == refs[0][1] + refs[1][1] == 2 * (3 + 10)
    ref_loss = refs[0][0] + refs[1][0]
    ref_grad = np.concatenate([np.zeros(4), refs[0][2], np.zeros(1), refs[1][2]])
    e_loss, e_grad = measure("pair-less window", loss, d, ref_loss, ref_grad)
    assert e_loss <= BOUND and e_grad <= BOUND
    assert bits(loss_s, loss) and bits(d_s, d) and int(ctr) == 0
    # a window of pair-less queries only: zero loss, zero pairs, zeros written
    r = Raw(score[:5], [4, 1, 0], targets[:5], 1.0, 0)
    loss, pairs = r.fwd()
    assert float(loss) == 0.0 and int(pairs) == 0 and torch.equal(r.bwd(1.0), torch.zeros(5, device="cuda"))
    # and no query at all
    r = Raw(torch.zeros(1, device="cuda"), [], np.zeros(1, np.float32), 1.0, 0)
    loss, pairs = r.fwd()
    assert float(loss) == 0.0 and int(pairs) == 0
    loss, pairs, _ = r.step(0.5, ctr)
    assert float(loss) == 0.0 and int(pairs) == 0 and int(ctr) == 0


# ------------------------------------------------------------------------------------------------ 4. strided input
def test_column_of_a_two_column_output_gives_the_bits_of_the_contiguous_call():
    scope = [5, 64, 65, 300, 2]
    score, targets = LR.window(13, scope)
    tt = torch.tensor(targets)
    out = torch.stack([torch.tensor(score), torch.tensor(score[::-1].copy())], 1).cuda().requires_grad_(True)
    assert out[:, 0].stride(0) == 2
    la, pa = RL.lambdarank_loss(out, scope, tt, 1.0, 10, 0)              # [M, 2]: the first column, read in place
    la.backward()
    s = torch.tensor(score).cuda().requires_grad_(True)
    lb, pb = RL.lambdarank_loss(s, scope, tt, 1.0, 10, 0)
    lb.backward()
    assert bits(la.detach().reshape(1), lb.detach().reshape(1)) and int(pa) == int(pb)
    assert bits(out.grad[:, 0].contiguous(), s.grad) and float(out.grad[:, 1].abs().max()) == 0.0
    r = Raw(out.detach()[:, 0], scope, targets, 1.0, 10)                 # and at the C ABI
    assert r.head[1] == 2
    lr_, _ = r.fwd()
    assert bits(lr_, lb.detach().reshape(1)) and bits(r.bwd(1.0), s.grad)


# ------------------------------------------------------------------------------------------------ 5. step against fwd + bwd
@pytest.mark.parametrize("k", [0, 10])
def test_step_writes_the_bits_of_forward_then_backward(k):
    scope = [5, 64, 65, 300, 2]
    score, targets = LR.window(14, scope)
    r = Raw(score, scope, targets, 1.0, k)
    loss_sum, pairs = r.fwd()
    scale = float(np.float32(1.0 / int(pairs)))
    d = r.bwd(scale)
    want_loss = torch.tensor([np.float32(loss_sum.item()) * np.float32(scale)], dtype=torch.float32).cuda()
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    for launch in range(3):                                              # one counter word, left at zero every time
        r.part.fill_(float("nan"))
        loss, p, ds = r.step(scale, ctr)
        assert int(ctr) == 0, launch
        assert bits(loss, want_loss) and int(p) == int(pairs), launch
        assert bits(ds, d), launch
    ctr.fill_(3 * len(scope))                                            # a multiple of Q serves like zero
    loss, p, ds = r.step(scale, ctr)
    assert int(ctr) == 0 and bits(loss, want_loss) and bits(ds, d)


# ------------------------------------------------------------------------------------------------ 6. shard additivity
def test_shards_normalised_by_the_window_add_up_to_the_window():
    scope = [3, 70, 2, 9, 130, 4]
    score, targets = LR.window(15, scope)
    _, pairs = Raw(score, scope, targets).fwd()
    P = int(pairs)

    def run(lo, hi):
        a, b = sum(scope[:lo]), sum(scope[:hi])
        s = torch.tensor(score[a:b]).cuda().requires_grad_(True)
        loss, own = RL.lambdarank_loss(s, scope[lo:hi], torch.tensor(targets[a:b]), 1.0, 0, 0, pairs=P)
        RL.backward(loss)
        return loss.detach().double().item(), int(own), s.grad

    lw, pw, gw = run(0, 6)
    l0, p0, g0 = run(0, 2)
    l1, p1, g1 = run(2, 6)
    assert pw == P == p0 + p1
    assert abs((l0 + l1) - lw) <= 1e-6 * abs(lw)
    assert bits(torch.cat([g0, g1]), gw)


# ------------------------------------------------------------------------------------------------ 7. trainer
def windows(seed0, scopes):
    out = []
    for i, scope in enumerate(scopes):
        qb = synth.make_queries(seed0 + i, len(scope), scope, atoms_lo=6, atoms_hi=12)
        tg = np.array([s.edges.shape[0] for s in qb.p_specs], np.float32) * 0.7 + 3.0 * qb.add_features[:, 0]
        tg = (tg + 0.05 * np.arange(len(tg), dtype=np.float32)).astype(np.float32)
        out.append(dict(r=featurization.BatchMolGraph(qb.r_specs, K=4), p=featurization.BatchMolGraph(qb.p_specs, K=4),
                        scope=qb.scope, targets=torch.tensor(tg), add=qb.add_features))
    return out


def train_once(strategy, fused, **kw):
    old = RL.FusedStep.enabled
    RL.FusedStep.enabled = fused
    try:
        torch.manual_seed(0)
        model = build_model(task_num=1, ffn_last_layer="no_softplus", add_features_dim=1, hidden_size=32, mpnn_depth=2,
                            mpnn_diff_depth=2, ffn_depth=2, use_bias=True, dropout=0.0).cuda()
        opt = TU.build_optimizer(model)
        sch = TU.build_lr_scheduler(opt, warmup_epochs=1.0, total_epochs=2, train_data_size=16, batch_size=4, init_lr=1e-4,
                                    max_lr=5e-4, final_lr=1e-4)
        train_w = windows(500, [[4, 3, 5], [2, 6, 9, 3], [5, 5, 2, 7, 3], [8, 2, 4]])
        val_w = windows(600, [[4, 3], [5, 2]])
        return RT.run_train(model, sch, train_w, val_w, None, opt, 2, 0, 0, train_strategy=strategy, task_type="baseline",
                            target_name="ea", **kw)
    finally:
        RL.FusedStep.enabled = old


def test_two_epochs_of_the_lambdarank_strategy_fused_and_unfused():
    before = train_once("sum_session", True)                             # taken before any LambdaRank call of this test
    hits = RL.FusedStep.hits
    fused = train_once("lambdarank", True, ndcg_k=0)
    assert RL.FusedStep.hits == hits + 2 * 4, "one hand-out per optimizer step"
    plain = train_once("lambdarank", False, ndcg_k=0)
    assert RL.FusedStep.hits == hits + 2 * 4
    assert len(fused) == len(plain) == 2
    assert all(np.isfinite(h["train_loss"]) and h["train_loss"] > 0 for h in fused)
    assert all(0.0 <= h["top1"] <= 1.0 for h in fused)
    assert [h["train_loss"] for h in fused] == [h["train_loss"] for h in plain]
    assert [h["train_loss"] for h in fused] != [h["train_loss"] for h in before]
    top = train_once("lambdarank", True, ndcg_k=1)                       # another truncation is another loss
    assert all(np.isfinite(h["train_loss"]) for h in top)
    assert [h["train_loss"] for h in top] != [h["train_loss"] for h in fused]
    after = train_once("sum_session", True)
    assert after == before
