"""GPU tests of the soft ranks, the ApproxNDCG loss (csrc/approx_ndcg.hip) and its strategy: parity of the forward value and
the gradient with the float64 restatement of tests/approx_ndcg_ref.py, soft_rank on its own and composed into the loss, the
bit-level contracts of the entry points (the one-launch step against fwd + bwd, repeated calls, strided input, truncation
beyond the list, unranked queries), the one-wave and four-wave forms against each other, shard additivity and two epochs of
the trainer with the fused step on and off.

Parity measure and bound.  |loss_sum - ref| ABSOLUTE for the loss (it lies in [0, Q] and can be near 0) and max |dscore - ref|
/ max |ref| over the window for the gradient.  Bound 1e-5, the project's parity bound (test_gpu_lambdarank.BOUND): the closed
form with float32 pair terms and float64 sums stays below 2e-7 on the CPU (tests/test_approx_ndcg_cpu.py), so the bound leaves
~50x for the device's expf and division and the kernel's sums must add nothing visible.  A window whose reference gradient is
below 1e-8 everywhere (a gated long list at T = 1 goes there: 1.8e-10 at C = 4096) has no meaningful ratio; it is held to
1e-12 absolute instead, and at most one window may take that exit - none of the windows below does."""
import functools

import numpy as np
import pytest
import torch

from tests import approx_ndcg_ref as AR
from tests import helpers as Hh
from tests.test_gpu_lambdarank import BOUND, bits, seg_of, train_once

from reactranker_amd import _lib
from reactranker_amd import loss as RL

pytestmark = pytest.mark.gpu

RAGGED = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 300]   # crosses the wave (64) and workgroup (256) boundaries
WINDOWS = {   # seed -> scope
    0: RAGGED,
    1: [64] * 64,                             # the workload's shape
    2: [5, 1, 1, 7, 70],                      # every score 0.5: every soft rank is (C + 1) / 2
    3: [1000],                                # one long list
    4: [8192],                                # the LDS limit
}
SETTINGS = [(1.0, 0), (0.1, 0), (1.0, 10), (0.01, 5)]
CASES = [(seed, T, k) for seed in WINDOWS for T, k in SETTINGS if seed != 4 or (T, k) == (1.0, 0)]
DEGENERATE = []                               # the cases that took the tiny-gradient exit


@functools.lru_cache(maxsize=None)
def case_window(seed):
    score, targets = AR.window(seed, WINDOWS[seed])
    if seed == 2:
        score[:] = 0.5
    score.setflags(write=False)
    targets.setflags(write=False)
    return score, targets


@functools.lru_cache(maxsize=None)
def reference(seed, T, k):
    score, targets = case_window(seed)
    loss, ranked, grad = AR.approx_ndcg(score, WINDOWS[seed], targets, T, k)
    grad.setflags(write=False)
    return loss, ranked, grad


def grad_error(d, ref):
    d = d.detach().double().cpu().numpy().reshape(-1)
    return float(np.max(np.abs(d - ref)) / np.max(np.abs(ref)))


def measure(log, what, loss, grad, ref_loss, ref_grad):
    """records, asserts and returns the two parity measures"""
    e_loss = abs(float(loss.detach()) - ref_loss)
    top = float(np.max(np.abs(ref_grad)))
    if top < 1e-8:
        e_abs = float(np.max(np.abs(grad.detach().double().cpu().numpy().reshape(-1) - ref_grad)))
        DEGENERATE.append(what)
        log(f"{what}: loss err {e_loss:.3e} (bound {BOUND:g}); reference gradient max {top:.3e} < 1e-8, absolute err {e_abs:.3e} (bound 1e-12)")
        assert e_loss <= BOUND and e_abs <= 1e-12 and len(DEGENERATE) <= 1, (e_loss, e_abs, DEGENERATE)
        return e_loss, e_abs
    e_grad = grad_error(grad, ref_grad)
    Hh.record(what + " loss", e_loss, BOUND)
    Hh.record(what + " grad", e_grad, BOUND)
    log(f"{what}: loss err {e_loss:.3e} abs, grad err {e_grad:.3e} of max (bound {BOUND:g})")
    assert e_loss <= BOUND and e_grad <= BOUND, (e_loss, e_grad)
    return e_loss, e_grad


class Raw:
    """the entry points called directly on device tensors"""

    def __init__(self, score, scope, targets, T=1.0, k=0):
        self.s = score if torch.is_tensor(score) else torch.tensor(np.asarray(score, np.float32)).cuda()
        self.t = torch.tensor(np.asarray(targets, np.float32)).cuda()
        self.seg, self.Q, self.L = seg_of(scope), len(scope), max(list(scope) + [0])
        self.n = int(sum(scope))
        self.head = [_lib.ptr(self.s), self.s.stride(0), _lib.ptr(self.t), _lib.ptr(self.seg), self.Q, self.L, float(T), int(k)]
        self.part = torch.empty(max(2 * self.Q, 2), dtype=torch.float32, device="cuda")

    def _nan(self):
        return torch.full((max(self.n, 1),), float("nan"), device="cuda")      # every entry must be WRITTEN

    def fwd(self):
        loss = torch.full((1,), float("nan"), device="cuda")
        ranked = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        _lib.check(_lib.lib().rr_approx_ndcg_fwd_f32(*self.head, _lib.ptr(loss), _lib.ptr(ranked), _lib.ptr(self.part), _lib.stream()))
        return loss, ranked

    def bwd(self, gloss):
        d = self._nan()
        g = torch.tensor([gloss], dtype=torch.float32).cuda()
        _lib.check(_lib.lib().rr_approx_ndcg_bwd_f32(*self.head, _lib.ptr(g), _lib.ptr(d), 1, _lib.stream()))
        return d[:self.n]

    def step(self, scale, counter):
        loss = torch.full((1,), float("nan"), device="cuda")
        ranked = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        d = self._nan()
        _lib.check(_lib.lib().rr_approx_ndcg_step_f32(*self.head, float(scale), _lib.ptr(loss), _lib.ptr(ranked), _lib.ptr(self.part),
                                                      _lib.ptr(counter), _lib.ptr(d), 1, _lib.stream()))
        return loss, ranked, d[:self.n]

    def ranks(self):
        a = self._nan()
        _lib.check(_lib.lib().rr_approx_ndcg_ranks_f32(*self.head, _lib.ptr(a), 1, _lib.stream()))
        return a[:self.n]


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("seed,T,k", CASES)
def test_forward_and_gradient_against_the_float64_restatement(seed, T, k, parity_log):
    scope = WINDOWS[seed]
    score, targets = case_window(seed)
    ref_loss, ref_ranked, ref_grad = reference(seed, T, k)
    tt = torch.tensor(np.array(targets))
    score = np.array(score)
    s = torch.tensor(score).cuda().requires_grad_(True)
    loss, ranked = RL.approx_ndcg_loss(s, scope, tt, T, k, 0)            # (the step launch; autograd's own ones -> bwd kernel)
    assert loss.dim() == 0 and ranked.dtype == torch.int64
    loss.backward()
    assert int(ranked) == ref_ranked                                     # exactly
    measure(parity_log, f"seed {seed} T {T} k {k}", loss, s.grad, ref_loss, ref_grad)
    with torch.no_grad():                                                # the forward entry point alone: the same bits
        loss_f, ranked_f = RL.approx_ndcg_loss(torch.tensor(score).cuda(), scope, tt, T, k, 0)
    assert bits(loss_f.reshape(1), loss.detach().reshape(1)) and int(ranked_f) == ref_ranked
    if seed == 0 and k == 0:                                             # normalised by a host query count, fused hand-out
        Q = len(scope)
        s2 = torch.tensor(score).cuda().requires_grad_(True)
        l2, _ = RL.approx_ndcg_loss(s2, scope, tt, T, k, 0, queries=Q)
        hits = RL.FusedStep.hits
        RL.backward(l2)
        assert RL.FusedStep.hits == hits + 1
        measure(parity_log, f"seed 0 T {T} over queries", l2, s2.grad, ref_loss / Q, ref_grad / Q)


# ------------------------------------------------------------------------------------------------ 2. soft_rank
def test_soft_rank_forward_and_backward_against_the_restatement(parity_log):
    score, _ = case_window(0)
    up = np.random.default_rng(7).standard_normal(len(score)).astype(np.float32)
    for T in (1.0, 0.1, 0.01):
        ref_r, ref_g = AR.soft_rank(score, RAGGED, T, up)
        s = torch.tensor(np.array(score)).cuda().requires_grad_(True)
        r = RL.soft_rank(s, RAGGED, T, 0)
        assert r.shape == (len(score),) and r.dtype == torch.float32
        (r * torch.tensor(up).cuda()).sum().backward()
        e_r = float(np.max(np.abs(r.detach().double().cpu().numpy() - ref_r) / ref_r))
        e_g = grad_error(s.grad, ref_g)
        Hh.record(f"soft_rank T {T} rank", e_r, BOUND)
        Hh.record(f"soft_rank T {T} grad", e_g, BOUND)
        parity_log(f"soft_rank ragged T {T}: rank err {e_r:.3e} relative, grad err {e_g:.3e} of max (bound {BOUND:g})")
        assert e_r <= BOUND and e_g <= BOUND, (T, e_r, e_g)
        off = 0
        for c in RAGGED:                                                 # the ranks of a query sum to C (C + 1) / 2
            assert abs(float(r.detach()[off:off + c].double().sum()) - c * (c + 1) / 2) <= BOUND * max(1, c * (c + 1) / 2), c
            off += c


@pytest.mark.parametrize("T,k", [(1.0, 0), (0.1, 10)])
def test_soft_rank_times_the_rank_gradient_backpropagates_to_the_loss_gradient(T, k, parity_log):
    score, targets = case_window(0)
    tt = torch.tensor(np.array(targets))
    s = torch.tensor(np.array(score)).cuda().requires_grad_(True)
    loss, _ = RL.approx_ndcg_loss(s, RAGGED, tt, T, k, 0)
    loss.backward()
    a = Raw(score, RAGGED, targets, T, k).ranks()
    assert torch.isfinite(a).all() and float(a[:1 + 2 + 3].abs().max()) > 0
    assert float(a[0]) == 0.0                                            # (the one-candidate query is unranked)
    _, _, _, ref_a = AR.approx_ndcg(score, RAGGED, targets, T, k, terms=True)
    e_a = grad_error(a, ref_a)
    s2 = torch.tensor(np.array(score)).cuda().requires_grad_(True)
    (RL.soft_rank(s2, RAGGED, T, 0) * a).sum().backward()
    e = grad_error(s2.grad, s.grad.double().cpu().numpy())
    parity_log(f"ragged T {T} k {k}: a err {e_a:.3e} of max against the restatement, composed grad err {e:.3e} of max (bound {BOUND:g})")
    assert e_a <= BOUND and e <= BOUND, (e_a, e)


# ------------------------------------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("k", [0, 10])
def test_step_writes_the_bits_of_forward_then_backward_on_every_call(k):
    scope = [5, 64, 65, 300, 2]
    score, targets = AR.window(14, scope)
    r = Raw(score, scope, targets, 0.5, k)
    loss_sum, ranked = r.fwd()
    assert int(ranked) == 5
    scale = float(np.float32(1.0 / len(scope)))
    d = r.bwd(scale)
    assert bits(r.bwd(scale), d) and bits(r.fwd()[0], loss_sum)          # a second call gives the same bits
    want_loss = torch.tensor([np.float32(loss_sum.item()) * np.float32(scale)], dtype=torch.float32).cuda()
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    for launch in range(3):                                              # one counter word, left at zero every time
        r.part.fill_(float("nan"))
        loss, p, ds = r.step(scale, ctr)
        assert int(ctr) == 0, launch
        assert bits(loss, want_loss) and int(p) == 5, launch
        assert bits(ds, d), launch
    ctr.fill_(3 * len(scope))                                            # a multiple of Q serves like zero
    loss, p, ds = r.step(scale, ctr)
    assert int(ctr) == 0 and bits(loss, want_loss) and bits(ds, d)


def test_column_of_a_two_column_output_gives_the_bits_of_the_contiguous_call():
    scope = [5, 64, 65, 300, 2]
    score, targets = AR.window(13, scope)
    tt = torch.tensor(targets)
    out = torch.stack([torch.tensor(score), torch.tensor(score[::-1].copy())], 1).cuda().requires_grad_(True)
    assert out[:, 0].stride(0) == 2
    la, ra = RL.approx_ndcg_loss(out, scope, tt, 0.5, 10, 0)             # [M, 2]: the first column, read in place
    la.backward()
    s = torch.tensor(score).cuda().requires_grad_(True)
    lb, rb = RL.approx_ndcg_loss(s, scope, tt, 0.5, 10, 0)
    lb.backward()
    assert bits(la.detach().reshape(1), lb.detach().reshape(1)) and int(ra) == int(rb)
    assert bits(out.grad[:, 0].contiguous(), s.grad) and float(out.grad[:, 1].abs().max()) == 0.0
    r = Raw(out.detach()[:, 0], scope, targets, 0.5, 10)                 # and at the C ABI
    assert r.head[1] == 2
    lr_, _ = r.fwd()
    assert bits(lr_, lb.detach().reshape(1)) and bits(r.bwd(1.0), s.grad)
    up = torch.tensor(np.random.default_rng(2).standard_normal(len(score)).astype(np.float32)).cuda()
    out2 = out.detach().clone().requires_grad_(True)                     # soft_rank likewise
    s2 = s.detach().clone().requires_grad_(True)
    ra_, rb_ = RL.soft_rank(out2, scope, 0.5, 0), RL.soft_rank(s2, scope, 0.5, 0)
    (ra_ * up).sum().backward()
    (rb_ * up).sum().backward()
    assert bits(ra_.detach(), rb_.detach()) and bits(out2.grad[:, 0].contiguous(), s2.grad)


def test_ndcg_k_at_or_beyond_the_list_length_gives_the_bits_of_zero():
    scope = [5, 64, 65]
    score, targets = AR.window(11, scope)
    base = Raw(score, scope, targets, 1.0, 0)
    l0, p0 = base.fwd()
    d0 = base.bwd(1.0)
    assert torch.isfinite(d0).all() and 0 < float(l0) < 3
    for k in (65, 66, 1000, 2 ** 31 - 1):
        r = Raw(score, scope, targets, 1.0, k)
        l, p = r.fwd()
        assert bits(l, l0) and int(p) == int(p0) == 3, k
        assert bits(r.bwd(1.0), d0), k
    l64, _ = Raw(score, scope, targets, 1.0, 64).fwd()                   # (64 does gate the list of 65)
    assert not bits(l64, l0)


def test_unranked_queries_add_nothing_and_their_gradient_is_written_as_zero(parity_log):
    scope = [4, 3, 1, 0, 5, 70]
    score, targets = AR.window(12, scope)
    targets[0:4] = 0.25                                                   # query 0: all targets equal; 2: one candidate; 3: empty
    targets[13:83] = -1.5                                                 # query 5: a four-wave list of equal targets
    r = Raw(score, scope, targets, 1.0, 0)
    loss, ranked = r.fwd()
    d = r.bwd(1.0)                                                        # into a NaN-filled buffer
    a = r.ranks()
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    loss_s, ranked_s, d_s = r.step(1.0, ctr)                              # likewise
    ref_loss, ref_ranked, ref_grad = AR.approx_ndcg(score, scope, targets, 1.0, 0)
    assert int(ranked) == int(ranked_s) == ref_ranked == 2
    zero = torch.zeros(83, device="cuda")
    for dd in (d, d_s, a):
        assert torch.isfinite(dd).all()
        assert torch.equal(dd[0:4], zero[0:4]) and float(dd[7]) == 0.0 and torch.equal(dd[13:83], zero[13:83])
    measure(parity_log, "unranked window", loss, d, ref_loss, ref_grad)
    assert bits(loss_s, loss) and bits(d_s, d) and int(ctr) == 0
    # a window of unranked queries only: zero loss, zero count, zeros written
    r = Raw(score[:5], [4, 1, 0], targets[:5], 1.0, 0)
    loss, ranked = r.fwd()
    assert float(loss) == 0.0 and int(ranked) == 0 and torch.equal(r.bwd(1.0), torch.zeros(5, device="cuda"))
    # and no query at all
    r = Raw(torch.zeros(1, device="cuda"), [], np.zeros(1, np.float32), 1.0, 0)
    loss, ranked = r.fwd()
    assert float(loss) == 0.0 and int(ranked) == 0
    loss, ranked, _ = r.step(0.5, ctr)
    assert float(loss) == 0.0 and int(ranked) == 0 and int(ctr) == 0


def test_one_wave_and_four_waves_agree_on_a_list_of_64(parity_log):
    scope = [64, 3, 64]
    score, targets = AR.window(16, scope)
    l = _lib.lib()
    got = {}
    try:
        for w in (1, 4):
            assert l.rr_approx_ndcg_set_waves(w) == 0 and l.rr_approx_ndcg_waves() == w
            r = Raw(score, scope, targets, 0.5, 10)
            got[w] = (r.fwd()[0], r.bwd(1.0))
    finally:
        assert l.rr_approx_ndcg_set_waves(0) == 0
    ref_loss, _, ref_grad = AR.approx_ndcg(score, scope, targets, 0.5, 10)
    for w in (1, 4):
        measure(parity_log, f"{w} wave(s), lists of 64", got[w][0], got[w][1], ref_loss, ref_grad)
    e_loss = abs(float(got[1][0]) - float(got[4][0]))
    e_grad = grad_error(got[1][1], got[4][1].double().cpu().numpy())
    parity_log(f"1 wave against 4 waves: loss {e_loss:.3e} abs, grad {e_grad:.3e} of max")
    assert e_loss <= BOUND and e_grad <= BOUND


# ------------------------------------------------------------------------------------------------ 4. shards and training
def test_shards_normalised_by_the_window_add_up_to_the_window():
    scope = [3, 70, 2, 9, 130, 4]          # both shards and the window are longer than 64: all three run four waves, and a
    score, targets = AR.window(15, scope)  # query's gradient depends on nothing but the query and the scale - the same bits
    Q = len(scope)

    def run(lo, hi):
        a, b = sum(scope[:lo]), sum(scope[:hi])
        s = torch.tensor(score[a:b]).cuda().requires_grad_(True)
        loss, own = RL.approx_ndcg_loss(s, scope[lo:hi], torch.tensor(targets[a:b]), 0.5, 0, 0, queries=Q)
        RL.backward(loss)
        return loss.detach().double().item(), int(own), s.grad

    lw, rw, gw = run(0, 6)
    l0, r0, g0 = run(0, 2)
    l1, r1, g1 = run(2, 6)
    assert rw == r0 + r1 == 6
    assert abs((l0 + l1) - lw) <= 1e-6 * abs(lw)                         # (three float32 sums of float32 partials)
    assert bits(torch.cat([g0, g1]), gw)


def test_two_epochs_of_the_approx_ndcg_strategy_fused_and_unfused():
    hits = RL.FusedStep.hits
    fused = train_once("approx_ndcg", True, temperature=0.5, ndcg_k=0)
    assert RL.FusedStep.hits == hits + 2 * 4, "one hand-out per optimizer step"
    plain = train_once("approx_ndcg", False, temperature=0.5, ndcg_k=0)
    assert RL.FusedStep.hits == hits + 2 * 4
    assert len(fused) == len(plain) == 2
    assert all(np.isfinite(h["train_loss"]) and 0 < h["train_loss"] < 1 for h in fused)   # a mean of 1 - NDCG values
    assert all(0.0 <= h["top1"] <= 1.0 for h in fused)
    assert [h["train_loss"] for h in fused] == [h["train_loss"] for h in plain]
    assert fused[1]["train_loss"] < fused[0]["train_loss"]
    other = train_once("approx_ndcg", True, temperature=0.1, ndcg_k=2)   # another temperature and truncation is another loss
    assert all(np.isfinite(h["train_loss"]) for h in other)
    assert [h["train_loss"] for h in other] != [h["train_loss"] for h in fused]
