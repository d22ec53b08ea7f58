"""GPU tests of the count-carrying finish the window losses share (finish_counted, csrc/loss_list.h): the second launch of
rr_ranknet_fwd_f32, rr_lambdarank_fwd_f32 and rr_approx_ndcg_fwd_f32, and the last-arriver finish inside
rr_lambdarank_step_f32 and rr_approx_ndcg_step_f32.  The entry points are called at the C ABI with the caller's own `partial`
buffer [2 * Q] (the query's loss as a float, its count as an int32), which is read back after every call:
  - the loss has exactly the bits of reduce_scale_kernel's order over the float halves (256 strided accumulators, then the
    halving tree of block_sum, csrc/wave_util.h), restated in numpy float32, times `scale` in float32;
  - the int64 count is the exact sum of the int32 halves;
  - step and fwd agree bit for bit, and the step leaves its ticket word at zero;
  - a window without queries gives +0.0f and 0.
The window sizes sit on each side of every edge of fixed_sum: one lane stride at 64, its four accumulators at 256.  Queries
have 1 to 4 candidates, some a single one and some with all targets equal, so both halves of a partial can be zero.
Every assertion is exact: no tolerances."""
import functools

import numpy as np
import pytest
import torch

from reactranker_amd import _lib

pytestmark = pytest.mark.gpu

QS = [1, 2, 63, 64, 65, 255, 256, 257, 600]
SCALES = [1.0, float(np.float32(0.37))]
# entry-point stem -> its hyper-parameters (sigma | temperature, ndcg_k), whether it has a step entry
KINDS = {"ranknet": ((1.0,), False), "lambdarank": ((1.0, 0), True), "approx_ndcg": ((1.0, 0), True)}


@functools.lru_cache(maxsize=None)
def window(Q):
    """(scope, score, targets) of Q queries: every fifth has one candidate, every seventh equal targets"""
    rng = np.random.default_rng(1000 + Q)
    scope = [1 if q % 5 == 3 else int(rng.integers(1, 5)) for q in range(Q)]
    score = rng.standard_normal(sum(scope)).astype(np.float32)
    targets = rng.integers(0, 3, sum(scope)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(scope)])
    for q in range(0, Q, 7):
        targets[off[q]:off[q + 1]] = 1.0
    for a in (score, targets):
        a.setflags(write=False)
    return tuple(scope), score, targets


def fixed_order_sum(v):
    """reduce_scale_kernel's sum of the float32 vector v: thread t adds v[t], v[t + 256], ... to 0.f in that order, then
    block_sum's tree, red[t] += red[t + o] for o = 128, 64, ..., 1"""
    v = np.asarray(v, np.float32)
    pad = np.zeros((len(v) + 255) // 256 * 256, np.float32)        # (x + 0.f == x: an accumulator is never -0.f)
    pad[:len(v)] = v
    acc = np.zeros(256, np.float32)
    for row in pad.reshape(-1, 256):
        acc = acc + row
    o = 128
    while o > 0:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o >>= 1
    return np.float32(acc[0])


class Call:
    """one window on the device and the buffers of a call, poisoned before every launch"""

    def __init__(self, scope, score, targets):
        self.Q, self.n = len(scope), int(sum(scope))
        self.s = torch.tensor(np.asarray(score, np.float32) if self.n else np.zeros(1, np.float32)).cuda()
        self.t = torch.tensor(np.asarray(targets, np.float32) if self.n else np.zeros(1, np.float32)).cuda()
        self.seg = torch.tensor(np.concatenate([[0], np.cumsum(scope)]).astype(np.int32)).cuda()
        self.L = max(list(scope) + [0])
        self.counter = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(self, kind, step, scale=1.0):
        """returns (loss bits, count, float halves, int32 halves) of one fwd or step call"""
        hyper, _ = KINDS[kind]
        loss = torch.full((1,), float("nan"), device="cuda")
        count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        part = torch.full((max(2 * self.Q, 2),), float("nan"), device="cuda")
        head = [_lib.ptr(self.s), 1, _lib.ptr(self.t), _lib.ptr(self.seg), self.Q, self.L, *hyper]
        if step:
            d = torch.empty(max(self.n, 1), device="cuda")
            name, tail = f"rr_{kind}_step_f32", [float(scale), _lib.ptr(loss), _lib.ptr(count), _lib.ptr(part),
                                                 _lib.ptr(self.counter), _lib.ptr(d), 1]
        else:
            name, tail = f"rr_{kind}_fwd_f32", [_lib.ptr(loss), _lib.ptr(count), _lib.ptr(part)]
        _lib.check(getattr(_lib.lib(), name)(*head, *tail, _lib.stream()), name)
        p = part[:2 * self.Q].cpu().numpy()
        return int(loss.view(torch.int32).item()), int(count.item()), p[0::2].copy(), p.view(np.int32)[1::2].copy()


def bits_of(x):
    return int(np.float32(x).view(np.int32))


@pytest.mark.parametrize("Q", QS)
def test_loss_bits_and_count_of_every_entry_point(Q):
    call = Call(*window(Q))
    for kind, (_, has_step) in KINDS.items():
        loss, count, vals, counts = call.run(kind, step=False)
        assert not np.isnan(vals).any(), f"{kind}: a partial was not written"
        if Q >= 63:
            assert (counts == 0).any() and (counts > 0).any(), f"{kind}: the window lost its empty or its counted queries"
        assert np.all(vals[counts == 0] == 0.0)
        assert loss == bits_of(fixed_order_sum(vals) * np.float32(1.0)), f"{kind} fwd, Q = {Q}"
        assert count == sum(int(c) for c in counts), f"{kind} fwd, Q = {Q}"
        if not has_step:
            continue
        for scale in SCALES:
            s_loss, s_count, s_vals, s_counts = call.run(kind, step=True, scale=scale)
            assert int(call.counter.item()) == 0, f"{kind} step, Q = {Q}: the ticket word was not re-armed"
            assert np.array_equal(s_vals.view(np.int32), vals.view(np.int32)) and np.array_equal(s_counts, counts)
            assert s_loss == bits_of(fixed_order_sum(s_vals) * np.float32(scale)), f"{kind} step, Q = {Q}, scale = {scale}"
            assert s_count == sum(int(c) for c in s_counts)
            if scale == 1.0:
                assert (s_loss, s_count) == (loss, count), f"{kind}, Q = {Q}: step and fwd disagree"


def test_a_window_without_queries_gives_plus_zero_and_no_count():
    call = Call((), [], [])
    for kind, (_, has_step) in KINDS.items():
        assert call.run(kind, step=False)[:2] == (0, 0), kind                # the bits of +0.0f, count 0
        if has_step:
            assert call.run(kind, step=True, scale=SCALES[1])[:2] == (0, 0), kind
            assert int(call.counter.item()) == 0
