"""Host side of the stream contract: functions._WorkspacePool's per-stream policy on fake (CPU) tensors, in the manner of
tests/test_poison_cpu.py's pool tests, and the pure host logic of the delayed-producer harness (tests/streams.py)."""
import pytest
import torch

from reactranker_amd import functions as Fn
from tests import streams as S
from tests.streams import Case


@pytest.fixture
def pool(monkeypatch):
    """an empty pool whose 'current stream' is whatever the test sets in `pool.now`"""
    monkeypatch.setattr(Fn._WorkspacePool, "free", [])
    monkeypatch.setattr(Fn._WorkspacePool, "allocs", 0)
    state = {"now": 0xA}
    monkeypatch.setattr(Fn._WorkspacePool, "stream_key", staticmethod(lambda device: state["now"]))
    monkeypatch.setattr(Fn._WorkspacePool, "now", state, raising=False)
    return Fn._WorkspacePool


CPU = torch.device("cpu")
A, B, C_ = 0xA, 0xB, 0xC


def _buf(n):
    return torch.zeros(n, dtype=torch.uint8)


def test_stream_key_of_a_device_without_streams_is_zero():
    assert Fn._WorkspacePool.stream_key(CPU) == 0 and Fn._WorkspacePool.stream_key(torch.device("meta")) == 0
    assert Fn._WorkspacePool.stream_key("cpu") == 0


def test_a_buffer_given_under_one_stream_is_not_handed_to_another_and_is_handed_to_the_next_take_of_its_own(pool):
    t = pool.take(1000, CPU)                                       # stream A
    assert pool.allocs == 1
    pool.give(t)
    assert t._rr_stream == A and pool.free == [t]
    pool.now["now"] = B
    u = pool.take(1000, CPU)
    assert u is not t and pool.allocs == 2                        # B allocates its own ...
    assert pool.free == [t]                                        # ... and a miss under B leaves A's buffer alone
    pool.give(u)
    assert u._rr_stream == B
    pool.now["now"] = A
    assert pool.take(900, CPU) is t and pool.free == [u] and pool.allocs == 2
    pool.now["now"] = B
    assert pool.take(900, CPU) is u and pool.free == [] and pool.allocs == 2


def test_the_give_records_the_stream_current_at_the_give(pool):
    t = pool.take(100, CPU)
    pool.now["now"] = B
    pool.give(t)                                                   # (a backward that ran under another stream than its forward)
    pool.now["now"] = A
    assert pool.take(100, CPU) is not t
    pool.now["now"] = B
    assert pool.take(100, CPU) is t


def test_best_fit_and_the_drop_on_a_too_large_request_look_at_the_own_stream_only(pool):
    a_small, a_big, b_mid = _buf(2000), _buf(5000), _buf(3000)
    pool.give(a_small)
    pool.give(a_big)
    pool.now["now"] = B
    pool.give(b_mid)
    pool.now["now"] = A
    assert pool.take(2500, CPU) is a_big                           # 3000 would fit better but is B's
    pool.give(a_big)
    t = pool.take(100000, CPU)                                     # nothing of A's is large enough: A's go, B's stays
    assert t.numel() == int(1.25 * 100000) + 4096 and pool.allocs == 1
    assert pool.free == [b_mid]


def test_the_cap_of_four_evicts_the_oldest_buffer_of_another_stream_and_never_one_of_the_own(pool):
    mine = [_buf(10 + i) for i in range(6)]
    for t in mine:
        pool.give(t)
    assert len(pool.free) == 4 and all(x is y for x, y in zip(pool.free, mine[:4]))     # as before: a full pool drops the newcomer
    pool.now["now"] = B
    theirs = [_buf(20 + i) for i in range(5)]
    for t in theirs[:4]:
        pool.give(t)                                               # each evicts the oldest of A's
    assert all(x is y for x, y in zip(pool.free, theirs[:4]))
    pool.give(theirs[4])                                           # only B's left: dropped
    assert len(pool.free) == 4 and all(x is y for x, y in zip(pool.free, theirs[:4]))
    pool.now["now"] = C_
    c = _buf(30)
    pool.give(c)
    assert len(pool.free) == 4 and pool.free[-1] is c and pool.free[0] is theirs[1]


def _parent_allocs(sequence):
    """allocations of the pool as it was before it knew about streams (one free list), for a take / give sequence"""
    free, allocs, held = [], 0, {}
    for op, tag, n in sequence:
        if op == "take":
            fit = [t for t in free if t >= n]
            if fit:
                held[tag] = min(fit)
                free.remove(held[tag])
            else:
                free, allocs = [], allocs + 1
                held[tag] = int(n * 1.25) + 4096
        elif len(free) < 4:
            free.append(held.pop(tag))
    return allocs


def test_a_one_stream_sequence_allocates_exactly_as_often_as_before(pool):
    """bench.py reads `allocs` around its timed region and expects none inside it"""
    seq = [("take", 0, 1000), ("give", 0, 0), ("take", 1, 1040), ("give", 1, 0), ("take", 2, 900), ("take", 3, 950), ("give", 2, 0),
           ("give", 3, 0), ("take", 4, 5346), ("give", 4, 0), ("take", 5, 5347), ("give", 5, 0), ("take", 6, 1000), ("give", 6, 0)]
    held = {}
    for op, tag, n in seq:
        if op == "take":
            held[tag] = pool.take(n, CPU)
        else:
            pool.give(held.pop(tag))
    assert pool.allocs == _parent_allocs(seq) == 3
    steady = pool.allocs
    for n in (1000, 1010, 990, 1020):                              # an epoch's steps differ by a few per cent: no new buffer
        pool.give(pool.take(n, CPU))
    assert pool.allocs == steady


# ---------------------------------------------------------------------------------------------- tests/streams.py, host logic
def test_delay_rule():
    assert S.delay_ms(0.0) == 20.0 and S.delay_ms(3.9) == 20.0     # never below 20 ms
    assert S.delay_ms(4.0) == 20.0 and S.delay_ms(6.0) == 30.0     # five times the enqueue time
    assert S.delay_ms(20.0) == 100.0 and S.delay_ms(1e6) == 100.0  # clamped: no spin above 100 ms
    assert (S.MIN_DELAY_MS, S.MAX_DELAY_MS, S.DELAY_FACTOR) == (20.0, 100.0, 5.0)


def test_spin_refuses_a_delay_above_the_cap():
    with pytest.raises(AssertionError):
        S.spin(None, 100.5)
    with pytest.raises(AssertionError):
        S.spin(None, 0.0)


def test_exemption_cap_of_a_case_table():
    ok = [Case(f"c{i}", None) for i in range(7)] + [Case("x", None, True, "returns Python numbers")]
    S.check_table("ok", ok)                                        # one in eight
    with pytest.raises(AssertionError, match="at most one in 8"):
        S.check_table("seven", ok[1:])                             # one in seven
    with pytest.raises(AssertionError, match="at most one in 8"):
        S.check_table("two", ok + [Case("y", None, True, "blocks")])
    with pytest.raises(AssertionError, match="no reason"):
        S.check_table("silent", ok[:7] + [Case("x", None, True, " ")])
    with pytest.raises(AssertionError, match="duplicate"):
        S.check_table("twice", ok[:7] + [Case("c0", None)])
    S.check_table("sixteen", ok + [Case(f"d{i}", None) for i in range(7)] + [Case("z", None, True, "blocks")])   # two in sixteen


def test_the_gpu_files_case_tables_respect_the_cap_and_name_their_exemptions():
    from tests.test_gpu_streams import SECTIONS
    assert set(SECTIONS) == {"A", "B", "C", "D"}
    for name, cases in SECTIONS.items():
        S.check_table(name, cases)
        assert len(cases) >= 8
    exempt = [(k, c.name) for k, cases in SECTIONS.items() for c in cases if c.host_sync]
    assert exempt == [("C", "probabilistic_calibration")]


def test_flatten_and_decoys():
    t = torch.arange(6.0)
    out = {"a": t, "b": [t[:2], None, (t[2:],)], "c": None}
    assert [k for k, _ in S.flatten(out)] == ["out.a", "out.b[0]", "out.b[2][0]"]
    with pytest.raises(TypeError):
        S.flatten({"a": 3.0})
    g = torch.Generator().manual_seed(0)
    m = torch.stack([torch.randn(50, generator=g), torch.rand(50, generator=g) + 0.5], 1)     # (mean, variance) columns
    d = S.decoy_of(m)
    assert d.shape == m.shape and not torch.equal(d, m) and bool(torch.isfinite(d).all())
    assert float(d[:, 1].min()) >= float(m[:, 1].min()) and float(d[:, 1].max()) <= float(m[:, 1].max())   # column by column
    v = torch.rand(9, generator=g)
    dv = S.decoy_of(v)
    assert float(dv.min()) >= float(v.min()) and float(dv.max()) <= float(v.max()) and not torch.equal(dv, v)
    assert torch.equal(S.decoy_of(torch.tensor([3.0])), torch.tensor([1.5]))
    with pytest.raises(AssertionError):
        S.decoy_of(torch.zeros(5))                                 # a constant tensor cannot be staged
    nan = torch.tensor([float("nan"), 1.0])
    assert S.same_bits(nan, nan.clone()) and not S.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not S.same_bits(torch.zeros(2), torch.zeros(3))
