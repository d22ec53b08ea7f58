"""tests/poison.py itself, on CPU tensors: the fills, the restore, the counters, the comparison routine on a deliberately leaky
function - and the two facts about the package the GPU file (tests/test_gpu_poison.py) leans on: no module allocates
uninitialised memory through a name the helper does not patch, and functions._WorkspacePool hands out what its docstring says."""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch

from reactranker_amd import functions as Fn
from tests import poison

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reactranker_amd")

# the table of the issue: what each fill reads as, per dtype the package allocates (float32, float64, int32, int64, uint8)
F32 = {0x00: 0.0, 0x7F: np.frombuffer(b"\x7f" * 4, np.float32)[0], 0xFF: float("nan")}
F64 = {0x00: 0.0, 0x7F: np.frombuffer(b"\x7f" * 8, np.float64)[0], 0xFF: float("nan")}


def _originals():
    return torch.empty, torch.empty_like, torch.Tensor.new_empty, Fn._WorkspacePool.__dict__["take"]


def test_the_fill_values_are_the_ones_the_table_states():
    assert math.isfinite(F32[0x7F]) and abs(F32[0x7F] / 3.39e38 - 1) < 2e-3
    assert math.isfinite(F64[0x7F]) and abs(F64[0x7F] / 1.4e306 - 1) < 2e-2
    assert np.isnan(np.frombuffer(b"\xff" * 4, np.float32)[0]) and np.isnan(np.frombuffer(b"\xff" * 8, np.float64)[0])
    assert np.frombuffer(b"\x7f" * 4, np.int32)[0] == 2139062143 and np.frombuffer(b"\xff" * 4, np.int32)[0] == -1


@pytest.mark.parametrize("byte", poison.FILLS)
def test_every_dtype_the_package_allocates_gets_its_pattern(byte):
    with poison.poisoned(byte) as c:
        f = torch.empty(3, 5, dtype=torch.float32)
        d = torch.empty(7, dtype=torch.float64)
        i = torch.empty(9, dtype=torch.int32)
        l = torch.empty(1, dtype=torch.int64)
        u = torch.empty(11, 3, dtype=torch.uint8)
        b = torch.empty(4, dtype=torch.bool)
        like = torch.empty_like(f[:, :4], memory_format=torch.contiguous_format)
        new = d.new_empty(6)
        newi = i.new_empty((2, 2))
        dst = torch.zeros(4)
        same = torch.empty(4, out=dst)                       # out=: passes through, neither filled nor counted
        z = torch.zeros(5), torch.zeros_like(f)
    assert c.buffers == 9 and c.bytes == 60 + 56 + 36 + 8 + 33 + 4 + 48 + 48 + 16
    assert same is dst and float(dst.abs().max()) == 0.0
    assert all(float(t.abs().max()) == 0.0 for t in z)

    def same_as(t, v):
        return bool(torch.isnan(t).all()) if math.isnan(v) else bool((t == v).all())
    assert same_as(f, F32[byte]) and same_as(like, F32[byte]) and like.shape == (3, 4)
    assert same_as(d, F64[byte]) and same_as(new, F64[byte]) and new.dtype == torch.float64
    want = 0 if byte == 0 else 1                                   # integers: never a byte pattern (it could become an index)
    assert bool((i == want).all()) and bool((l == want).all()) and bool((newi == want).all()) and newi.dtype == torch.int32
    assert bool((u == byte).all()) and bool((b == bool(byte)).all())


def test_the_whole_storage_is_filled_not_only_the_elements_in_view():
    with poison.poisoned(0x7F):
        t = torch.empty(4, 8)[:, :5]                               # (what segment_mean_fwd does: a pitched output)
    raw = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage(), 0, (t.untyped_storage().nbytes(),))
    assert raw.numel() == 128 and bool((raw == 0x7F).all())


def test_all_four_names_come_back_also_after_an_exception():
    before = _originals()
    with poison.poisoned(0xFF):
        during = _originals()
        assert all(a is not b for a, b in zip(before, during))
    assert all(a is b for a, b in zip(before, _originals()))
    with pytest.raises(ZeroDivisionError):
        with poison.poisoned(0xFF):
            torch.empty(3)
            1 / 0
    assert all(a is b for a, b in zip(before, _originals()))
    assert isinstance(Fn._WorkspacePool.__dict__["take"], classmethod)


def test_nothing_is_installed_at_import():
    assert torch.empty.__module__ != poison.__name__ and getattr(torch.empty, "__name__", "") == "empty"
    assert Fn._WorkspacePool.take.__func__.__module__ == Fn.__name__


def test_the_pool_is_refilled_on_every_take_with_its_headroom_and_spared_ranges_are_left(monkeypatch):
    monkeypatch.setattr(Fn._WorkspacePool, "free", [])
    monkeypatch.setattr(Fn._WorkspacePool, "allocs", 0)
    cpu = torch.device("cpu")
    with poison.poisoned(0x7F, spare_pool=[(16, 32), (100, 104)]) as c:
        t = Fn._WorkspacePool.take(1000, cpu)
        assert t.numel() == 1250 + 4096 and c.buffers == 1 and c.takes == 1 and c.bytes == t.numel() - 20
        keep = torch.ones_like(t, dtype=torch.bool)
        keep[16:32] = keep[100:104] = False
        assert bool((t[keep] == 0x7F).all())                      # headroom included
        t.fill_(3)                                                 # "the previous step's activations"
        Fn._WorkspacePool.give(t)
        t2 = Fn._WorkspacePool.take(900, cpu)
        assert t2 is t and c.buffers == 2 and c.takes == 2
        assert bool((t2[keep] == 0x7F).all()) and bool((t2[~keep] == 3).all())
    assert Fn._WorkspacePool.allocs == 1


def test_spared_ranges_may_overlap_reach_past_the_storage_and_hold_for_integers_too():
    o = torch.empty
    t = torch.zeros(100, dtype=torch.uint8)
    assert poison.fill(o, t, 0x7F, [(10, 30), (20, 40), (90, 500), (-5, 2), (50, 50)]) == 100 - 30 - 10 - 2
    keep = torch.zeros(100, dtype=torch.bool)
    keep[0:2] = keep[10:40] = keep[90:] = True
    assert bool((t[keep] == 0).all()) and bool((t[~keep] == 0x7F).all())
    i = torch.full((10,), 7, dtype=torch.int32)
    assert poison.fill(o, i, 0xFF, [(6, 9), (30, 36)]) == 40 - 8 - 8     # elements 1, 2 (bytes 4..11) and 7, 8 (28..35) stay
    assert i.tolist() == [1, 7, 7, 1, 1, 1, 1, 7, 7, 1]
    f = torch.zeros(4, dtype=torch.float32)
    assert poison.fill(o, f, 0xFF, [(0, 16)]) == 0 and float(f.abs().max()) == 0.0


def test_counters_count():
    with poison.poisoned(0x00) as c:
        assert (c.buffers, c.bytes) == (0, 0)
        torch.empty(10)
        assert (c.buffers, c.bytes) == (1, 40)
        torch.empty_like(torch.zeros(2, 3, dtype=torch.float64))
        assert (c.buffers, c.bytes) == (2, 88)
        torch.empty(0)
        assert (c.buffers, c.bytes) == (3, 88)


def test_a_leaky_function_is_reported_and_a_clean_one_is_not():
    report, counters, last = poison.fill_dependence(lambda: torch.empty(8).sum())
    # the three fills sum to 0, inf and NaN: whatever the plain run's memory held, at most one of them can agree with it
    assert len(report) >= 2 and all(r.startswith("fill 0x") for r in report)
    assert all(counters[b].buffers == 1 and counters[b].bytes == 32 for b in poison.FILLS)
    assert bool(torch.isnan(last))

    def clean():
        out = torch.empty(8)
        out.copy_(torch.arange(8.0))
        part = torch.empty(5, dtype=torch.float64)               # scratch: written, then read
        part[:] = 2.0
        return {"out": out, "sum": float(part.sum()), "nested": [out[:3], None, (out.new_empty(0),)]}
    report, counters, _ = poison.fill_dependence(clean)
    assert report == [] and all(counters[b].buffers == 3 for b in poison.FILLS)

    # a stale word multiplied by zero: only the NaN fill sees it (the fills are compared with each other here, not with a
    # plain run: what recycled host memory holds is anybody's guess)
    snaps = {}
    for byte in poison.FILLS:
        with poison.poisoned(byte):
            snaps[byte] = poison.snapshot(torch.empty(4) * 0.0)
    assert poison.differences(snaps[0x00], snaps[0x7F]) == [] and poison.differences(snaps[0x00], snaps[0xFF])
    # ... an added one: the finite fill sees it as well
    for byte in poison.FILLS:
        with poison.poisoned(byte):
            snaps[byte] = poison.snapshot(torch.empty(4) + 1.0)
    assert poison.differences(snaps[0x00], snaps[0x7F]) and poison.differences(snaps[0x00], snaps[0xFF])
    # a legitimate NaN in the result is not a difference, -0.0 against 0.0 is
    assert poison.fill_dependence(lambda: torch.full((3,), float("nan")))[0] == []
    assert poison.differences(poison.snapshot(torch.tensor([0.0])), poison.snapshot(torch.tensor([-0.0])))
    # a sliced-off pad column is not part of the result
    assert poison.fill_dependence(lambda: torch.empty(4, 8)[:, :5].zero_())[0] == []


def test_the_package_allocates_uninitialised_memory_through_the_patched_names_only():
    """torch.empty / torch.empty_like / Tensor.new_empty are what poisoned() replaces; any other route to uninitialised
    memory in reactranker_amd/*.py would be invisible to tests/test_gpu_poison.py."""
    banned = re.compile(r"empty_strided|\bresize_\(|\bresize_as_\(|torch\.Tensor\(|torch\.(?:cuda\.)?(?:Float|Double|Half|Int|Long|Byte)Tensor\(|"
                        r"\.new\(|\bempty_quantized|\bempty_permuted|from torch import .*\bempty")
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) > 10
    hits, uses = [], 0
    for path in files:
        with open(path) as f:
            for no, line in enumerate(f, 1):
                code = line.split("#", 1)[0]
                if banned.search(code):
                    hits.append(f"{os.path.basename(path)}:{no}: {line.strip()}")
                uses += len(re.findall(r"torch\.empty(?:_like)?\(|\.new_empty\(", code))
    assert not hits, "\n".join(hits)
    assert uses >= 60                                              # the scan does see the allocations it is about


# ---------------------------------------------------------------------------------------------- functions._WorkspacePool
@pytest.fixture
def pool(monkeypatch):
    monkeypatch.setattr(Fn._WorkspacePool, "free", [])
    monkeypatch.setattr(Fn._WorkspacePool, "allocs", 0)
    return Fn._WorkspacePool


def _buf(n, device="cpu"):
    return torch.zeros(n, dtype=torch.uint8, device=device)


def test_pool_takes_the_best_fit_among_the_sufficient_buffers(pool):
    cpu = torch.device("cpu")
    a, b, c = _buf(5000), _buf(2000), _buf(3000)
    for t in (a, b, c):
        pool.give(t)
    assert pool.take(2500, cpu) is c                              # 2000 is too small, 3000 beats 5000
    assert pool.take(2000, cpu) is b                              # exactly enough is enough
    assert pool.take(1, cpu) is a
    assert pool.free == [] and pool.allocs == 0


def test_pool_ignores_buffers_of_another_device(pool):
    cpu = torch.device("cpu")
    other = _buf(1 << 20, device="meta")
    pool.give(other)
    t = pool.take(1000, cpu)
    assert t is not other and t.device == cpu and pool.allocs == 1
    assert pool.free == [other]                                    # and a miss on this device leaves the other device's alone


def test_pool_drops_this_devices_buffers_on_a_too_large_request_and_allocates_with_headroom(pool):
    cpu = torch.device("cpu")
    other = _buf(10, device="meta")
    for t in (_buf(100), other, _buf(200)):
        pool.give(t)
    t = pool.take(100000, cpu)
    assert t.numel() == int(1.25 * 100000) + 4096 and t.dtype == torch.uint8
    assert pool.free == [other] and pool.allocs == 1
    assert pool.take(1001, cpu).numel() == int(1.25 * 1001) + 4096 == 5347 and pool.allocs == 2


def test_pool_keeps_at_most_four_buffers(pool):
    bufs = [_buf(10 + i) for i in range(6)]
    for t in bufs:
        pool.give(t)
    assert len(pool.free) == 4 and all(x is y for x, y in zip(pool.free, bufs[:4]))


def test_pool_counts_only_real_allocations(pool):
    cpu = torch.device("cpu")
    t = pool.take(1000, cpu)
    assert pool.allocs == 1
    for n in (1000, 10, 5346):                                     # all fit the first buffer with its headroom
        pool.give(t)
        assert pool.take(n, cpu) is t
    assert pool.allocs == 1
    pool.give(t)
    assert pool.take(5347, cpu) is not t and pool.allocs == 2


def test_every_exclusion_of_the_gpu_file_quotes_a_sentence_of_the_header():
    """tests/test_gpu_poison.py may leave storage out of a comparison only where include/reactranker_hip.h calls it unspecified"""
    from tests.test_gpu_poison import EXCLUDED
    with open(os.path.join(os.path.dirname(PKG), "include", "reactranker_hip.h")) as f:
        text = " ".join(f.read().replace("*", " ").split())
    assert len(EXCLUDED) == 3
    for case, what, quote in EXCLUDED:
        sentence = " ".join(quote.split('"')[1].split())
        assert "unspecified" in sentence and sentence in text, case
