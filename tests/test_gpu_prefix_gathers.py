"""The shared-prefix gathers (rr_gather2_sum_dropmask_f32, rr_gather_sum_dropsrc_f32) against (i) the numpy composition of
tests/prefix_gathers_ref.py and (ii) the existing entry points run one after the other on the same inputs - bit for bit
(gather_ref.same_bits: int32 views, signs of zero included).

Only the padding row of the two-level sum is a tree (padrow_sum over the partial rows): the numpy composition takes that one
row from the existing launch (rr_gather_sum_epi_f32), everything downstream of it is restated.

The second accumulator the issue made optional (the sum of the per-copy layers' dZ over the same table walk) is not built, so
it has no cases here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from reactranker_amd import functions as Fn
from reactranker_amd._lib import check, lib, ptr, stream
from tests import gather_ref as R
from tests import poison
from tests import prefix_gathers_ref as P
from tests import streams as S

pytestmark = pytest.mark.gpu
F32 = np.float32
N_SRC = 1031


def dev(a):
    return torch.as_tensor(a).cuda()


def _r4(n):
    return (n + 3) // 4 * 4


@functools.lru_cache(maxsize=8)
def _values(n, H, seed):
    """[n, H] normal values with 1 % negative zeros, exact zeros and rows 7 and 11 (where they exist) all -0.0"""
    rng = np.random.default_rng(7000 + 31 * seed + H)
    v = rng.standard_normal((n, H)).astype(F32)
    v[rng.random((n, H)) < 0.01] = -0.0
    v[rng.random((n, H)) < 0.01] = 0.0
    if n > 11:
        v[7] = v[11] = -0.0
    return v


def _table(rows, K, hi, seed, lo=-1, floor=0):
    """[rows, K] entries in [lo, hi), never in [0, floor) (floor = 1 keeps row 0 out); row 2 all pad, row 3 names rows of -0.0 only,
    row 4 pads followed by one entry"""
    rng = np.random.default_rng(seed)
    t = rng.integers(lo, hi, size=(rows, K)).astype(np.int32)
    t[(t >= 0) & (t < floor)] = floor
    if rows > 2:
        t[2] = -1
    if rows > 3 and hi > 11:
        t[3] = 7
    if rows > 4:
        t[4] = -1
        t[4, -1] = min(11, hi - 1)
    return t


def _bits(got, ref, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    if not R.same_bits(got, ref):
        bad = np.argwhere(np.ascontiguousarray(got, F32).view(np.int32) != np.ascontiguousarray(ref, F32).view(np.int32))
        r, c = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ref.size} elements differ in bits; first at row {r} column {c}: "
                             f"got {got[r, c]!r}, reference {ref[r, c]!r}; rows affected {np.unique(bad[:, 0])[:8]}")


def _mid(src, in_idx, H, part):
    """the intermediate as the step plan's launch stores it: rr_gather_sum_epi_f32 without a mask or addends"""
    n_mid, Ki = in_idx.shape
    out = torch.empty(n_mid, H, dtype=torch.float32, device="cuda")
    E = _lib.GatherEpi()
    E.mask_scale = 1.0
    check(lib().rr_gather_sum_epi_f32(ptr(src), src.shape[0], src.stride(0), ptr(in_idx), n_mid, Ki, H, ptr(part),
                                      0 if part is None else part.shape[0], 0 if part is None else part.stride(0), C.byref(E),
                                      ptr(out), H, stream()), "rr_gather_sum_epi_f32")
    return out


def _a_inputs(n_mid, n_out, Ki, Ko, H, seed, n_partial=None, n_src=N_SRC):
    src = _values(n_src, H, seed)
    in_idx = _table(n_mid, Ki, n_src, 100 + seed)
    # with partials, intermediate row 0 is the padding row: named by output row 0 only, in first position (the precondition)
    out_idx = _table(n_out, Ko, n_mid, 200 + seed, floor=1 if n_partial is not None else 0)
    part = None
    if n_partial is not None:
        out_idx[0, 0] = 0
        part = np.random.default_rng(300 + seed).standard_normal((n_partial, _r4(H))).astype(F32)
    y = _values(n_out, H, seed + 1).copy()
    return src, in_idx, out_idx, y, part


def _check_a(n_mid, n_out, Ki, Ko, H, p, seed=1, n_partial=None, scale=None, n_src=N_SRC, what=""):
    src, in_idx, out_idx, y, part = _a_inputs(n_mid, n_out, Ki, Ko, H, seed, n_partial, n_src)
    scale = float(R.keep_scale(p)) if scale is None else scale
    d_src, d_in, d_out, d_y = dev(src), dev(in_idx), dev(out_idx), dev(y)
    d_part = None if part is None else dev(part)
    got = Fn.gather2_sum_dropmask(d_src, d_in, d_y, scale, d_out, H, p, 77 + seed, row0_partial=d_part)
    mid = _mid(d_src, d_in, H, d_part)
    seq = Fn.gather_sum_dropmask(mid, d_y, scale, d_out, H, p, 77 + seed)
    torch.cuda.synchronize()
    name = f"rr_gather2_sum_dropmask_f32 {what} n_out={n_out} Ki={Ki} Ko={Ko} H={H} p={p} partials={n_partial}"
    _bits(got, seq.cpu().numpy(), name + " against the two launches")
    row0 = None if part is None else mid[0].cpu().numpy()
    _bits(got, P.gather2_sum_dropmask(src, in_idx, y, scale, out_idx, H, p, 77 + seed, row0=row0), name + " against numpy")
    return got


@pytest.mark.parametrize("Ki", [1, 2, 3, 4, 5, 9])
def test_two_level_sum_inner_and_outer_widths(Ki):
    """inner widths on the unrolled form (1..4) and the run-time loop (5, 9); outer widths in whole groups of 8 and remainders"""
    for Ko in (1, 3, 8, 9, 64, 65):
        _check_a(211, 37, Ki, Ko, 32, 0.1, seed=Ki + Ko)


@pytest.mark.parametrize("H", [4, 8, 300])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_two_level_sum_widths_and_dropout(H, p):
    _check_a(151, 29, 3, 11, H, p, seed=3)
    _check_a(151, 29, 3, 11, H, p, seed=4, scale=-1.5)               # a negative scale: products that are -0.0


def test_two_level_sum_index_edge_cases_are_in_the_inputs():
    src, in_idx, out_idx, y, _ = _a_inputs(211, 37, 3, 9, 32, 5)
    assert (in_idx < 0).any() and (out_idx < 0).any() and (out_idx[2] < 0).all() and (in_idx[2] < 0).all()
    assert (y == 0).any() and (y < 0).any() and np.signbit(src[7]).all() and (in_idx[3] == 7).all()
    got = _check_a(211, 37, 3, 9, 32, 0.1, seed=5).cpu().numpy()
    assert not np.signbit(got[2]).any() and (got[2] == 0).all()      # an all-negative outer row: +0.0


@pytest.mark.parametrize("n_partial", [None, 1, 3, 257, 513])
def test_two_level_sum_padding_row(n_partial):
    for Ki, Ko, H in ((3, 9, 300), (1, 1, 32), (5, 4, 8)):
        _check_a(97, 41, Ki, Ko, H, 0.1, seed=6, n_partial=n_partial)


GEOMS = {"one_wg": (32, 30), "xcd": (300, 54), "plain": (300, 977), "capped": (300, 28001)}


def _geometry(name):
    H, n_out = GEOMS[name]
    g = R.geometry(n_out, H)
    if name == "one_wg":
        assert g["one_workgroup"]
    elif name == "xcd":
        assert g["xcd"] and not g["capped"] and g["blocks"] > 1
    elif name == "plain":
        assert not g["xcd"] and not g["capped"] and g["blocks"] > 1
    else:
        assert g["capped"] and g["passes"] >= 2 and n_out * H * 4 < 40e6, g
    return H, n_out


@pytest.mark.parametrize("name", list(GEOMS))
def test_two_level_sum_grid_geometry(name):
    H, n_out = _geometry(name)
    Ko = 1 if name == "capped" else 5
    _check_a(n_out + 13, n_out, 3, Ko, H, 0.1, seed=8, what=name)
    _check_a(n_out + 13, n_out, 3, Ko, H, 0.1, seed=9, n_partial=3, what=name)


# ------------------------------------------------------------------------------------------------ the forward gather
def _b_inputs(n_y, n_map, n_out, K, H, seed):
    y = _values(n_y, H, seed)
    rng = np.random.default_rng(400 + seed)
    cmap = rng.integers(0, n_y, size=n_map).astype(np.int32)         # repeats: n_map > n_y
    cmap[0] = 0
    cmap[1] = 0
    if n_map > 12:
        cmap[5] = -1                                                 # a copy of nothing: the zero row
        cmap[7] = cmap[11] = min(7, n_y - 1)
    idx = _table(n_out, K, n_map, 500 + seed)
    idx[0, 0] = 0                                                    # row 0 is an ordinary row
    return y, cmap, idx


def _check_b(n_y, n_map, n_out, K, H, p, seed=1, what=""):
    y, cmap, idx = _b_inputs(n_y, n_map, n_out, K, H, seed)
    d_y, d_map, d_idx = dev(y), dev(cmap), dev(idx)
    got = Fn.gather_sum_dropsrc(d_y, d_map, d_idx, H, p, 55 + seed)
    seq = Fn.gather_sum(Fn.gather_dropout(d_y, d_map, H, p, 55 + seed), d_idx, H)
    torch.cuda.synchronize()
    name = f"rr_gather_sum_dropsrc_f32 {what} n_out={n_out} K={K} H={H} p={p}"
    _bits(got, seq.cpu().numpy(), name + " against the two launches")
    _bits(got, P.gather_sum_dropsrc(y, cmap, idx, H, p, 55 + seed), name + " against numpy")
    return got


@pytest.mark.parametrize("K", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("H", [4, 8, 300])
def test_dropped_source_sum_widths_and_dropout(K, H):
    for p in (0.0, 0.1, 0.5):
        _check_b(61, 409, 83, K, H, p, seed=K)


@pytest.mark.parametrize("name", list(GEOMS))
def test_dropped_source_sum_grid_geometry(name):
    H, n_out = _geometry(name)
    for K in ((4,) if name == "capped" else (4, 6)):                 # (the capped case once: its numpy reference hashes 17M elements)
        _check_b(257, 2 * n_out + 5, n_out, K, H, 0.1, seed=12, what=name)


def test_the_seed_changes_both_results():
    src, in_idx, out_idx, y, _ = _a_inputs(211, 37, 3, 9, 32, 2)
    a = [Fn.gather2_sum_dropmask(dev(src), dev(in_idx), dev(y), 1.25, dev(out_idx), 32, 0.5, s) for s in (1, 2)]
    assert not torch.equal(a[0], a[1])
    yb, cmap, idx = _b_inputs(61, 409, 83, 3, 32, 2)
    b = [Fn.gather_sum_dropsrc(dev(yb), dev(cmap), dev(idx), 32, 0.5, s) for s in (1, 2)]
    assert not torch.equal(b[0], b[1])


# ------------------------------------------------------------------------------------------------ stream contract, poison
def _stream_cases():
    def two_level():
        src, in_idx, out_idx, y, part = _a_inputs(977 + 13, 977, 3, 9, 300, 21, n_partial=3)
        t = [dev(src), dev(y), dev(part)]
        d_in, d_out = dev(in_idx), dev(out_idx)
        return t, lambda t: Fn.gather2_sum_dropmask(t[0], d_in, t[1], 1.25, d_out, 300, 0.1, 9, row0_partial=t[2])

    def dropped_source():
        y, cmap, idx = _b_inputs(257, 1959, 977, 4, 300, 22)
        d_map, d_idx = dev(cmap), dev(idx)
        return [dev(y)], lambda t: Fn.gather_sum_dropsrc(t[0], d_map, d_idx, 300, 0.1, 9)

    return [S.Case("gather2_sum_dropmask", two_level), S.Case("gather_sum_dropsrc", dropped_source)]


@pytest.mark.parametrize("case", _stream_cases(), ids=lambda c: c.name)
def test_both_entries_run_on_the_callers_stream(case):
    assert S.staged(case).status == "armed"


def _pitched_call(H, n_out, call):
    """call(out view) on a [n_out, H + 4] buffer from torch.empty (poisoned under a fill): -> the payload; the pad columns must
    hold afterwards what they held before"""
    buf = torch.empty(n_out, H + 4, dtype=torch.float32, device="cuda")
    before = buf[:, H:].clone()
    call(buf[:, :H])
    torch.cuda.synchronize()
    assert S.same_bits(buf[:, H:].clone(), before), "pad columns of a pitched `out` were written"
    return buf[:, :H]


@pytest.mark.parametrize("n_partial", [None, 3])
def test_two_level_sum_does_not_depend_on_what_memory_held(n_partial):
    src, in_idx, out_idx, y, part = _a_inputs(211, 97, 3, 9, 300, 31, n_partial=n_partial)
    d = [dev(src), dev(in_idx), dev(y), dev(out_idx), None if part is None else dev(part)]

    def fn():
        dense = Fn.gather2_sum_dropmask(d[0], d[1], d[2], 1.25, d[3], 300, 0.1, 9, row0_partial=d[4])
        pitched = _pitched_call(300, 97, lambda o: Fn.gather2_sum_dropmask(d[0], d[1], d[2], 1.25, d[3], 300, 0.1, 9, row0_partial=d[4],
                                                                           out=o))
        return dense, pitched

    report, counters, last = poison.fill_dependence(fn, sync=torch.cuda.synchronize)
    assert not report, report
    assert counters[0xFF].buffers >= 2                               # (both outputs came from poisoned allocations)
    assert torch.equal(last[0], last[1]) and bool(torch.isfinite(last[0]).all())   # every element of out is written


def test_dropped_source_sum_does_not_depend_on_what_memory_held():
    y, cmap, idx = _b_inputs(61, 409, 97, 4, 300, 32)
    d = [dev(y), dev(cmap), dev(idx)]

    def fn():
        dense = Fn.gather_sum_dropsrc(d[0], d[1], d[2], 300, 0.1, 9)
        pitched = _pitched_call(300, 97, lambda o: Fn.gather_sum_dropsrc(d[0], d[1], d[2], 300, 0.1, 9, out=o))
        return dense, pitched

    report, counters, last = poison.fill_dependence(fn, sync=torch.cuda.synchronize)
    assert not report, report
    assert counters[0xFF].buffers >= 2
    assert torch.equal(last[0], last[1]) and bool(torch.isfinite(last[0]).all())
