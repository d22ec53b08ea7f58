"""Greedy k-center selection without a GPU: the numpy oracle against hand-worked cases and against itself (f32 chain == float64
on integer inputs), the new symbols' declaration, export and binding, every status code the header lists (all returned before
any launch), and the Python argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from tests import selection_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rr_kcenter_workspace_bytes", "rr_kcenter_f32", "rr_kcenter_blocks", "rr_kcenter_set_blocks")
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -4, -5
PTR = C.c_void_p(4096)          # a non-null pointer that is never followed: every call below returns before a launch
INF = np.inf


# ---------------------------------------------------------------------------------------------- the oracle
X6 = np.array([[0.0], [10.0], [4.0], [10.0], [7.0], [-2.0]])


@pytest.mark.parametrize("greedy", [S.greedy64, S.greedy32], ids=["f64", "f32"])
def test_oracle_on_a_hand_worked_example_with_a_tie(greedy):
    # round 0: every score is +inf, the index decides -> row 0; round 1: rows 1 and 3 both at 100 -> row 1 (row 3, its twin,
    # drops to 0 and is taken last); round 2: row 2 at 16 (row 4 stays at 9: 9 < 9 is false); then rows 4, 5, the twin, padding
    r = greedy(X6, 7)
    assert r["picks"].tolist() == [0, 1, 2, 4, 5, 3, -1]
    assert r["gain"].tolist() == [INF, 100.0, 16.0, 9.0, 4.0, 0.0, -1.0]
    assert r["min_dist"].tolist() == [0.0] * 6
    assert r["assign"].tolist() == [0, 1, 2, 1, 3, 4]
    assert r["tied"].tolist() == [True, True, False, False, False, False, False]


@pytest.mark.parametrize("greedy", [S.greedy64, S.greedy32], ids=["f64", "f32"])
def test_oracle_with_weights_init_dist_and_ineligible_rows(greedy):
    # weight 0 keeps row 4 out of the picks but not out of the state; weight 5 lifts row 2 to 80
    r = greedy(X6, 6, weight=[1, 1, 5, 1, 0, 1])
    assert r["picks"].tolist() == [0, 1, 2, 5, 3, -1]
    assert r["gain"].tolist() == [INF, 100.0, 80.0, 4.0, 0.0, -1.0]
    assert r["min_dist"].tolist() == [0.0, 0.0, 0.0, 0.0, 9.0, 0.0]
    assert r["assign"].tolist() == [0, 1, 2, 1, 1, 3]
    # init_dist: row 5 starts farthest; a row with a NaN is NaN for good; negative, NaN and +inf weights are ineligible
    x = X6.copy()
    x[2] = np.nan
    r = greedy(x, 3, init_dist=[1, 1, 1, 1, 1, 30], weight=[-1, 1, 1, np.nan, INF, 1])
    assert r["picks"].tolist() == [5, 1, -1]
    assert r["gain"].tolist() == [30.0, 1.0, -1.0]
    assert np.array_equal(r["min_dist"], [1.0, 0.0, np.nan, 0.0, 1.0, 0.0], equal_nan=True)
    assert r["assign"].tolist() == [-1, 1, -1, 1, -1, 0]
    # no rows at all, and n == 0
    r = greedy(np.zeros((0, 3)), 2)
    assert r["picks"].tolist() == [-1, -1] and r["gain"].tolist() == [-1.0, -1.0] and r["min_dist"].shape == (0,)
    r = greedy(X6, 0, init_dist=[3] * 6)
    assert r["picks"].shape == (0,) and r["min_dist"].tolist() == [3.0] * 6 and r["assign"].tolist() == [-1] * 6


def test_chain32_by_hand_and_replay():
    # H = 6: group 0 (columns 0..3) on lane 0, group 1 (columns 4, 5) on lane 1; the butterfly adds lane 1 into lane 0 last
    x = np.array([[1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 0]], np.float32)
    assert S.chain32(x, 1).tolist() == [91.0, 0.0]
    a, b = np.float32(1.0), np.float32(2.0 ** -12)                    # b^2 = 2^-24, half an ulp of 1: each is rounded away
    one = np.array([[a, b, b, b], [0, 0, 0, 0]], np.float32)          # (to even) inside one chain ...
    assert S.chain32(one, 1)[0] == np.float32(1.0)
    two = np.zeros((2, 8), np.float32)                                # ... but in a chain of their own they sum to 1.5 ulp first
    two[0, 0], two[0, 4:7] = a, b
    assert S.chain32(two, 1)[0] == np.float32(1.0 + 2.0 ** -22)
    got, best = S.replay64(X6, [0, 3, 2])
    assert got.tolist() == [INF, 100.0, 16.0] and best.tolist() == [INF, 100.0, 16.0]
    assert S.gamma(29) == 2 ** -18


@pytest.mark.parametrize("H", [1, 3, 4, 30, 257, 300])
def test_greedy32_equals_greedy64_on_integer_inputs(H):
    rng = np.random.default_rng(H)
    P, n = 150, 24
    x = rng.integers(-3, 4, (P, H)).astype(np.float32)
    x[rng.integers(0, P, 8)] = x[rng.integers(0, P, 8)]
    for w, init in ((None, None), (rng.integers(1, 4, P).astype(np.float32), rng.integers(0, 40, P).astype(np.float32))):
        a, b = S.greedy64(x, n, init, w), S.greedy32(x, n, init, w)
        for key in ("picks", "gain", "min_dist", "assign", "tied"):
            assert np.array_equal(np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)), key
        assert H > 4 or a["tied"].any()


# ---------------------------------------------------------------------------------------------- the binding
def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "reactranker_hip.h")).read()
    declared = set(re.findall(r"\b(rr_[a-z0-9_]+)\s*\(", hdr))
    l = _lib.lib()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert getattr(l, s).argtypes is not None, s
    assert l.rr_version() == 8 == _lib.ABI_VERSION
    assert "#define RR_KCENTER_MAX_PICKS 65536" in hdr and _lib.RR_KCENTER_MAX_PICKS == 65536
    assert "kcenter.hip" in open(os.path.join(REPO, "reactranker_amd", "csrc", "Makefile")).read()


def _kc(x=PTR, ld=8, P=100, H=8, n=5, init=None, w=None, picks=PTR, gain=PTR, md=PTR, assign=PTR, ws=PTR, ws_bytes=1 << 30):
    return _lib.lib().rr_kcenter_f32(x, ld, P, H, n, init, w, picks, gain, md, assign, ws, C.c_size_t(ws_bytes), None)


def test_status_codes_come_back_before_any_launch():
    l = _lib.lib()
    for name in ("x", "picks", "gain", "md", "assign", "ws"):
        assert _kc(**{name: None}) == ARG, name
    assert _kc(P=-1) == ARG and _kc(n=-1) == ARG
    assert _kc(H=0) == ARG and _kc(H=-2) == ARG
    assert _kc(ld=7) == ARG                                                # a pitch below H
    assert _kc(n=65537) == UNSUPPORTED
    assert _kc(P=1 << 31) == UNSUPPORTED
    need = C.c_size_t()
    assert l.rr_kcenter_workspace_bytes(100, 5, C.byref(need)) == OK and need.value >= 100
    assert _kc(ws_bytes=need.value - 1) == WORKSPACE
    assert _kc(ws_bytes=0) == WORKSPACE
    assert _kc(P=0, n=0, ws_bytes=need.value) == OK                        # nothing to write: nothing is launched
    # the sizing call itself
    assert l.rr_kcenter_workspace_bytes(100, 5, None) == ARG
    assert l.rr_kcenter_workspace_bytes(-1, 5, C.byref(need)) == ARG
    assert l.rr_kcenter_workspace_bytes(100, -1, C.byref(need)) == ARG
    assert l.rr_kcenter_workspace_bytes(100, 65537, C.byref(need)) == UNSUPPORTED
    assert l.rr_kcenter_workspace_bytes(1 << 31, 5, C.byref(need)) == UNSUPPORTED
    assert l.rr_kcenter_workspace_bytes(0, 0, C.byref(need)) == OK and need.value > 0
    assert l.rr_kcenter_workspace_bytes((1 << 31) - 1, 65536, C.byref(need)) == OK and need.value >= (1 << 31) - 1


def test_the_blocks_setting_is_checked_and_does_not_move_the_workspace():
    l = _lib.lib()
    assert l.rr_kcenter_blocks() == 0
    a, b = C.c_size_t(), C.c_size_t()
    try:
        assert l.rr_kcenter_set_blocks(1) == OK and l.rr_kcenter_blocks() == 1
        assert l.rr_kcenter_workspace_bytes(5000, 64, C.byref(a)) == OK
        assert l.rr_kcenter_set_blocks(4096) == OK and l.rr_kcenter_blocks() == 4096
        assert l.rr_kcenter_workspace_bytes(5000, 64, C.byref(b)) == OK
        assert a.value == b.value >= 2 * 4096 * 8 + 5000                   # the pairs of two launches at the largest grid + a byte per row
        assert l.rr_kcenter_set_blocks(-1) == ARG and l.rr_kcenter_set_blocks(4097) == ARG and l.rr_kcenter_blocks() == 4096
    finally:
        assert l.rr_kcenter_set_blocks(0) == OK
    assert l.rr_kcenter_blocks() == 0


# ---------------------------------------------------------------------------------------------- the Python layer
def test_python_argument_checks_raise_before_any_launch():
    from reactranker_amd import neighbors as N
    x = torch.zeros(7, 5)
    with pytest.raises(ValueError, match="GPU"):
        N.kcenter_greedy(x, 2)                                               # CPU tensors
    for n in (-1, 65537, 2.5):
        with pytest.raises(ValueError, match="n must be"):
            N.kcenter_greedy(x, n)
    with pytest.raises(ValueError, match="width 0"):
        N.kcenter_greedy(torch.zeros(7, 0), 2)
    with pytest.raises(ValueError, match="matrix"):
        N.kcenter_greedy(torch.zeros(5), 2)
    with pytest.raises(ValueError, match="float32"):
        N.kcenter_greedy(x.double(), 2)
    assert N.MAX_PICKS == 65536 and N.KCENTER_ROWS_PER_WORKGROUP == 4
    # the per-row arrays are checked against the matrix (here on a device that needs no GPU to name)
    meta = torch.zeros(7, 5, device="meta")
    for bad in (torch.zeros(6, device="meta"), torch.zeros(7, device="meta", dtype=torch.float64), torch.zeros(7), [0.0] * 7):
        with pytest.raises(ValueError, match="init_dist"):
            N._per_row(bad, 7, meta.device, "init_dist")
        with pytest.raises(ValueError, match="weight"):
            N._per_row(bad, 7, meta.device, "weight")
    assert N._per_row(torch.zeros(7, device="meta"), 7, meta.device, "weight").shape == (7,)


def test_a_cpu_tensor_error_names_the_function_that_was_called():
    from reactranker_amd import neighbors as N
    x = torch.zeros(7, 5)
    with pytest.raises(ValueError, match=r"^kcenter_greedy: .*GPU"):
        N.kcenter_greedy(x, 2)
    with pytest.raises(ValueError, match=r"^row_sqnorm: .*GPU"):
        N.row_sqnorm(x)
