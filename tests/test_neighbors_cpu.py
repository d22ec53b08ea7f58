"""Nearest-neighbour search without a GPU: the float64 oracle against hand-worked cases, the new symbols' declaration, export
and binding, every status code the header lists (all returned before any launch), and the Python argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from tests import neighbors_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rr_row_sqnorm_f32", "rr_knn_workspace_bytes", "rr_knn_f32", "rr_knn_geometry", "rr_knn_splits", "rr_knn_set_splits")
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -4, -5
P = C.c_void_p(4096)            # a non-null pointer that is never followed: every call below returns before a launch


# ---------------------------------------------------------------------------------------------- the oracle
def test_oracle_orders_ties_by_index():
    q = np.array([[0.0, 0.0]])
    b = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [-1.0, 0.0], [0.0, 0.0], [2.0, 0.0]])
    dist, idx, D = R.knn_ref(q, b, 4)
    assert D.tolist() == [[1.0, 1.0, 0.0, 1.0, 0.0, 4.0]]
    assert idx.tolist() == [[2, 4, 0, 1]]
    assert dist.tolist() == [[0.0, 0.0, 1.0, 1.0]]


def test_oracle_excludes_groups_and_nan_and_pads():
    q = np.array([[0.0], [10.0], [5.0]])
    b = np.array([[1.0], [2.0], [np.nan], [11.0]])
    dist, idx, _ = R.knn_ref(q, b, 3, q_group=[7, -1, 3], b_group=[7, 3, 3, -1])
    # row 0: bank 0 shares group 7, bank 2 is NaN; row 1: group -1 matches nothing (bank 3 also carries -1); row 2: group 3
    # removes bank 1 (and the NaN row)
    assert idx.tolist() == [[1, 3, -1], [3, 1, 0], [0, 3, -1]]
    assert dist[0].tolist() == [4.0, 121.0, np.inf]
    assert dist[1].tolist() == [1.0, 64.0, 81.0]
    assert dist[2].tolist() == [16.0, 36.0, np.inf]


def test_oracle_with_fewer_rows_than_k_and_none():
    q = np.array([[1.0, 2.0]])
    dist, idx, _ = R.knn_ref(q, np.array([[1.0, 4.0]]), 3)
    assert idx.tolist() == [[0, -1, -1]] and dist.tolist() == [[4.0, np.inf, np.inf]]
    dist, idx, _ = R.knn_ref(q, np.zeros((0, 2)), 2)
    assert idx.tolist() == [[-1, -1]] and dist.tolist() == [[np.inf, np.inf]]


def test_oracle_infinite_distance_sorts_before_the_padding():
    D = np.array([[np.inf, 3.0, 1.0]])
    dist, idx = R.knn_from_distances(D, 4)
    assert idx.tolist() == [[2, 1, 0, -1]] and dist.tolist() == [[1.0, 3.0, np.inf, np.inf]]


def test_bound_and_latent_distance_by_hand():
    q, b = np.array([[3.0, 4.0]]), np.array([[0.0, 0.0], [1.0, 0.0]])
    assert np.allclose(R.tol(q, b), 2 * 5 * 2.0 ** -24 * np.array([[25.0, 26.0]]), rtol=0, atol=0)
    ld = R.latent_distance_ref(np.array([[4.0, 9.0, np.inf], [np.inf] * 3]), np.array([[0, 1, -1], [-1] * 3]))
    assert ld.tolist() == [2.5, np.inf]


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
    assert "#define RR_KNN_MAX_K 64" in hdr


def test_geometry_reports_the_compiled_limits():
    from reactranker_amd import neighbors as N
    row_tile, bank_tile, max_k = N.geometry()
    assert max_k == 64 == N.MAX_K == _lib.RR_KNN_MAX_K
    assert row_tile >= 16 and row_tile % 16 == 0 and bank_tile >= 16 and bank_tile % 16 == 0
    _lib.lib().rr_knn_geometry(None, None, None)           # null slots are skipped


def _knn(q=P, ld_q=8, M=4, bank=P, ld_b=8, N=100, H=8, k=3, qg=None, bg=None, bn=None, dist=P, idx=P, ws=P, ws_bytes=1 << 30):
    return _lib.lib().rr_knn_f32(q, ld_q, M, bank, ld_b, N, H, k, qg, bg, bn, dist, idx, ws, C.c_size_t(ws_bytes), None)


def test_status_codes_come_back_before_any_launch():
    l = _lib.lib()
    for name in ("q", "bank", "dist", "idx", "ws"):
        assert _knn(**{name: None}) == ARG, name
    assert _knn(qg=P) == ARG and _knn(bg=P) == ARG                         # one group array without the other
    assert _knn(M=-1) == ARG and _knn(N=-1) == ARG
    assert _knn(H=0) == ARG and _knn(k=0) == ARG and _knn(k=-3) == ARG
    assert _knn(ld_q=7) == ARG and _knn(ld_b=7) == ARG                     # a pitch below H
    assert _knn(k=65) == UNSUPPORTED
    assert _knn(N=1 << 31) == UNSUPPORTED
    need = C.c_size_t()
    assert l.rr_knn_workspace_bytes(4, 100, 3, C.byref(need)) == OK and need.value >= 4 * 4 + 100 * 4
    assert _knn(ws_bytes=need.value - 1) == WORKSPACE
    assert _knn(ws_bytes=0) == WORKSPACE
    assert _knn(M=0, ws_bytes=need.value) == OK                            # no rows: nothing is launched
    # the sizing call itself
    assert l.rr_knn_workspace_bytes(4, 100, 3, None) == ARG
    assert l.rr_knn_workspace_bytes(-1, 100, 3, C.byref(need)) == ARG
    assert l.rr_knn_workspace_bytes(4, -1, 3, C.byref(need)) == ARG
    assert l.rr_knn_workspace_bytes(4, 100, 0, C.byref(need)) == ARG
    assert l.rr_knn_workspace_bytes(4, 100, 65, C.byref(need)) == UNSUPPORTED
    assert l.rr_knn_workspace_bytes(0, 0, 1, C.byref(need)) == OK and need.value > 0
    # the norms
    assert l.rr_row_sqnorm_f32(None, 8, 4, 8, P, None) == ARG and l.rr_row_sqnorm_f32(P, 8, 4, 8, None, None) == ARG
    assert l.rr_row_sqnorm_f32(P, 8, -1, 8, P, None) == ARG and l.rr_row_sqnorm_f32(P, 8, 4, 0, P, None) == ARG
    assert l.rr_row_sqnorm_f32(P, 7, 4, 8, P, None) == ARG
    assert l.rr_row_sqnorm_f32(P, 8, 0, 8, P, None) == OK


def test_workspace_grows_with_the_split_count_and_the_setting_is_checked():
    l = _lib.lib()
    assert l.rr_knn_splits() == 0
    one, seven = C.c_size_t(), C.c_size_t()
    try:
        assert l.rr_knn_set_splits(1) == OK and l.rr_knn_splits() == 1
        assert l.rr_knn_workspace_bytes(100, 5000, 64, C.byref(one)) == OK
        assert l.rr_knn_set_splits(7) == OK
        assert l.rr_knn_workspace_bytes(100, 5000, 64, C.byref(seven)) == OK
        assert seven.value >= one.value + 100 * 7 * 64 * 8                 # the per-split lists [M, S, k], distance and index
        assert _knn(M=100, N=5000, k=64, ws_bytes=one.value) == WORKSPACE
        assert l.rr_knn_set_splits(-1) == ARG and l.rr_knn_set_splits(1 << 20) == ARG and l.rr_knn_splits() == 7
    finally:
        assert l.rr_knn_set_splits(0) == OK
    assert l.rr_knn_splits() == 0


# ---------------------------------------------------------------------------------------------- the Python layer
def test_python_argument_checks_raise_before_any_launch():
    from reactranker_amd import neighbors as N
    q, b = torch.zeros(3, 5), torch.zeros(7, 5)
    with pytest.raises(ValueError, match="GPU"):
        N.knn(q, b, 2)                                                       # CPU tensors
    for k in (0, -1, 65, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            N.knn(q, b, k)
    with pytest.raises(ValueError, match="width"):
        N.knn(q, torch.zeros(7, 6), 2)
    with pytest.raises(ValueError, match="width"):
        N.knn(torch.zeros(3, 0), torch.zeros(7, 0), 2)
    with pytest.raises(ValueError, match="matrix"):
        N.knn(torch.zeros(5), b, 2)
    with pytest.raises(ValueError, match="float32"):
        N.knn(q.double(), b, 2)
    with pytest.raises(ValueError, match="go together"):
        N.knn(q, b, 2, q_group=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="metric"):
        N.knn(q, b, 2, metric="manhattan")
    with pytest.raises(ValueError, match="GPU"):
        N.row_sqnorm(q)
