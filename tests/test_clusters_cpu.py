"""Sphere-exclusion clustering and cluster-held-out splits without a GPU: the numpy oracle against hand-worked cases and against
itself (f32 chain == float64 on integer inputs), the new symbols' declaration, export and binding, every status code the header
lists for rr_radius_count_f32 and rr_sphere_exclusion_f32 (all returned before any launch), the Python argument checks, and the
split rules of cluster_split / cluster_kfold, which run on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from reactranker_amd import clusters as K
from tests import cluster_ref as CR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rr_radius_count_workspace_bytes", "rr_radius_count_f32", "rr_sphere_exclusion_workspace_bytes",
           "rr_sphere_exclusion_f32", "rr_sphere_exclusion_blocks", "rr_sphere_exclusion_set_blocks")
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -4, -5
PTR = C.c_void_p(4096)          # a non-null pointer that is never followed: every call below returns before a launch
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------- the oracle
X7 = np.array([[0.0], [1.0], [2.0], [10.0], [11.0], [5.0], [1.0]])


@pytest.mark.parametrize("exclusion", [CR.exclusion64, CR.exclusion32], ids=["f64", "f32"])
def test_oracle_on_a_hand_worked_example(exclusion):
    # r2 = 1.5: rows within distance 1.  counts: row 0 -> {0, 1, 6}, row 1 -> {0, 1, 2, 6}, row 2 -> {1, 2, 6}, rows 3, 4 -> {3, 4},
    # row 5 -> {5}, row 6 = row 1
    key = CR.count64(X7, X7, 1.5)
    assert key.tolist() == [3, 4, 3, 2, 2, 1, 4]
    # Butina: rows 1 and 6 tie at 4 -> row 1 (index), takes 0, 1, 2, 6; then rows 3 and 4 tie at 2 -> row 3; then row 5
    r = exclusion(X7, 1.5, key)
    assert r["centres"].tolist() == [1, 3, 5] and r["labels"].tolist() == [0, 0, 0, 1, 1, 2, 0]
    assert r["by_index"].tolist() == [True, True, False]
    # the leader algorithm: index order.  Row 0 takes 0, 1, 6; row 2 - inside row 1's sphere, but row 1 is gone - is its own centre
    r = exclusion(X7, 1.5, None, 6)
    assert r["centres"].tolist() == [0, 2, 3, 5, -1, -1] and r["labels"].tolist() == [0, 0, 1, 2, 2, 3, 0]
    assert r["by_index"].tolist() == [True, True, True, False, False, False]
    # too few rounds leave rows at -1; a non-finite row is -2 for good; r2 = 0 joins exact duplicates only; r2 = inf: one cluster
    r = exclusion(X7, 1.5, key, 1)
    assert r["centres"].tolist() == [1] and r["labels"].tolist() == [0, 0, 0, -1, -1, -1, 0]
    x = X7.copy()
    x[2] = np.nan
    r = exclusion(x, 0.0, None)
    assert r["labels"].tolist() == [0, 1, -2, 2, 3, 4, 1] and r["centres"].tolist() == [0, 1, 3, 4, 5]
    r = exclusion(x, np.float32(np.inf), None, 2)
    assert r["labels"].tolist() == [0, 0, -2, 0, 0, 0, 0] and r["centres"].tolist() == [0, -1]
    r = exclusion(np.zeros((0, 3)), 1.0, None, 2)
    assert r["centres"].tolist() == [-1, -1] and r["labels"].shape == (0,)
    member_d, held = CR.replay64(X7, [1, 3, 5, -1], np.array([0, 0, 0, 1, 1, 2, 0]), key)
    assert member_d.tolist() == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0] and held.tolist() == [True] * 4
    assert CR.replay64(X7, [6, 3, 5], np.array([0, 0, 0, 1, 1, 2, 0]), key)[1].tolist() == [False, True, True]


def test_count64_excludes_groups_and_nan_and_counts_the_row_itself():
    x = X7.copy()
    x[5] = np.nan
    g = np.array([0, 0, 1, 2, -1, 3, -1])
    assert CR.count64(x, x, 1.5).tolist() == [3, 4, 3, 2, 2, 0, 4]
    assert CR.count64(x, x, 1.5, g, g).tolist() == [1, 2, 2, 1, 2, 0, 4]
    assert CR.count64(x, x[:0], 1.5).tolist() == [0] * 7 and CR.count64(x[:0], x, 1.5).shape == (0,)
    assert CR.r2_of(3.0) == np.float32(9.0) and CR.r2_of(np.inf) == np.float32(np.inf)
    assert CR.r2_of(0.1) == np.float32(np.float64(0.1) ** 2) != np.float32(0.1) ** 2


@pytest.mark.parametrize("H", [1, 3, 4, 30, 257, 300])
def test_exclusion32_equals_exclusion64_on_integer_inputs(H):
    rng = np.random.default_rng(H)
    P = 150
    x = rng.integers(-3, 4, (P, H)).astype(np.float32)
    x[rng.integers(0, P, 8)] = x[rng.integers(0, P, 8)]
    D = np.stack([CR.S.dist64(x, r) for r in range(P)])
    r2 = np.floor(np.quantile(D, 0.1)) + 0.5
    key = CR.count64(x, x, r2)
    tied = False
    for k in (key, None, rng.integers(0, 5, P)):
        a, b = CR.exclusion64(x, r2, k), CR.exclusion32(x, r2, k)
        for name in ("labels", "centres", "by_index"):
            assert np.array_equal(a[name], b[name]), name
        assert (a["labels"] >= 0).all() and len(a["centres"]) == a["labels"].max() + 1
        tied = tied or a["by_index"].any()
    assert tied


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
    assert "#define RR_SPHERE_EXCLUSION_MAX_ROUNDS 65536" in hdr and _lib.RR_SPHERE_EXCLUSION_MAX_ROUNDS == 65536 == K.MAX_ROUNDS
    mk = open(os.path.join(REPO, "reactranker_amd", "csrc", "Makefile")).read()
    assert "cluster.hip" in mk and "row_chain.h" in mk
    # the difference chain has one copy: both streaming files include it, neither restates it
    csrc = os.path.join(REPO, "reactranker_amd", "csrc")
    for name in ("kcenter.hip", "cluster.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "row_chain.h"' in text and "acc + t * t;" not in text, name
    assert "acc + t * t;" in open(os.path.join(csrc, "row_chain.h")).read()


def _rc(q=PTR, ld_q=8, M=4, bank=PTR, ld_b=8, N=100, H=8, r2=1.0, qg=None, bg=None, bn=None, count=PTR, ws=PTR, ws_bytes=1 << 30):
    return _lib.lib().rr_radius_count_f32(q, ld_q, M, bank, ld_b, N, H, C.c_float(r2), qg, bg, bn, count, ws,
                                          C.c_size_t(ws_bytes), None)


def test_radius_count_status_codes_come_back_before_any_launch():
    l = _lib.lib()
    for name in ("q", "bank", "count", "ws"):
        assert _rc(**{name: None}) == ARG, name
    assert _rc(qg=PTR) == ARG and _rc(bg=PTR) == ARG                       # one group array without the other
    assert _rc(M=-1) == ARG and _rc(N=-1) == ARG
    assert _rc(H=0) == ARG and _rc(H=-2) == ARG
    assert _rc(ld_q=7) == ARG and _rc(ld_b=7) == ARG                       # a pitch below H
    assert _rc(r2=NAN) == ARG and _rc(r2=-1.0) == ARG and _rc(r2=-INF) == ARG
    assert _rc(N=1 << 31) == UNSUPPORTED and _rc(M=1 << 31) == UNSUPPORTED
    need = C.c_size_t()
    assert l.rr_radius_count_workspace_bytes(4, 100, C.byref(need)) == OK and need.value >= 4 * 4 + 100 * 4
    assert _rc(ws_bytes=need.value - 1) == WORKSPACE
    assert _rc(ws_bytes=0) == WORKSPACE
    assert _rc(M=0, ws_bytes=need.value) == OK                             # no rows: nothing is launched
    assert _rc(M=0, r2=INF, ws_bytes=need.value) == OK and _rc(M=0, r2=0.0, ws_bytes=need.value) == OK
    # the sizing call itself
    assert l.rr_radius_count_workspace_bytes(4, 100, None) == ARG
    assert l.rr_radius_count_workspace_bytes(-1, 100, C.byref(need)) == ARG
    assert l.rr_radius_count_workspace_bytes(4, -1, C.byref(need)) == ARG
    assert l.rr_radius_count_workspace_bytes(1 << 31, 4, C.byref(need)) == UNSUPPORTED
    assert l.rr_radius_count_workspace_bytes(4, 1 << 31, C.byref(need)) == UNSUPPORTED
    assert l.rr_radius_count_workspace_bytes(0, 0, C.byref(need)) == OK and need.value > 0
    # the partial counts [M, S] follow knn's split setting
    one, seven = C.c_size_t(), C.c_size_t()
    try:
        assert l.rr_knn_set_splits(1) == OK
        assert l.rr_radius_count_workspace_bytes(100, 5000, C.byref(one)) == OK
        assert l.rr_knn_set_splits(7) == OK
        assert l.rr_radius_count_workspace_bytes(100, 5000, C.byref(seven)) == OK
        assert seven.value >= one.value + 100 * 7 * 4
        assert _rc(M=100, N=5000, ws_bytes=one.value) == WORKSPACE
    finally:
        assert l.rr_knn_set_splits(0) == OK


def _se(x=PTR, ld=8, P=100, H=8, r2=1.0, key=None, first=0, n=5, labels=PTR, centres=PTR, ws=PTR, ws_bytes=1 << 30):
    return _lib.lib().rr_sphere_exclusion_f32(x, ld, P, H, C.c_float(r2), key, first, n, labels, centres, ws, C.c_size_t(ws_bytes),
                                              None)


def test_sphere_exclusion_status_codes_come_back_before_any_launch():
    l = _lib.lib()
    for name in ("x", "labels", "centres", "ws"):
        assert _se(**{name: None}) == ARG, name
    assert _se(P=-1) == ARG and _se(n=-1) == ARG and _se(first=-1) == ARG
    assert _se(H=0) == ARG and _se(H=-2) == ARG
    assert _se(ld=7) == ARG                                                # a pitch below H
    assert _se(r2=NAN) == ARG and _se(r2=-1.0) == ARG and _se(r2=-INF) == ARG
    assert _se(n=65537) == UNSUPPORTED
    assert _se(P=1 << 31) == UNSUPPORTED
    assert _se(first=(1 << 31) - 3, n=5) == UNSUPPORTED                    # a round number past int32
    need = C.c_size_t()
    assert l.rr_sphere_exclusion_workspace_bytes(100, C.byref(need)) == OK and need.value >= 2 * 4096 * 8
    assert _se(ws_bytes=need.value - 1) == WORKSPACE
    assert _se(ws_bytes=0) == WORKSPACE
    assert _se(P=0, n=0, ws_bytes=need.value) == OK                        # nothing to write: nothing is launched
    assert _se(P=0, n=0, r2=INF, ws_bytes=need.value) == OK and _se(P=0, n=0, r2=0.0, first=7, ws_bytes=need.value) == OK
    # the sizing call itself
    assert l.rr_sphere_exclusion_workspace_bytes(100, None) == ARG
    assert l.rr_sphere_exclusion_workspace_bytes(-1, C.byref(need)) == ARG
    assert l.rr_sphere_exclusion_workspace_bytes(1 << 31, C.byref(need)) == UNSUPPORTED
    assert l.rr_sphere_exclusion_workspace_bytes(0, C.byref(need)) == OK and need.value > 0
    assert l.rr_sphere_exclusion_workspace_bytes((1 << 31) - 1, C.byref(need)) == OK


def test_the_blocks_setting_is_checked_and_does_not_move_the_workspace():
    l = _lib.lib()
    assert l.rr_sphere_exclusion_blocks() == 0
    a, b = C.c_size_t(), C.c_size_t()
    try:
        assert l.rr_sphere_exclusion_set_blocks(1) == OK and l.rr_sphere_exclusion_blocks() == 1
        assert l.rr_sphere_exclusion_workspace_bytes(5000, C.byref(a)) == OK
        assert l.rr_sphere_exclusion_set_blocks(4096) == OK and l.rr_sphere_exclusion_blocks() == 4096
        assert l.rr_sphere_exclusion_workspace_bytes(5000, C.byref(b)) == OK
        assert a.value == b.value
        assert l.rr_sphere_exclusion_set_blocks(-1) == ARG and l.rr_sphere_exclusion_set_blocks(4097) == ARG
        assert l.rr_sphere_exclusion_blocks() == 4096 and l.rr_kcenter_blocks() == 0      # a word of its own
    finally:
        assert l.rr_sphere_exclusion_set_blocks(0) == OK
    assert l.rr_sphere_exclusion_blocks() == 0


# ---------------------------------------------------------------------------------------------- the Python layer
def test_python_argument_checks_raise_before_any_launch():
    x, y = torch.zeros(7, 5), torch.zeros(3, 5)
    with pytest.raises(ValueError, match="GPU"):
        K.radius_count(y, x, 1.0)                                            # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        K.sphere_exclusion(x, 1.0)
    for r in (-1.0, NAN, -INF):
        with pytest.raises(ValueError, match="radius"):
            K.radius_count(y, x, r)
        with pytest.raises(ValueError, match="radius"):
            K.sphere_exclusion(x, r)
    with pytest.raises(ValueError, match="width"):
        K.radius_count(y, torch.zeros(7, 6), 1.0)
    with pytest.raises(ValueError, match="go together"):
        K.radius_count(y, x, 1.0, q_group=[0, 1, 2])
    with pytest.raises(ValueError, match="order"):
        K.sphere_exclusion(x, 1.0, order="size")
    for n in (-1, 65537, 2.5):
        with pytest.raises(ValueError, match="max_clusters"):
            K.sphere_exclusion(x, 1.0, max_clusters=n)
    with pytest.raises(ValueError, match="width 0"):
        K.sphere_exclusion(torch.zeros(7, 0), 1.0)
    with pytest.raises(ValueError, match="matrix"):
        K.sphere_exclusion(torch.zeros(5), 1.0)
    with pytest.raises(ValueError, match="float32"):
        K.sphere_exclusion(x.double(), 1.0)
    with pytest.raises(ValueError, match="quantile"):
        K.suggest_radius(x, quantile=1.5)
    assert K.radius_squared(3.0) == 9.0 and K.radius_squared(INF) == INF and K.radius_squared(0.0) == 0.0
    assert K.radius_squared(0.1) == float(CR.r2_of(0.1)) and K.ROWS_PER_WORKGROUP == 4 and K.ROUND_BATCH == 256


# ---------------------------------------------------------------------------------------------- the folds
def _labels(sizes, seed, negatives=0):
    lab = np.repeat(np.arange(len(sizes)), sizes)
    lab = np.concatenate([lab, np.full(negatives, -1), np.full(negatives, -2)])
    return lab[np.random.default_rng(seed).permutation(lab.size)]


SIZES = [40, 7, 7, 7, 7, 3, 3, 3, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 12, 12, 25]


@pytest.mark.parametrize("fractions", [(0.8, 0.1, 0.1), (0.5, 0.5), (3, 1, 1, 1), (1.0,)], ids=str)
def test_cluster_split_keeps_clusters_whole_and_meets_its_targets(fractions):
    lab = _labels(SIZES, 3, negatives=5)
    folds = K.cluster_split(lab, fractions, seed=1)
    assert isinstance(folds, np.ndarray) and folds.dtype == np.int64 and folds.shape == lab.shape
    fr = np.asarray(fractions, np.float64) / np.sum(fractions)
    assert np.array_equal(folds, CR.folds_ref(lab, fr, 1))
    assert (folds[lab < 0] == -1).all() and (folds[lab >= 0] >= 0).all() and folds.max() < len(fractions)
    for c in range(len(SIZES)):
        assert len(set(folds[lab == c].tolist())) == 1, c                   # whole clusters only
    have = np.bincount(folds[folds >= 0], minlength=len(fractions))
    assert (np.abs(have - fr * sum(SIZES)) < max(SIZES)).all()                # within one cluster of the target
    # a tensor in, a tensor out; deterministic per seed
    t = K.cluster_split(torch.from_numpy(lab), fractions, seed=1)
    assert torch.is_tensor(t) and t.dtype == torch.int64 and np.array_equal(t.numpy(), folds)
    assert np.array_equal(K.cluster_split(lab, fractions, seed=1), folds)


def test_another_seed_moves_clusters_of_equal_size():
    lab = _labels(SIZES, 3)
    a = K.cluster_split(lab, (0.6, 0.2, 0.2), seed=0)
    others = [K.cluster_split(lab, (0.6, 0.2, 0.2), seed=s) for s in range(1, 6)]
    assert any(not np.array_equal(a, o) for o in others)
    for o in others:                                                          # the fold sizes do not depend on the seed
        assert np.array_equal(np.bincount(o), np.bincount(a))
    distinct = _labels([9, 8, 7, 6, 5, 4, 3, 2, 1], 4)                        # no two clusters of one size: the seed cannot matter
    assert all(np.array_equal(K.cluster_split(distinct, seed=0), K.cluster_split(distinct, seed=s)) for s in range(1, 4))


def test_cluster_kfold_and_degenerate_inputs():
    lab = _labels(SIZES, 5, negatives=2)
    folds = K.cluster_kfold(lab, 4, seed=2)
    assert np.array_equal(folds, CR.folds_ref(lab, [0.25] * 4, 2))
    have = np.bincount(folds[folds >= 0], minlength=4)
    assert (np.abs(have - sum(SIZES) / 4) < max(SIZES)).all() and (folds[lab < 0] == -1).all()
    for c in range(len(SIZES)):
        assert len(set(folds[lab == c].tolist())) == 1
    assert sorted(set(folds[folds >= 0].tolist())) == [0, 1, 2, 3]
    # a single giant cluster goes to fold 0, under either rule
    giant = np.zeros(50, np.int64)
    assert (K.cluster_split(giant) == 0).all() and (K.cluster_kfold(giant, 5) == 0).all()
    assert (K.cluster_split(np.full(4, -1)) == -1).all() and K.cluster_split(np.zeros(0, np.int64)).shape == (0,)
    with pytest.raises(ValueError, match="fractions"):
        K.cluster_split(giant, (0.5, -0.5))
    with pytest.raises(ValueError, match="fractions"):
        K.cluster_split(giant, (0.0, 0.0))
    for k in (0, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            K.cluster_kfold(giant, k)


def test_a_cpu_tensor_error_names_the_function_that_was_called():
    x, y = torch.zeros(7, 5), torch.zeros(3, 5)
    with pytest.raises(ValueError, match=r"^sphere_exclusion: .*GPU"):
        K.sphere_exclusion(x, 1.0)
    with pytest.raises(ValueError, match=r"^radius_count: .*GPU"):
        K.radius_count(y, x, 1.0)
