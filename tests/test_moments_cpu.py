"""The embedding Gaussian without a GPU: the numpy restatement of tests/moments_ref.py against independent truths (np.cov, affine
invariance of the Mahalanobis distance, the mean-distance identity, PCA score variances, the sign rule), the eigen
post-processing of reactranker_amd.latent_gaussian against it, the new symbols' declaration, export and binding, every status
code (all returned before any launch) and the Python argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from reactranker_amd import latent_gaussian as G
from tests import moments_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rr_moments_workspace_bytes", "rr_moments_chunks", "rr_col_moments_f64", "rr_moments_blocks", "rr_moments_set_blocks",
           "rr_center_project_f32")
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -4, -5
PTR = C.c_void_p(4096)          # a non-null pointer that is never followed: every call below returns before a launch


def data(seed, N, H, cond=10.0):
    """rows of a Gaussian whose covariance has condition number about cond^2, shifted off the origin"""
    rng = np.random.default_rng(seed)
    scale = np.logspace(0, np.log10(cond), H)
    mix = np.linalg.qr(rng.standard_normal((H, H)))[0]
    return ((rng.standard_normal((N, H)) * scale) @ mix + 3.0).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("N,H", [(2, 1), (5, 3), (257, 17), (1025, 33)])
def test_moments_ref_against_numpy_cov(N, H):
    x = data(N + H, N, H)
    x64 = x.astype(np.float64)
    for ddof in (0, 1):
        mean, cov, n = R.cov_ref(x, ddof)
        assert n == N
        want = np.cov(x64.T, ddof=ddof).reshape(H, H)
        scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
        assert np.abs(mean.astype(np.float64) - x64.mean(0)).max() <= 1e-13 * np.abs(x64).max()
        assert (np.abs(cov.astype(np.float64) - want) <= 1e-12 * scale).all()
    assert np.array_equal(cov, cov.T)


def test_row_filter_and_degenerate_counts():
    x = data(3, 9, 4)
    x[2, 1], x[5, 0], x[7, 3] = np.nan, np.inf, -np.inf
    assert R.used_rows(x).tolist() == [True, True, False, True, True, False, True, False, True]
    mean, sc, n = R.moments_ref(x)
    m2, s2, n2 = R.moments_ref(x[[0, 1, 3, 4, 6, 8]])
    assert n == n2 == 6 and np.array_equal(mean, m2) and np.array_equal(sc, s2)
    mean, sc, n = R.moments_ref(np.full((3, 4), np.nan, np.float32))
    assert n == 0 and not mean.any() and not sc.any()
    assert R.moments_ref(np.zeros((0, 4), np.float32))[2] == 0
    assert np.isnan(R.cov_ref(x[:1], 1)[1]).all() and not np.isnan(R.cov_ref(x[:1], 0)[1]).any()


def test_chunk_function_is_the_librarys():
    l = _lib.lib()
    for H in (1, 64, 65, 300, 322, 600, 1024):
        for N in (0, 1, 1023, 1024, 1025, 2048, 2049, 65536, 65537, 10 ** 6, 2 ** 31 - 1):
            assert l.rr_moments_chunks(N, H) == R.chunks(N, H) == G.chunks(N, H), (N, H)
        assert R.chunk_boundaries(H) == [1024, 2048]
    assert R.chunks(10 ** 6, 300) == 64 and R.chunks(10 ** 6, 1024) == 32          # 8 MiB slabs: the 256 MiB budget binds
    assert l.rr_moments_chunks(5, 1025) == 0 and l.rr_moments_chunks(-1, 8) == 0 and l.rr_moments_chunks(5, 0) == 0


def test_affine_invariance_of_the_mahalanobis_distance():
    """x -> x A + b with a well-conditioned A leaves the distances of a full-rank fit unchanged.  cond(cov) ~ 100 and cond(A) < 10
    keep the float64 eigen-decompositions well inside 1e-9 relative (checked here: the restatement's own precondition)."""
    N, H = 400, 12
    x = data(5, N, H)
    rng = np.random.default_rng(6)
    A = np.linalg.qr(rng.standard_normal((H, H)))[0] * np.linspace(1.0, 4.0, H)
    assert np.linalg.cond(A) < 10
    z = x.astype(np.float64) @ A + rng.standard_normal(H)
    f1 = R.fit_ref(x)
    # the transformed rows are not float32: fit them in float64 directly
    mean2 = z.mean(0)
    e2 = R.eigen_ref(np.cov(z.T))
    assert f1["rank"] == e2["rank"] == H and np.linalg.cond(f1["cov"]) < 1e3
    d1 = R.mahalanobis_ref(x, f1)
    d2 = R.project_ref(z, mean2, e2["components"] / np.sqrt(e2["eigenvalues"]))[1]
    assert np.abs(d1 - d2).max() <= 1e-9 * d1.max()
    # the identity: the bank's own mean squared distance is rank (n - 1) / n
    assert abs(d1.mean() - H * (N - 1) / N) <= 1e-9 * H


def test_pca_score_variances_are_the_eigenvalues_and_the_ratio_sums_to_one():
    x = data(8, 300, 9)
    f = R.fit_ref(x)
    y = R.project_ref(x, f["mean"], f["components_r"])[0]
    assert np.abs(y.var(axis=0, ddof=1) - f["eigenvalues"]).max() <= 1e-10 * f["eigenvalues"][0]
    assert np.abs(np.cov(y.T) - np.diag(f["eigenvalues"])).max() <= 1e-10 * f["eigenvalues"][0]
    assert (np.diff(f["eigenvalues"]) <= 0).all() and abs(f["explained_variance_ratio"].sum() - 1.0) < 1e-12
    lam = R.eigen_ref(f["cov"], shrinkage=0.25)["eigenvalues"]
    assert np.allclose(lam, 0.75 * f["eigenvalues"] + 0.25 * f["eigenvalues"].mean(), rtol=1e-12)
    assert R.fit_ref(x, rank=3)["whitener"].shape == (9, 3)


def test_the_sign_rule_makes_the_fit_invariant_to_a_row_permutation():
    x = data(9, 200, 7)
    a, b = R.fit_ref(x), R.fit_ref(x[np.random.default_rng(1).permutation(200)])
    big = np.abs(a["components"]).argmax(axis=0)
    assert (a["components"][big, np.arange(7)] > 0).all()
    assert np.abs(a["components"] - b["components"]).max() < 1e-9 and np.abs(a["whitener"] - b["whitener"]).max() < 1e-9
    # ties in magnitude go to the lower index
    e = R.eigen_ref(np.array([[2.0, 1.0], [1.0, 2.0]]))
    assert e["components"][0, 0] > 0 and e["components"][0, 1] > 0 and e["components"][1, 1] < 0


def test_rank_deficient_inputs_land_in_the_dropped_set():
    x = data(10, 300, 8)
    dup = np.concatenate([x, x[:, :3]], axis=1)                     # three duplicated columns
    assert R.fit_ref(dup)["rank"] == 8
    few = data(11, 5, 12)                                           # N < H: n - 1 directions carry variance
    assert R.fit_ref(few)["rank"] == 4
    const = np.concatenate([x, np.full((300, 1), 2.5, np.float32)], axis=1)
    assert R.fit_ref(const)["rank"] == 8
    assert R.fit_ref(x, eig_floor=0.5)["rank"] < 8


def test_eigen_model_is_the_restatement():
    x = data(12, 120, 10)
    cov = R.cov_ref(x)[1].astype(np.float64)
    for kw in (dict(), dict(shrinkage=0.3), dict(rank=4), dict(eig_floor=0.2)):
        got, want = G.eigen_model(torch.from_numpy(cov), **kw), R.eigen_ref(cov, **kw)
        assert got["rank"] == want["rank"]
        assert np.allclose(got["eigenvalues"].numpy(), want["eigenvalues"], rtol=1e-10, atol=1e-12 * want["eigenvalues"][0])
        assert np.abs(got["components"].numpy() - want["components"]).max() < 1e-8
        assert np.allclose(got["explained_variance_ratio"].numpy(), want["explained_variance_ratio"], atol=1e-12)
    for bad in (dict(shrinkage=-0.1), dict(shrinkage=1.5), dict(rank=0), dict(rank=11), dict(rank=2.5), dict(eig_floor=1.0)):
        with pytest.raises(ValueError):
            G.eigen_model(torch.from_numpy(cov), **bad)
    with pytest.raises(ValueError, match="finite"):
        G.eigen_model(torch.full((3, 3), float("nan"), dtype=torch.float64))


def test_sq_chain_and_project_bounds_by_hand():
    y = np.arange(1, 21, dtype=np.float32)[None, :]                  # exact: any order gives 2870
    assert R.sq_chain32(y).tolist() == [2870.0]
    a, b = np.float32(1.0), np.float32(2.0 ** -12)                   # b^2 = 2^-24, half an ulp of 1
    one = np.zeros((1, 8), np.float32)
    one[0, 0], one[0, 1:4] = a, b                                    # all in chain 0: each b^2 is rounded away (to even)
    assert R.sq_chain32(one)[0] == np.float32(1.0)
    two = np.zeros((1, 8), np.float32)
    two[0, 0], two[0, 4:7] = a, b                                    # chain 1 sums them to 1.5 ulp first
    assert R.sq_chain32(two)[0] == np.float32(1.0 + 2.0 ** -22)
    x, W = np.ones((2, 3)), np.ones((3, 2))
    by, bs = R.project_bounds(x, None, W)
    assert np.allclose(by, 2 * 6 * 2.0 ** -24 * 3) and bs.shape == (2,)


# ---------------------------------------------------------------------------------------------- the binding
def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "reactranker_hip.h")).read()
    declared = set(re.findall(r"\b(rr_[a-z0-9_]+)\s*\(", hdr))
    l = _lib.lib()
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS and getattr(l, s).argtypes is not None, s
    assert l.rr_version() == 8 == _lib.ABI_VERSION
    assert "#define RR_MOMENTS_MAX_H 1024" in hdr and _lib.RR_MOMENTS_MAX_H == 1024 == G.MAX_H == R.MAX_H
    assert "moments.hip" in open(os.path.join(REPO, "reactranker_amd", "csrc", "Makefile")).read()


def _mo(x=PTR, ld=8, N=100, H=8, mean=PTR, sc=PTR, n=PTR, ws=PTR, ws_bytes=1 << 40):
    return _lib.lib().rr_col_moments_f64(x, ld, N, H, mean, sc, n, ws, C.c_size_t(ws_bytes), None)


def _cp(x=PTR, ld=8, N=100, H=8, center=PTR, W=PTR, R_=4, y=PTR, sq=PTR):
    return _lib.lib().rr_center_project_f32(x, ld, N, H, center, W, R_, y, sq, None)


def test_status_codes_come_back_before_any_launch():
    l = _lib.lib()
    for name in ("x", "mean", "sc", "n", "ws"):
        assert _mo(**{name: None}) == ARG, name
    assert _mo(N=-1) == ARG and _mo(H=0) == ARG and _mo(H=-3) == ARG and _mo(ld=7) == ARG
    assert _mo(H=1025, ld=1025) == UNSUPPORTED and _mo(N=1 << 31) == UNSUPPORTED
    assert _mo(H=1025, ld=1025, ws_bytes=0) == UNSUPPORTED                   # the order: unsupported before workspace
    need = C.c_size_t()
    assert l.rr_moments_workspace_bytes(100, 8, C.byref(need)) == OK and need.value >= 100 + 64 * 64 * 8
    assert _mo(ws_bytes=need.value - 1) == WORKSPACE and _mo(ws_bytes=0) == WORKSPACE
    assert l.rr_moments_workspace_bytes(100, 8, None) == ARG
    assert l.rr_moments_workspace_bytes(-1, 8, C.byref(need)) == ARG and l.rr_moments_workspace_bytes(5, 0, C.byref(need)) == ARG
    assert l.rr_moments_workspace_bytes(5, 1025, C.byref(need)) == UNSUPPORTED
    assert l.rr_moments_workspace_bytes(1 << 31, 8, C.byref(need)) == UNSUPPORTED
    assert l.rr_moments_workspace_bytes(0, 1, C.byref(need)) == OK and need.value > 0
    assert l.rr_moments_workspace_bytes((1 << 31) - 1, 1024, C.byref(need)) == OK
    assert (1 << 31) - 1 + 32 * 1024 * 1024 * 8 <= need.value <= (1 << 31) + (1 << 28) + (1 << 20)
    for name in ("x", "W"):
        assert _cp(**{name: None}) == ARG, name
    assert _cp(y=None, sq=None) == ARG
    assert _cp(N=-1) == ARG and _cp(H=0) == ARG and _cp(ld=7) == ARG and _cp(R_=0) == ARG and _cp(R_=9) == ARG
    assert _cp(N=1 << 31) == UNSUPPORTED
    assert _cp(N=0) == OK and _cp(N=0, center=None, y=None) == OK            # nothing to write: nothing is launched


def test_the_blocks_setting_is_checked_and_does_not_move_the_workspace():
    l = _lib.lib()
    assert l.rr_moments_blocks() == 0
    a, b = C.c_size_t(), C.c_size_t()
    try:
        assert l.rr_moments_set_blocks(1) == OK and l.rr_moments_blocks() == 1
        assert l.rr_moments_workspace_bytes(5000, 300, C.byref(a)) == OK
        assert l.rr_moments_set_blocks(4096) == OK and l.rr_moments_blocks() == 4096
        assert l.rr_moments_workspace_bytes(5000, 300, C.byref(b)) == OK
        assert a.value == b.value >= 5000 + 5 * 320 * 320 * 8
        assert l.rr_moments_set_blocks(-1) == ARG and l.rr_moments_set_blocks(4097) == ARG and l.rr_moments_blocks() == 4096
    finally:
        assert l.rr_moments_set_blocks(0) == OK


# ---------------------------------------------------------------------------------------------- the Python layer
def test_python_argument_checks_raise_before_any_launch():
    x = torch.zeros(7, 5)
    with pytest.raises(ValueError, match="GPU"):
        G.moments(x)
    with pytest.raises(ValueError, match="GPU"):
        G.EmbeddingGaussian.fit(x)
    with pytest.raises(ValueError, match="GPU"):
        G.center_project(x, None, torch.zeros(5, 2))
    with pytest.raises(ValueError, match="ddof"):
        G.moments(x, ddof=2)
    with pytest.raises(ValueError, match="matrix"):
        G.moments(torch.zeros(5))
    with pytest.raises(ValueError, match="float32"):
        G.moments(x.double())
    with pytest.raises(ValueError, match="width 0"):
        G.moments(torch.zeros(7, 0))
    from reactranker_amd import neighbors as Nb
    assert Nb.APPLICABILITY_METHODS == ("knn", "mahalanobis")
    with pytest.raises(ValueError, match="method"):
        Nb.evaluate_applicability(None, None, [], "ck.pt", 0, method="euclid")
    with pytest.raises(ValueError, match="gaussian"):
        Nb.evaluate_applicability(None, None, [], "ck.pt", 0, gaussian=object())


def test_a_cpu_tensor_error_names_the_function_that_was_called():
    x = torch.zeros(7, 5)
    with pytest.raises(ValueError, match=r"^moments: .*GPU"):
        G.moments(x)
    with pytest.raises(ValueError, match=r"^center_project: .*GPU"):
        G.center_project(x, None, torch.zeros(5, 2))
