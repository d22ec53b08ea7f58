"""A Gaussian model of the embedding space: covariance, Mahalanobis distance, whitening and PCA of the
model's reaction vectors (neighbors.reaction_vectors, a ReactionBank).

  moments             (mean f64 [H], cov f64 [H, H], n_used) of the rows of a matrix: rr_col_moments_f64 (csrc/moments.hip), two
                      passes over the rows in f64 on the matrix core; rows that hold a NaN or an infinity are left out
  center_project      (x - center) @ W and / or its squared row norms in one kernel (rr_center_project_f32); with the norms only,
                      the product is never written
  EmbeddingGaussian   fit (eigen-decomposition of the covariance, float64 on the CPU: one H x H copy), mahalanobis, whiten,
                      project, save / load, from_bank

Euclidean neighbors.knn / kcenter_greedy on whiten()-ed rows are the Mahalanobis search and selection.
There is no CPU path: tensors on the CPU raise."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _embed, _lib
from ._lib import check, lib, ptr, stream

MAX_H = _lib.RR_MOMENTS_MAX_H


def chunks(n_rows: int, width: int) -> int:
    """how many contiguous chunks rr_col_moments_f64 cuts `n_rows` rows of `width` columns into (rr_moments_chunks)"""
    return int(lib().rr_moments_chunks(int(n_rows), int(width)))


def scatter(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(mean f64 [H], scatter f64 [H, H], n_used int64 0-dim), all on the device and without a host synchronisation:
    rr_col_moments_f64 as include/reactranker_hip.h states it.  scatter = sum over the used rows of (x - mean)(x - mean)^T."""
    x = _embed.rows(x, "x", "moments", min_width=1)
    N, H, dev = x.shape[0], x.shape[1], x.device
    if H > MAX_H:
        raise ValueError(f"moments: rows of width {H} (at most {MAX_H})")
    if N > 2 ** 31 - 1:
        raise ValueError(f"moments: {N} rows (at most 2^31 - 1)")
    mean = torch.empty(H, dtype=torch.float64, device=dev)
    sc = torch.empty(H, H, dtype=torch.float64, device=dev)
    n_used = torch.empty((), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _embed.scratch("rr_moments_workspace_bytes", dev, N, H)
        src = x if N > 0 else _embed.placeholder(dev)
        check(lib().rr_col_moments_f64(ptr(src), _embed.pitch(x), N, H, ptr(mean), ptr(sc), ptr(n_used), ptr(ws), nbytes,
                                       stream()), "rr_col_moments_f64")
    return mean, sc, n_used


def moments(x: torch.Tensor, ddof: int = 1) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(mean f64 [H], cov f64 [H, H], n_used) of the rows of `x` (float32 GPU matrix, contiguous rows, any pitch, H <= 1024).
    Rows that hold a NaN or an infinity are left out and not counted.  cov = scatter / (n_used - ddof), exactly symmetric; all
    NaN when n_used - ddof <= 0.  Reading n_used synchronises the host with the stream.
    ValueError - before any launch - for CPU tensors, other dtypes, width 0 or above 1024, or a ddof that is not 0 or 1."""
    if ddof not in (0, 1):
        raise ValueError(f"moments: ddof must be 0 or 1 (got {ddof!r})")
    mean, sc, n_used = scatter(x)
    n = int(n_used)
    # (a device tensor as the divisor: torch divides by a Python number through its reciprocal, which is not the rounded quotient)
    cov = sc / (n_used - ddof).to(torch.float64) if n - ddof > 0 else torch.full_like(sc, float("nan"))
    return mean, cov, n


def center_project(x: torch.Tensor, center: Optional[torch.Tensor], W: torch.Tensor, want_y: bool = True, want_sq: bool = False):
    """(y [N, R] or None, sq [N] or None): y = (x - center) @ W, sq = its squared row norms, float32, by rr_center_project_f32
    (include/reactranker_hip.h states the chains).  center [H] float32 or None (zeros); W [H, R] float32, 1 <= R <= H.  With
    want_y False the product is never written.  Ordered on the current stream, no scratch."""
    who = "center_project"
    x = _embed.rows(x, "x", who, min_width=1)
    N, H, dev = x.shape[0], x.shape[1], x.device
    if not torch.is_tensor(W) or W.dim() != 2 or W.dtype != torch.float32 or W.device != dev:
        raise ValueError(f"{who}: `W` must be a float32 matrix [H, R] on {dev}")
    if W.shape[0] != H or not (1 <= W.shape[1] <= H):
        raise ValueError(f"{who}: `W` has shape {tuple(W.shape)} for rows of width {H} ([H, R] with 1 <= R <= H required)")
    if center is not None and (not torch.is_tensor(center) or center.dtype != torch.float32 or center.device != dev
                               or center.numel() != H):
        raise ValueError(f"{who}: `center` must be {H} float32 values on {dev}")
    if not (want_y or want_sq):
        raise ValueError(f"{who}: nothing asked for (want_y and want_sq both False)")
    if N > 2 ** 31 - 1:
        raise ValueError(f"{who}: {N} rows (at most 2^31 - 1)")
    W = W.detach().contiguous()
    R = W.shape[1]
    center = None if center is None else center.detach().reshape(-1).contiguous()
    y = torch.empty(N, R, dtype=torch.float32, device=dev) if want_y else None
    sq = torch.empty(N, dtype=torch.float32, device=dev) if want_sq else None
    if N > 0:
        with torch.cuda.device(dev):
            check(lib().rr_center_project_f32(ptr(x), _embed.pitch(x), N, H, ptr(center), ptr(W), R, ptr(y), ptr(sq), stream()),
                  "rr_center_project_f32")
    return y, sq


def eigen_model(cov: torch.Tensor, shrinkage: float = 0.0, rank: Optional[int] = None, eig_floor: Optional[float] = None) -> dict:
    """The eigen post-processing of fit(), on the CPU in float64 (no GPU needed): dict(eigenvalues [H] descending, after shrinkage;
    components [H, H], column k the eigenvector of eigenvalue k with its largest-magnitude entry positive (ties: the lower index);
    rank: how many leading directions the whitening keeps; explained_variance_ratio [H])."""
    cov = torch.as_tensor(cov).detach().to(device="cpu", dtype=torch.float64)
    H = cov.shape[0]
    if cov.dim() != 2 or cov.shape[1] != H or H < 1:
        raise ValueError(f"EmbeddingGaussian: the covariance must be a square matrix (got {tuple(cov.shape)})")
    if not (0.0 <= float(shrinkage) <= 1.0):
        raise ValueError(f"EmbeddingGaussian: shrinkage must lie in [0, 1] (got {shrinkage!r})")
    if rank is not None and (int(rank) != rank or not (1 <= int(rank) <= H)):
        raise ValueError(f"EmbeddingGaussian: rank must be an integer in [1, {H}] (got {rank!r})")
    floor = H * 2.0 ** -24 if eig_floor is None else float(eig_floor)
    if not (0.0 <= floor < 1.0):
        raise ValueError(f"EmbeddingGaussian: eig_floor is a fraction of the largest eigenvalue in [0, 1) (got {eig_floor!r})")
    if not bool(torch.isfinite(cov).all()):
        raise ValueError("EmbeddingGaussian: the covariance is not finite (fewer than two usable rows?)")
    lam, vec = torch.linalg.eigh(cov)
    lam, vec = lam.flip(0), vec.flip(1)
    lam = lam.clamp_min(0.0)
    s = float(shrinkage)
    lam = (1.0 - s) * lam + s * lam.mean()
    big = vec.abs().argmax(dim=0)                                    # (argmax returns the first of equal maxima: the lower index)
    sign = torch.sign(vec[big, torch.arange(H)])
    sign = torch.where(sign == 0, torch.ones_like(sign), sign)
    vec = vec * sign
    keep = int((lam > floor * lam[0]).sum()) if float(lam[0]) > 0 else 0
    if rank is not None:
        keep = min(keep, int(rank))
    total = float(lam.sum())
    evr = lam / total if total > 0 else torch.zeros_like(lam)
    return dict(eigenvalues=lam, components=vec.contiguous(), rank=keep, explained_variance_ratio=evr)


class EmbeddingGaussian:
    """The Gaussian of a set of reaction vectors.  mean_ f64 [H], cov_ f64 [H, H], eigenvalues_ f64 [H] (descending, after
    shrinkage), components_ f32 [H, rank_] (device), whitener_ = components_ / sqrt(eigenvalue) f32 [H, rank_] (device), n_ (rows
    used), rank_, explained_variance_ratio_ f64 [H]."""

    def __init__(self, mean, cov, eig: dict, n: int, device):
        dev = torch.device(device)
        r = int(eig["rank"])
        if r < 1:
            raise ValueError("EmbeddingGaussian: no direction of positive variance is left (constant or too few rows)")
        self.mean_ = torch.as_tensor(mean).detach().to("cpu", torch.float64)
        self.cov_ = torch.as_tensor(cov).detach().to("cpu", torch.float64)
        self.eigenvalues_ = eig["eigenvalues"]
        self.explained_variance_ratio_ = eig["explained_variance_ratio"]
        self.n_, self.rank_ = int(n), r
        comp = eig["components"][:, :r]
        self.components_ = comp.to(torch.float32).contiguous().to(dev)
        self.whitener_ = (comp / self.eigenvalues_[:r].sqrt()).to(torch.float32).contiguous().to(dev)
        self.center_ = self.mean_.to(torch.float32).to(dev)

    @classmethod
    def fit(cls, vectors: torch.Tensor, shrinkage: float = 0.0, rank: Optional[int] = None,
            eig_floor: Optional[float] = None) -> "EmbeddingGaussian":
        """moments(vectors, ddof=1), then torch.linalg.eigh of the covariance in float64 on the CPU (eigen_model says what
        happens to the eigenvalues and signs).  Directions whose eigenvalue is at most eig_floor (default H 2^-24, the f32 noise
        floor of the inputs) times the largest are dropped from the whitening; rank = r keeps at most the top r."""
        x = _embed.rows(vectors, "vectors", "EmbeddingGaussian.fit", min_width=1)
        mean, cov, n = moments(x, ddof=1)
        if n < 2:
            raise ValueError(f"EmbeddingGaussian.fit: {n} usable rows (at least 2 needed)")
        return cls(mean, cov, eigen_model(cov, shrinkage, rank, eig_floor), n, x.device)

    @classmethod
    def from_bank(cls, bank, **kw) -> "EmbeddingGaussian":
        """fit(bank.vectors, ...) of a neighbors.ReactionBank"""
        return cls.fit(bank.vectors, **kw)

    def _check(self, vectors, who):
        x = _embed.rows(vectors, "vectors", who, min_width=1)
        if x.shape[1] != self.center_.numel():
            raise ValueError(f"{who}: vectors of width {x.shape[1]}, the model was fitted on width {self.center_.numel()}")
        if x.device != self.center_.device:
            raise ValueError(f"{who}: vectors on {x.device}, the model on {self.center_.device}")
        return x

    def mahalanobis(self, vectors: torch.Tensor) -> torch.Tensor:
        """[M] float32 SQUARED Mahalanobis distances to the fitted Gaussian over its rank_ kept directions; one kernel, four
        bytes written per row.  A row that holds a NaN gives NaN."""
        x = self._check(vectors, "EmbeddingGaussian.mahalanobis")
        return center_project(x, self.center_, self.whitener_, want_y=False, want_sq=True)[1]

    def whiten(self, vectors: torch.Tensor) -> torch.Tensor:
        """[M, rank_] float32: squared Euclidean distances between whitened rows are squared Mahalanobis distances"""
        x = self._check(vectors, "EmbeddingGaussian.whiten")
        return center_project(x, self.center_, self.whitener_)[0]

    def project(self, vectors: torch.Tensor, n_components: int = 2) -> torch.Tensor:
        """[M, n_components] float32 PCA scores (the first n_components <= rank_ principal directions)"""
        n = int(n_components)
        if n != n_components or not (1 <= n <= self.rank_):
            raise ValueError(f"EmbeddingGaussian.project: n_components must be an integer in [1, {self.rank_}] (got {n_components!r})")
        x = self._check(vectors, "EmbeddingGaussian.project")
        return center_project(x, self.center_, self.components_[:, :n].contiguous())[0]

    def save(self, path) -> None:
        torch.save(dict(mean=self.mean_, cov=self.cov_, eigenvalues=self.eigenvalues_, rank=self.rank_, n=self.n_,
                        explained_variance_ratio=self.explained_variance_ratio_, components=self.components_.cpu(),
                        whitener=self.whitener_.cpu()), path)

    @classmethod
    def load(cls, path, device) -> "EmbeddingGaussian":
        d = torch.load(path, map_location="cpu")
        self = cls.__new__(cls)
        dev = torch.device(device)
        self.mean_, self.cov_, self.eigenvalues_ = d["mean"], d["cov"], d["eigenvalues"]
        self.explained_variance_ratio_ = d["explained_variance_ratio"]
        self.n_, self.rank_ = int(d["n"]), int(d["rank"])
        self.components_, self.whitener_ = d["components"].to(dev), d["whitener"].to(dev)
        self.center_ = self.mean_.to(torch.float32).to(dev)
        return self
