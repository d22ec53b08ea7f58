"""Sphere-exclusion clustering of reaction embeddings and cluster-held-out splits: how to split the data
so that validation measures generalisation instead of near-duplicate recall.

  radius_count      neighbours of every query row within a radius of a bank (rr_radius_count_f32: knn's tile walk with a
                    counting epilogue) - the local density of a training set around a candidate
  sphere_exclusion  Taylor-Butina clustering (rr_sphere_exclusion_f32): the densest unassigned row becomes a centre, every
                    unassigned row inside its sphere joins it, repeat; order='index' is the leader algorithm
  suggest_radius    a radius from the data: a quantile of the distance to the k-th neighbour
  query_vectors     the mean reaction vector per query (the ranking data is split by query, not by candidate)
  cluster_split     whole clusters to folds by target fractions; cluster_kfold: the same with k equal folds (host, deterministic)
  split_report      how far the held-out folds lie from fold 0, to set a cluster split next to a random one

What the clustering guarantees: every member lies within the radius of its centre, and two centres lie farther than the radius
apart.  NOT that two members of different clusters lie farther apart than the radius.

radius_count, sphere_exclusion, suggest_radius, query_vectors and split_report take GPU tensors only; there is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _embed, _lib
from ._lib import check, lib, ptr, stream
from .neighbors import knn

MAX_ROUNDS = _lib.RR_SPHERE_EXCLUSION_MAX_ROUNDS
ROWS_PER_WORKGROUP = 4                                     # one wavefront per row, 256 threads (csrc/cluster.hip)
ROUND_BATCH = 256                                          # rounds per call when the number of clusters is not given
ORDERS = ("density", "index")
REPORT_LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)


def radius_squared(radius) -> float:
    """THE rule that turns a radius into the squared radius the kernels compare against: float32(float64(radius) ** 2).
    ValueError for a negative radius or a NaN; +inf is allowed."""
    r = float(radius)
    if not r >= 0.0:
        raise ValueError(f"radius must be >= 0 and not a NaN (got {radius!r})")
    with np.errstate(over="ignore"):
        return float(np.float32(np.float64(r) ** 2))


def radius_count(queries: torch.Tensor, bank: torch.Tensor, radius, q_group=None, b_group=None,
                 bank_sqnorm=None) -> torch.Tensor:
    """How many bank rows lie within `radius` of every query row: int64 [M].

    count[m] = #{n : d(m, n) <= r2 and (m, n) not excluded} with r2 = float32(float64(radius) ** 2) and d = knn()'s squared
    distance max(0, |q|^2 + |b|^2 - 2 q.b) in f32, bit for bit (include/reactranker_hip.h states the chains).  A pair is
    excluded when q_group[m] == b_group[n] >= 0 (both or neither given) or when its distance is a NaN.  A row compared with
    itself counts like any other pair.  bank_sqnorm: row_sqnorm(bank) kept from an earlier call.
    Scratch comes from torch's allocator on the current stream, and the call is ordered on that stream.
    ValueError - before any launch - for CPU tensors, widths that differ or are 0, one group array without the other, or a
    radius that is negative or a NaN."""
    who = "radius_count"
    _embed.matrix(queries, "queries", who)
    _embed.matrix(bank, "bank", who)
    r2 = radius_squared(radius)
    if queries.shape[1] != bank.shape[1] or queries.shape[1] < 1:
        raise ValueError(f"radius_count: queries have width {queries.shape[1]}, the bank {bank.shape[1]} (equal and >= 1 required)")
    if (q_group is None) != (b_group is None):
        raise ValueError("radius_count: q_group and b_group go together (both or neither)")
    q, b = _embed.rows(queries, "queries", who), _embed.rows(bank, "bank", who)
    if q.device != b.device:
        raise ValueError(f"radius_count: queries on {q.device}, bank on {b.device}")
    M, N, H, dev = q.shape[0], b.shape[0], q.shape[1], q.device
    if max(M, N) > 2 ** 31 - 1:
        raise ValueError(f"radius_count: {max(M, N)} rows (at most 2^31 - 1)")
    qg = bg = None
    if q_group is not None:
        qg, bg = _embed.group(q_group, M, dev, "q_group", who), _embed.group(b_group, N, dev, "b_group", who)
    bn = None if bank_sqnorm is None else _embed.per_row(bank_sqnorm, N, None, "bank_sqnorm", who)
    count = torch.empty(M, dtype=torch.int32, device=dev)
    if M == 0:
        return count.to(torch.int64)
    if N == 0:                                             # (the C entry wants a bank pointer even when it holds no row)
        b, bg = _embed.empty_bank(H, dev, bg is not None)
    with torch.cuda.device(dev):
        ws, nbytes = _embed.scratch("rr_radius_count_workspace_bytes", dev, M, N)
        check(lib().rr_radius_count_f32(ptr(q), _embed.pitch(q), M, ptr(b), _embed.pitch(b), N, H, C.c_float(r2),
                                        ptr(qg), ptr(bg), ptr(bn), ptr(count), ptr(ws), nbytes, stream()), "rr_radius_count_f32")
    return count.to(torch.int64)


def sphere_exclusion(vectors: torch.Tensor, radius, order: str = "density", key=None, max_clusters: Optional[int] = None) -> dict:
    """Sphere-exclusion clustering of `vectors` [P, H]: dict(labels [P] int64, centres [K] int64, sizes [K] int64, key [P] int64
    or None, n_clusters, n_unassigned: 0-dim int64 tensors) - rr_sphere_exclusion_f32, include/reactranker_hip.h states it.

    Round t takes the unassigned row with the largest key (TIES go to the LOWER row index, so the labels are the same on every
    run) as centre t; every unassigned row within `radius` of it - the centre itself included - gets label t.  Distances are
    kcenter_greedy's sum_h (x[i,h] - x[c,h])^2 in f32, compared against r2 = float32(float64(radius) ** 2).  A row that holds a
    NaN or an infinity gets label -2 and is never a centre or a member; a row no round has reached yet has label -1.
    order 'density' (Taylor-Butina): key = radius_count(vectors, vectors, radius), the number of rows within the radius, taken
    once before the first round.  order 'index' (the leader algorithm): every key equal, so rows become centres in index order
    and no [P, P] pass is needed.  An explicit integer `key` [P] (int32 range) overrides both.
    max_clusters = n: exactly n rounds in one call of the library, no host synchronisation; centres and sizes have n entries,
    those of rounds that found no unassigned row hold -1 and 0.  Rows may be left at -1 when n is too small.
    max_clusters = None: rounds run in batches of 256; after each batch the host reads the batch's last centre (4 bytes) and
    stops at the first -1 - every round before that assigned at least its centre, so there are at most P rounds.  centres is
    trimmed to the real ones and no row is left at -1.
    `vectors`: float32 GPU matrix with contiguous rows, any pitch.  Scratch comes from torch's allocator on the current stream,
    and every call is ordered on that stream.
    ValueError - before any launch - for CPU tensors, width 0, an unknown order, a radius that is negative or a NaN, a key that
    is not P integers, or max_clusters outside [0, 65536]."""
    _embed.matrix(vectors, "vectors", "sphere_exclusion")
    if order not in ORDERS:
        raise ValueError(f"sphere_exclusion: order must be one of {ORDERS} (got {order!r})")
    r2 = radius_squared(radius)
    n = None
    if max_clusters is not None:
        n = int(max_clusters)
        if n != max_clusters or not (0 <= n <= MAX_ROUNDS):
            raise ValueError(f"sphere_exclusion: max_clusters must be an integer in [0, {MAX_ROUNDS}] (got {max_clusters!r})")
    if vectors.shape[1] < 1:
        raise ValueError("sphere_exclusion: rows of width 0")
    x = _embed.rows(vectors, "vectors", "sphere_exclusion")
    P, H, dev = x.shape[0], x.shape[1], x.device
    if P > 2 ** 31 - 1:
        raise ValueError(f"sphere_exclusion: {P} rows (at most 2^31 - 1)")
    if key is not None:
        k32 = _embed.group(key, P, dev, "key", "sphere_exclusion")
    elif order == "density" and P > 0:
        k32 = radius_count(x, x, radius).to(torch.int32)
    else:
        k32 = None
    labels = torch.empty(P, dtype=torch.int32, device=dev)
    one = _embed.placeholder(dev, torch.int32)
    with torch.cuda.device(dev):
        ws, nbytes = _embed.scratch("rr_sphere_exclusion_workspace_bytes", dev, P)

        def rounds(first, count, out):
            check(lib().rr_sphere_exclusion_f32(ptr(x) if P > 0 else ptr(one), _embed.pitch(x), P, H, C.c_float(r2), ptr(k32),
                                                first, count, ptr(labels) if P > 0 else ptr(one),
                                                ptr(out) if count > 0 else ptr(one), ptr(ws), nbytes, stream()),
                  "rr_sphere_exclusion_f32")
        if n is not None:
            centres = torch.empty(n, dtype=torch.int32, device=dev)
            rounds(0, n, centres)
        elif P == 0:
            centres = torch.empty(0, dtype=torch.int32, device=dev)
        else:
            batches, first = [], 0
            while True:                                            # (at most P / 256 + 1 batches: see the docstring)
                batch = torch.empty(ROUND_BATCH, dtype=torch.int32, device=dev)
                rounds(first, ROUND_BATCH, batch)
                batches.append(batch)
                first += ROUND_BATCH
                if int(batch[-1]) < 0:
                    break
            centres = torch.cat(batches)
            centres = centres[centres >= 0]
    centres = centres.to(torch.int64)
    labels = labels.to(torch.int64)
    K = centres.shape[0]
    sizes = torch.zeros(K, dtype=torch.int64, device=dev)
    if K > 0 and P > 0:
        member = labels >= 0
        sizes.index_add_(0, torch.where(member, labels, torch.zeros_like(labels)), member.to(torch.int64))
    return dict(labels=labels, centres=centres, sizes=sizes, key=None if k32 is None else k32.to(torch.int64),
                n_clusters=(centres >= 0).sum(), n_unassigned=(labels == -1).sum())


def suggest_radius(vectors: torch.Tensor, k: int = 8, quantile: float = 0.5) -> float:
    """A radius that makes `k` neighbours typical: the `quantile` of the distance from every row to its k-th nearest other row
    (knn with every row in a group of its own, so a row does not find itself; rows with fewer than k neighbours, or with
    non-finite values, are left out).  A Python float; ValueError when no row has k neighbours."""
    if not 0.0 <= float(quantile) <= 1.0:
        raise ValueError(f"suggest_radius: quantile must lie in [0, 1] (got {quantile!r})")
    x = _embed.rows(vectors, "vectors", "suggest_radius")
    g = torch.arange(x.shape[0], dtype=torch.int32, device=x.device)
    dist, _ = knn(x, x, k, q_group=g, b_group=g)
    d = dist[:, int(k) - 1]
    d = d[torch.isfinite(d)]
    if d.numel() == 0:
        raise ValueError(f"suggest_radius: no row has {k} neighbours")
    return float(torch.quantile(d.double().sqrt(), float(quantile)))


def query_vectors(vectors: torch.Tensor, group) -> torch.Tensor:
    """The mean reaction vector of every query: [Q, H] float32 for `vectors` [N, H] and `group` [N], the running index of the
    query a row belongs to (ReactionBank.group's numbering: 0 .. Q - 1, every query with at least one row).  Sums in float64."""
    x = _embed.rows(vectors, "vectors", "query_vectors")
    g = _embed.group(group, x.shape[0], x.device, "group", "query_vectors").to(torch.int64)
    if x.shape[0] == 0:
        return torch.zeros(0, x.shape[1], dtype=torch.float32, device=x.device)
    lo, hi = int(g.min()), int(g.max())
    if lo < 0:
        raise ValueError("query_vectors: negative query index")
    n = torch.zeros(hi + 1, dtype=torch.float64, device=x.device).index_add_(0, g, torch.ones_like(g, dtype=torch.float64))
    if bool((n == 0).any()):
        raise ValueError("query_vectors: a query index in 0 .. max has no row")
    s = torch.zeros(hi + 1, x.shape[1], dtype=torch.float64, device=x.device).index_add_(0, g, x.double())
    return (s / n[:, None]).to(torch.float32)


# ------------------------------------------------------------------------------------------------ folds (host)
def _folds(labels, targets: Sequence[float], seed: int):
    """labels -> fold per row (numpy int64) by the rule of cluster_split; targets are fractions that sum to 1"""
    lab = np.asarray(labels.detach().cpu() if torch.is_tensor(labels) else labels).reshape(-1).astype(np.int64)
    folds = np.full(lab.shape[0], -1, np.int64)
    ids, sizes = np.unique(lab[lab >= 0], return_counts=True)
    if ids.size == 0:
        return folds
    rank = np.random.default_rng(int(seed)).permutation(ids.size)         # ties between clusters of one size: seeded
    order = np.lexsort((rank, -sizes))
    want = np.asarray(targets, np.float64) * float(sizes.sum())
    have = np.zeros(len(want), np.float64)
    fold_of = np.empty(ids.size, np.int64)
    for c in order:
        f = int(np.argmax(want - have))                                   # the largest remaining deficit; ties: the lowest fold
        fold_of[c] = f
        have[f] += sizes[c]
    folds[lab >= 0] = fold_of[np.searchsorted(ids, lab[lab >= 0])]
    return folds


def _like(folds, labels):
    return torch.from_numpy(folds).to(labels.device) if torch.is_tensor(labels) else folds


def cluster_split(labels, fractions=(0.8, 0.1, 0.1), seed: int = 0):
    """A fold per row such that no cluster is cut: int64, a tensor on the labels' device for a tensor, an array for an array.

    Clusters (the distinct non-negative labels) are taken in order of size descending, ties in the order of a permutation
    seeded by `seed`; each goes to the fold with the largest remaining deficit against its target count, fractions[f] / sum of
    fractions times the number of rows with a non-negative label, ties to the lowest fold.  So every fold ends within the size
    of the largest cluster of its target, and one giant cluster goes to fold 0.  Rows with a negative label get fold -1.
    Runs on the host; deterministic for a given seed."""
    fr = np.asarray(fractions, np.float64).reshape(-1)
    if fr.size < 1 or not np.isfinite(fr).all() or (fr < 0).any() or fr.sum() <= 0:
        raise ValueError(f"cluster_split: fractions must be non-negative with a positive sum (got {fractions!r})")
    return _like(_folds(labels, fr / fr.sum(), seed), labels)


def cluster_kfold(labels, k: int, seed: int = 0):
    """cluster_split with k equal targets: a fold in 0 .. k - 1 per row, whole clusters only, -1 for a negative label."""
    kk = int(k)
    if kk != k or kk < 1:
        raise ValueError(f"cluster_kfold: k must be a positive integer (got {k!r})")
    return _like(_folds(labels, np.full(kk, 1.0 / kk), seed), labels)


def split_report(vectors: torch.Tensor, folds, k: int = 1) -> dict:
    """How far the held-out rows lie from the training rows: dict(levels, folds, n, quantiles [len(folds), len(levels)] float64
    on the host) - per held-out fold f >= 1 (ascending) the quantiles REPORT_LEVELS of the distance (not squared) from its n
    rows to their k-th nearest row of fold 0.  One knn call with the folds as groups: the bank is every row, and every row
    outside fold 0 shares one group id with the queries, so only fold 0 can be found.  A held-out row without k such
    neighbours counts as +inf.  Rows with a negative fold are in neither side."""
    x = _embed.rows(vectors, "vectors", "split_report")
    f = _embed.group(folds, x.shape[0], x.device, "folds", "split_report").to(torch.int64)
    held = (f >= 1).nonzero().reshape(-1)
    ids = sorted(set(f[held].cpu().tolist()))
    out = torch.full((len(ids), len(REPORT_LEVELS)), float("nan"), dtype=torch.float64)
    counts = []
    if held.numel() > 0:
        bg = torch.where(f == 0, torch.full_like(f, -1), torch.ones_like(f))
        dist, _ = knn(x[held].contiguous(), x, k, q_group=torch.ones_like(held), b_group=bg)
        d = dist[:, int(k) - 1].double().sqrt()
        levels = torch.tensor(REPORT_LEVELS, dtype=torch.float64, device=x.device)
        for j, fold in enumerate(ids):
            rows = d[f[held] == fold]
            counts.append(int(rows.numel()))
            fin = rows[torch.isfinite(rows)]
            if fin.numel() == rows.numel():
                out[j] = torch.quantile(rows, levels).cpu()
            else:                                                  # (torch.quantile interpolates inf - inf to a NaN)
                srt = torch.sort(rows).values
                pos = (levels * (rows.numel() - 1)).round().long()
                out[j] = srt[pos].cpu()
    return dict(levels=REPORT_LEVELS, folds=ids, n=counts, quantiles=out)
