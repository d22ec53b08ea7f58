"""Nearest-neighbour search over reaction embeddings: has the model seen anything like this reaction?

The embedding is the model's own reaction vector (the diff encoder's readout, RR_SAVED_VECS of a step plan); the search is
rr_knn_f32 (csrc/knn.hip): squared Euclidean distances from the matrix core, tile by tile, into a sorted list per query row -
the [M, N] distance matrix is never written.  On top of it:

  reaction_vectors        the embedding of every candidate of a list of batches, one eval-mode forward each
  knn                     (dist [M, k] float32, idx [M, k] int64) of query rows against bank rows, with optional group exclusion
  ReactionBank            vectors + squared norms + targets + query index per row of a set of reactions; save / load / query
  latent_distance         mean distance to the k nearest bank rows: a one-forward uncertainty for every task type
  evaluate_applicability  that distance - or the Mahalanobis distance to the bank's Gaussian (latent_gaussian, DESIGN.md section
                          4j) - against the model's error on a test set (uncertainty.uncertainty_calibration)
  split_overlap           test rows that have a (near-)duplicate in the bank
  kcenter_greedy          greedy k-center selection (rr_kcenter_f32): n rows of a pool, each the farthest
                          (optionally times a weight) from a labelled set and from the rows taken before it
  acquire                 which reactions to compute next: kcenter_greedy over a model's embedding of a pool, started from the
                          distance to a ReactionBank, optionally weighted by the predictive uncertainty

There is no CPU path: tensors on the CPU raise."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _embed, _lib
from . import eval as E
from . import uncertainty as U
from ._lib import check, lib, ptr, stream
from .functions import StepPlan
from .utils import load_checkpoint

MAX_K = _lib.RR_KNN_MAX_K
MAX_PICKS = _lib.RR_KCENTER_MAX_PICKS
KCENTER_ROWS_PER_WORKGROUP = 4                             # one wavefront per row, 256 threads (csrc/kcenter.hip)
METRICS = ("sqeuclidean", "cosine")
APPLICABILITY_METHODS = ("knn", "mahalanobis")


def geometry() -> Tuple[int, int, int]:
    """(query rows per workgroup, bank rows per tile, largest k) of the compiled library (rr_knn_geometry)"""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    lib().rr_knn_geometry(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def row_sqnorm(x: torch.Tensor) -> torch.Tensor:
    """sum_h x[r, h]^2 per row by the library's fixed f32 chain (rr_row_sqnorm_f32): what knn() takes as `bank_sqnorm`"""
    x = _embed.rows(x, "x", "row_sqnorm")
    if x.shape[1] < 1:
        raise ValueError("row_sqnorm: rows of width 0")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    if x.shape[0] == 0:
        return out
    with torch.cuda.device(x.device):
        check(lib().rr_row_sqnorm_f32(ptr(x), _embed.pitch(x), x.shape[0], x.shape[1], ptr(out), stream()), "rr_row_sqnorm_f32")
    return out


def _unit_rows(x: torch.Tensor) -> torch.Tensor:
    n = x.norm(dim=1, keepdim=True)
    return torch.where(n > 0, x / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(x))


def knn(queries: torch.Tensor, bank: torch.Tensor, k: int, q_group=None, b_group=None, bank_sqnorm=None,
        metric: str = "sqeuclidean") -> Tuple[torch.Tensor, torch.Tensor]:
    """The k nearest bank rows of every query row: (dist [M, k] float32 ascending, idx [M, k] int64).

    dist = max(0, |q|^2 + |b|^2 - 2 q.b) in f32 (include/reactranker_hip.h states the chains); ties go to the lower bank
    index.  A pair is excluded when q_group[m] == b_group[n] >= 0 (both or neither given; integer arrays, one entry per row)
    or when its distance is a NaN.  When fewer than k rows qualify the remaining slots hold dist = +inf, idx = -1.
    bank_sqnorm: row_sqnorm(bank) kept from an earlier call (metric 'sqeuclidean' only).
    metric 'cosine': rows are divided by their norm with torch first (a zero row stays zero) and the result is halved, so
    dist = 1 - cos for non-zero rows; a zero row is then at distance 1/2 from every unit row (and 0 from another zero row).
    Scratch comes from torch's allocator on the current stream, and the call is ordered on that stream.
    ValueError - before any launch - for CPU tensors, k outside [1, 64], widths that differ or are 0, or one group array
    without the other."""
    if metric not in METRICS:
        raise ValueError(f"knn: metric must be one of {METRICS} (got {metric!r})")
    _embed.matrix(queries, "queries", "knn")
    _embed.matrix(bank, "bank", "knn")
    kk = int(k)
    if kk != k or not (1 <= kk <= MAX_K):
        raise ValueError(f"knn: k must be an integer in [1, {MAX_K}] (got {k!r})")
    if queries.shape[1] != bank.shape[1] or queries.shape[1] < 1:
        raise ValueError(f"knn: queries have width {queries.shape[1]}, the bank {bank.shape[1]} (equal and >= 1 required)")
    if (q_group is None) != (b_group is None):
        raise ValueError("knn: q_group and b_group go together (both or neither)")
    q, b = _embed.rows(queries, "queries", "knn"), _embed.rows(bank, "bank", "knn")
    if q.device != b.device:
        raise ValueError(f"knn: queries on {q.device}, bank on {b.device}")
    M, N, H = q.shape[0], b.shape[0], q.shape[1]
    dev = q.device
    qg = bg = None
    if q_group is not None:
        qg, bg = _embed.group(q_group, M, dev, "q_group", "knn"), _embed.group(b_group, N, dev, "b_group", "knn")
    bn = None
    if metric == "cosine":
        if bank_sqnorm is not None:
            raise ValueError("knn: bank_sqnorm belongs to metric 'sqeuclidean' (cosine normalises the rows first)")
        q, b = _unit_rows(q), _unit_rows(b)
    elif bank_sqnorm is not None:
        bn = _embed.per_row(bank_sqnorm, N, None, "bank_sqnorm", "knn")
    dist = torch.empty(M, kk, dtype=torch.float32, device=dev)
    idx = torch.empty(M, kk, dtype=torch.int32, device=dev)
    if M == 0:
        return dist, idx.to(torch.int64)
    if N == 0:                                             # (the C entry wants a bank pointer even when it holds no row)
        b, bg = _embed.empty_bank(H, dev, bg is not None)
    with torch.cuda.device(dev):
        ws, nbytes = _embed.scratch("rr_knn_workspace_bytes", dev, M, N, kk)
        check(lib().rr_knn_f32(ptr(q), _embed.pitch(q), M, ptr(b), _embed.pitch(b), N, H, kk, ptr(qg), ptr(bg),
                               ptr(bn), ptr(dist), ptr(idx), ptr(ws), nbytes, stream()), "rr_knn_f32")
    if metric == "cosine":
        dist = dist * 0.5
    return dist, idx.to(torch.int64)


# ------------------------------------------------------------------------------------------------ the embedding
def _forward_with_vectors(model, r_batch, p_batch, add_features, gpu):
    """(model output, reaction vectors [M, H + F] as a copy) of one batch; the caller has set eval mode, no_grad and
    StepPlan.keep_last.  On the step-plan path the vectors are RR_SAVED_VECS of the forward that made the output; where a
    model does not qualify for a plan (hidden size % 4 != 0) the encoder modules are run once more, as
    encoder(p) - encoder(r) -> diff_encoder: the same kernels launch by launch."""
    StepPlan.last = None
    out = model(r_batch, p_batch, gpu=gpu, add_features=add_features)
    if StepPlan.last is not None:                          # (the saved rows are padded to the plan's pitch: keep H + F columns)
        return out, StepPlan.saved(_lib.RR_SAVED_VECS)[:, :int(model.ffn.hidden_size)].clone()
    if torch.is_tensor(add_features):
        add_features = add_features.detach().cpu().numpy()
    r_h, p_h = model.encoder(r_batch, gpu), model.encoder(p_batch, gpu)
    return out, model.diff_encoder(p_h - r_h, p_batch, gpu, features_batch=add_features).clone()


@contextlib.contextmanager
def _eval_keeping_vectors(model):
    """eval mode, no_grad and StepPlan.keep_last for the forwards inside; model.training, StepPlan.keep_last and StepPlan.last
    are left as found"""
    was_training, old_keep, old_last = model.training, StepPlan.keep_last, StepPlan.last
    try:
        model.eval()
        StepPlan.keep_last = True
        with torch.no_grad():
            yield
    finally:
        StepPlan.keep_last, StepPlan.last = old_keep, old_last
        model.train(was_training)


def reaction_vectors(model, batches: Iterable, gpu, include_features: bool = False) -> torch.Tensor:
    """The model's reaction vector of every candidate of `batches` ((r, p, scope, targets, add_features) tuples, the form
    the evaluators take; batches without queries are skipped): one eval-mode forward per batch under no_grad (on the step-plan
    path; _forward_with_vectors says what happens without one), the first H columns of RR_SAVED_VECS (all of them - the additional features behind the H readout columns - with
    include_features) copied out of the step's workspace before another step can reuse it.  [sum M, H] float32 on the device.
    model.training, StepPlan.keep_last and StepPlan.last are left as found."""
    H = int(model.encoder.hidden_size)
    out = []
    with _eval_keeping_vectors(model):
        for r_batch, p_batch, scope, _targets, add_features in batches:
            if len(scope) == 0:
                continue
            _, v = _forward_with_vectors(model, r_batch, p_batch, add_features, gpu)
            out.append(v if include_features else v[:, :H].contiguous())
    if not out:
        dev = torch.device("cuda", torch.cuda.current_device() if gpu is None else gpu)
        return torch.zeros(0, H, dtype=torch.float32, device=dev)
    return torch.cat(out, 0)


class ReactionBank:
    """The reactions a model was trained on, as the search needs them: vectors [N, H], sqnorm [N] (row_sqnorm of them),
    targets [N] float32 and group [N] int32 = the running index of the query a row belongs to (so that "neighbours from
    OTHER queries" and leave-one-query-out of the bank against itself are one knn call)."""

    def __init__(self, vectors: torch.Tensor, targets, group, sqnorm: Optional[torch.Tensor] = None):
        self.vectors = _embed.rows(vectors, "vectors", "ReactionBank").contiguous()
        dev, N = self.vectors.device, self.vectors.shape[0]
        self.targets = torch.as_tensor(targets).reshape(-1).to(device=dev, dtype=torch.float32)
        if self.targets.numel() != N:
            raise ValueError(f"ReactionBank: {self.targets.numel()} targets for {N} rows")
        self.group = _embed.group(group, N, dev, "group", "ReactionBank")
        self.sqnorm = row_sqnorm(self.vectors) if sqnorm is None else sqnorm.to(device=dev, dtype=torch.float32).reshape(-1)
        if self.sqnorm.numel() != N:
            raise ValueError(f"ReactionBank: {self.sqnorm.numel()} norms for {N} rows")

    def __len__(self) -> int:
        return int(self.vectors.shape[0])

    @classmethod
    def from_batches(cls, model, batches: Sequence, gpu, include_features: bool = False) -> "ReactionBank":
        batches = [b for b in batches if len(b[2]) > 0]
        vec = reaction_vectors(model, batches, gpu, include_features)
        targets = torch.cat([torch.as_tensor(b[3]).reshape(-1).to(torch.float32) for b in batches]) if batches else torch.zeros(0)
        sizes = [int(c) for b in batches for c in b[2]]
        group = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes, dtype=torch.int64))
        return cls(vec, targets, group)

    def save(self, path) -> None:
        torch.save(dict(vectors=self.vectors.cpu(), sqnorm=self.sqnorm.cpu(), targets=self.targets.cpu(),
                        group=self.group.cpu()), path)

    @classmethod
    def load(cls, path, device) -> "ReactionBank":
        d = torch.load(path, map_location="cpu")
        dev = torch.device(device)
        return cls(d["vectors"].to(dev), d["targets"], d["group"], sqnorm=d["sqnorm"])

    def query(self, vectors: torch.Tensor, k: int, group=None):
        """(dist [M, k], idx [M, k] int64, targets [M, k]) of the k nearest bank rows; `group` (one query index per row)
        excludes the bank rows of the same query; targets of padding slots (idx -1) are NaN."""
        bg = None if group is None else self.group
        dist, idx = knn(vectors, self.vectors, k, q_group=group, b_group=bg, bank_sqnorm=self.sqnorm)
        if len(self) == 0:
            return dist, idx, torch.full_like(dist, float("nan"))
        t = self.targets[idx.clamp_min(0)]
        return dist, idx, torch.where(idx >= 0, t, torch.full_like(t, float("nan")))


def latent_distance(bank: ReactionBank, vectors: torch.Tensor, k: int, group=None) -> torch.Tensor:
    """Per row, the mean of sqrt(d) over the (at most k) neighbours found in the bank; +inf when there are none."""
    dist, idx, _ = bank.query(vectors, k, group)
    found = idx >= 0
    n = found.sum(dim=1)
    s = torch.where(found, dist.sqrt(), torch.zeros_like(dist)).sum(dim=1)
    return torch.where(n > 0, s / n.clamp_min(1).to(s.dtype), torch.full_like(s, float("inf")))


def evaluate_applicability(model, bank: ReactionBank, test_batches: Sequence[dict], path_checkpoints, gpu: int, k: int = 8,
                           target_name: str = "ea", fractions=U.DEFAULT_FRACTIONS, method: str = "knn", gaussian=None) -> dict:
    """Applicability domain of a trained model: the latent distance of every test candidate to `bank` against its error.
    `test_batches` are the dicts main.test takes (r, p, scope, targets, add); the checkpoint is loaded and the targets are
    standardised as evaluate_uncertainty does.  One eval-mode forward per batch gives both the scores (column 0) and the
    reaction vectors.  Returns dict(distance [n], pred [n], targets [n] (standardised), scope, calibration =
    uncertainty_calibration(pred, targets, distance, fractions) - Spearman rho of error and distance plus the
    error-confidence curve -, qstats [Q, 12] = eval.ranking_stats per query, query_distance [Q] = mean distance per query).
    A bank without rows gives +inf distances, which the calibration sorts like any other value.
    method 'mahalanobis'  puts sqrt(d^2), d^2 the squared Mahalanobis distance to the bank's Gaussian,
    where the latent distance goes; `gaussian` is a fitted latent_gaussian.EmbeddingGaussian (None: fitted from the bank's
    vectors with its defaults) and k is not used.  Everything else is the same."""
    if not isinstance(path_checkpoints, (str, bytes)) and hasattr(path_checkpoints, "__len__"):
        raise ValueError("evaluate_applicability takes one checkpoint path")
    if method not in APPLICABILITY_METHODS:
        raise ValueError(f"evaluate_applicability: method must be one of {APPLICABILITY_METHODS} (got {method!r})")
    if gaussian is not None and method != "mahalanobis":
        raise ValueError("evaluate_applicability: `gaussian` belongs to method 'mahalanobis'")
    U._check_fractions(fractions)
    f = U._standardizer(U._scaler_of(path_checkpoints), target_name)
    batches = []
    for b in test_batches:
        y = np.asarray(torch.as_tensor(b["targets"]).cpu(), np.float64).reshape(-1)
        if len(b["scope"]) > 0:
            batches.append((b["r"], b["p"], b["scope"], torch.tensor(f(y), dtype=torch.float32), b.get("add")))
    if not batches:
        raise ValueError("no queries to evaluate")
    model = model.cuda(gpu)
    load_checkpoint(path_checkpoints, model, map_location="cpu")
    H = int(model.encoder.hidden_size)
    if bank.vectors.shape[1] != H:
        raise ValueError(f"the bank holds vectors of width {bank.vectors.shape[1]}, the model's are {H}")
    if method == "mahalanobis" and gaussian is None:
        from .latent_gaussian import EmbeddingGaussian
        gaussian = EmbeddingGaussian.from_bank(bank)
    preds, dists, stats = [], [], []
    with _eval_keeping_vectors(model):
        for r_batch, p_batch, scope, targets, add in batches:
            out, vec = _forward_with_vectors(model, r_batch, p_batch, add, gpu)
            vec = vec[:, :H]
            pred = U._first_column(out)
            preds.append(pred)
            dists.append(latent_distance(bank, vec, k) if method == "knn" else gaussian.mahalanobis(vec).sqrt())
            stats.append(E.ranking_stats(pred, scope, targets, gpu, 0.25)[0])
    pred, distance = torch.cat(preds), torch.cat(dists)
    targets = torch.cat([b[3].reshape(-1) for b in batches]).to(pred.device)
    scope = [int(c) for b in batches for c in b[2]]
    seg = torch.repeat_interleave(torch.arange(len(scope), device=pred.device), torch.tensor(scope, device=pred.device))
    qd = torch.zeros(len(scope), dtype=torch.float64, device=pred.device).index_add_(0, seg, distance.double())
    qd = qd / torch.tensor(scope, dtype=torch.float64, device=pred.device)
    return dict(distance=distance, pred=pred, targets=targets, scope=scope,
                calibration=U.uncertainty_calibration(pred, targets, distance, fractions),
                qstats=torch.cat(stats, 0), query_distance=qd)


def split_overlap(bank: ReactionBank, vectors: torch.Tensor, rel_tol: float = 1e-6) -> dict:
    """Leakage between a bank and another split: dict(count, rows [count] int64, nearest [M] int64, dist [M]) where `rows`
    are the rows of `vectors` whose nearest bank row lies within d <= rel_tol * (|q|^2 + |b|^2)."""
    dist, idx = knn(vectors, bank.vectors, 1, bank_sqnorm=bank.sqnorm)
    dist, idx = dist[:, 0], idx[:, 0]
    qn = row_sqnorm(vectors) if vectors.shape[0] > 0 else dist
    bn = bank.sqnorm[idx.clamp_min(0)] if len(bank) > 0 else torch.zeros_like(dist)
    hit = (idx >= 0) & (dist <= float(rel_tol) * (qn + bn))
    rows = hit.nonzero().reshape(-1)
    return dict(count=int(rows.numel()), rows=rows, nearest=idx, dist=dist)


# ------------------------------------------------------------------------------------------------ selection
def _per_row(t, rows: int, dev, name: str) -> torch.Tensor:
    return _embed.per_row(t, rows, dev, name, "kcenter_greedy")


def kcenter_greedy(vectors: torch.Tensor, n: int, init_dist=None, weight=None) -> dict:
    """Greedy k-center (farthest-first) selection of `n` rows of `vectors` [P, H]: dict(picks [n] int64, gain [n] float32,
    min_dist [P] float32, assign [P] int64) - rr_kcenter_f32, include/reactranker_hip.h states the arithmetic.

    min_dist starts as init_dist (squared distance of every row to what is labelled already; None: +inf) and assign as -1; a
    row that holds a NaN or an infinity gets min_dist NaN and is never picked.  Round t takes the row with the largest score
    weight[i] * min_dist[i] (weight None: min_dist[i]) among the rows not taken yet whose min_dist is not NaN and, with
    weights, whose weight lies in (0, +inf).  TIES go to the LOWER row index, so the picks are the same on every run.  Then
    every row r with d(r, pick) < min_dist[r] gets that distance and assign[r] = t.  When no row is eligible the remaining
    slots hold picks = -1, gain = -1.  gain[t] is the score the pick had when it was taken; min_dist / assign describe the
    state after the last round (the coverage radius squared is min_dist.max(), the clustering is assign).
    The rounds use d(r, c) = sum_h (x[r,h] - x[c,h])^2 in f32 (a picked row and its exact duplicates end at exactly 0);
    an init_dist that comes from knn() carries knn's |q|^2 + |b|^2 - 2 q.b arithmetic instead - both are kept as given and
    compared as numbers.
    `vectors`: float32 GPU matrix with contiguous rows, any pitch.  Scratch comes from torch's allocator on the current
    stream, and the call is ordered on that stream: n + 1 launches, no host synchronisation in between.
    ValueError - before any launch - for CPU tensors, width 0, n outside [0, 65536], or an init_dist / weight that is not
    P float32 values on the same device."""
    _embed.matrix(vectors, "vectors", "kcenter_greedy")
    nn = int(n)
    if nn != n or not (0 <= nn <= MAX_PICKS):
        raise ValueError(f"kcenter_greedy: n must be an integer in [0, {MAX_PICKS}] (got {n!r})")
    if vectors.shape[1] < 1:
        raise ValueError("kcenter_greedy: rows of width 0")
    x = _embed.rows(vectors, "vectors", "kcenter_greedy")
    P, H, dev = x.shape[0], x.shape[1], x.device
    if P > 2 ** 31 - 1:
        raise ValueError(f"kcenter_greedy: {P} rows (at most 2^31 - 1)")
    init = None if init_dist is None else _per_row(init_dist, P, dev, "init_dist")
    w = None if weight is None else _per_row(weight, P, dev, "weight")
    picks = torch.empty(nn, dtype=torch.int32, device=dev)
    gain = torch.empty(nn, dtype=torch.float32, device=dev)
    min_dist = torch.empty(P, dtype=torch.float32, device=dev)
    assign = torch.empty(P, dtype=torch.int32, device=dev)
    if P > 0 or nn > 0:
        with torch.cuda.device(dev):
            ws, nbytes = _embed.scratch("rr_kcenter_workspace_bytes", dev, P, nn)
            one = _embed.placeholder(dev)
            check(lib().rr_kcenter_f32(ptr(x) if P > 0 else ptr(one), _embed.pitch(x), P, H, nn, ptr(init), ptr(w),
                                       ptr(picks) if nn > 0 else ptr(one), ptr(gain) if nn > 0 else ptr(one),
                                       ptr(min_dist) if P > 0 else ptr(one), ptr(assign) if P > 0 else ptr(one), ptr(ws),
                                       nbytes, stream()), "rr_kcenter_f32")
    return dict(picks=picks.to(torch.int64), gain=gain, min_dist=min_dist, assign=assign.to(torch.int64))


def acquire(model, bank: ReactionBank, pool_batches: Sequence, n: int, gpu, weight=None) -> dict:
    """Which `n` candidates of a pool to label next: kcenter_greedy over the model's reaction vectors of `pool_batches`
    ((r, p, scope, targets, add_features) tuples as reaction_vectors takes them; the targets are ignored and may be None;
    batches without queries are skipped), started from init_dist = the squared distance of every pool row to its nearest row
    of `bank` (knn with k = 1 and bank.sqnorm; an empty bank gives +inf everywhere).  One eval-mode forward per batch.
    weight: None (pure coverage), a [rows] float32 tensor on the model's device (e.g. the std of
    uncertainty.mc_dropout_predict), or 'std': the per-candidate predictive std of the model's distributional head, read
    from the same forward as uncertainty.distribution_predict reads it (ValueError for a head that has none).
    Returns dict(rows [n] int64 into the concatenated pool; batch, query, candidate [n] int64: the batch (counting only
    batches with queries), the query inside it and the candidate inside that query; gain [n]; radius_before, radius_after:
    0-dim tensors, sqrt of the largest min_dist before and after the picks over the rows whose vectors are finite (NaN when
    there is no such row, +inf before the picks with an empty bank); min_dist [rows]; assign [rows]; init_dist [rows]: what
    the rounds started from).  Padding picks (rows = -1) have batch = query = candidate = -1.
    Ties go to the lower row index (kcenter_greedy).  init_dist carries knn's distance arithmetic (norms minus twice the dot
    product), the rounds the difference form.  knn's form leaves a rounding residue (a few 2^-21 at unit scale) between a row
    and itself, so one case is set exactly: a pool row whose nearest bank row holds the same bits starts at 0 - a reaction
    that is labelled already scores 0 and is taken last, in index order, never on that residue.
    model.training, StepPlan.keep_last and StepPlan.last are left as found."""
    batches = [b for b in pool_batches if len(b[2]) > 0]
    kind = None
    if isinstance(weight, str):
        if weight != "std":
            raise ValueError(f"acquire: weight must be None, a tensor or 'std' (got {weight!r})")
        kind = U._kind_of(model, None)
    H = int(model.encoder.hidden_size)
    if bank.vectors.shape[1] != H:
        raise ValueError(f"the bank holds vectors of width {bank.vectors.shape[1]}, the model's are {H}")
    vecs, stds = [], []
    with _eval_keeping_vectors(model):
        for r_batch, p_batch, scope, _targets, add in batches:
            out, vec = _forward_with_vectors(model, r_batch, p_batch, add, gpu)
            vecs.append(vec[:, :H].contiguous())
            if kind is not None:
                zeros = torch.zeros(vec.shape[0], dtype=torch.float32)
                stds.append(U.analytic_stats(out, scope, zeros, kind, gpu=gpu)["std"])
    dev = bank.vectors.device
    vec = torch.cat(vecs, 0) if vecs else torch.zeros(0, H, dtype=torch.float32, device=dev)
    if kind is not None:
        weight = torch.cat(stds) if stds else torch.zeros(0, dtype=torch.float32, device=dev)
    init = None
    if len(bank) > 0 and vec.shape[0] > 0:
        dist, idx, _ = bank.query(vec, 1)
        dist, idx = dist[:, 0], idx[:, 0]
        # a pool row that IS its nearest bank row (the same bits) is at distance 0; knn's norms-minus-dot arithmetic leaves a
        # rounding residue there, on which reactions that are labelled already would otherwise be picked first
        labelled = (idx >= 0) & (vec == bank.vectors[idx.clamp_min(0)]).all(dim=1)
        init = torch.where(labelled, torch.zeros_like(dist), dist).contiguous()
    res = kcenter_greedy(vec, n, init_dist=init, weight=weight)
    rows, min_dist = res["picks"], res["min_dist"]
    finite = ~torch.isnan(min_dist)
    before = torch.full_like(min_dist, float("inf")) if init is None else init

    def radius(d):                                         # (no finite row: sqrt(-inf) is the NaN the docstring promises)
        if d.numel() == 0:
            return torch.full((), float("nan"), dtype=torch.float32, device=vec.device)
        return torch.where(finite, d, torch.full_like(d, float("-inf"))).max().sqrt()
    sizes = [[int(c) for c in b[2]] for b in batches]
    q_start = np.cumsum([0] + [c for s in sizes for c in s])[:-1]
    q_batch = [j for j, s in enumerate(sizes) for _ in s]
    q_index = [i for s in sizes for i in range(len(s))]
    if len(q_batch) > 0:
        as_dev = lambda a: torch.as_tensor(np.asarray(a, np.int64), device=rows.device)   # noqa: E731
        q_start, q_batch, q_index = as_dev(q_start), as_dev(q_batch), as_dev(q_index)
        q = (torch.bucketize(rows.clamp_min(0), q_start, right=True) - 1)
        none = torch.full_like(rows, -1)
        batch = torch.where(rows >= 0, q_batch[q], none)
        query = torch.where(rows >= 0, q_index[q], none)
        cand = torch.where(rows >= 0, rows - q_start[q], none)
    else:
        batch, query, cand = rows.clone(), rows.clone(), rows.clone()
    return dict(rows=rows, batch=batch, query=query, candidate=cand, gain=res["gain"], radius_before=radius(before),
                radius_after=radius(min_dist), min_dist=min_dist, assign=res["assign"], init_dist=before)
