"""numpy oracle of the sphere-exclusion clustering and the cluster-held-out splits (reactranker_amd.clusters,
rr_radius_count_f32 / rr_sphere_exclusion_f32).  Restatements of include/reactranker_hip.h:

  count64       neighbours within r2 by brute-force float64 distances (tests/neighbors_ref.py: distances64, excluded)
  exclusion64   the rounds on float64 distances sum_h (x[i,h] - x[c,h])^2: what the clustering means
  exclusion32   the rounds on tests/selection_ref.py's chain32, the kernel's f32 chain: what the kernel's BITS are
  replay64      along GIVEN centres: the float64 key order held at every round (each centre had the largest key among the rows
                that were unassigned when it was taken)
  folds_ref     the split rule of cluster_split / cluster_kfold, written out row by row

exclusion64 / exclusion32 return dict(labels [P] int64, centres [n] int64 (padding -1), by_index [n] bool); by_index[t] says
that more than one unassigned row held round t's largest key, so that the index decided."""
import numpy as np

from tests import neighbors_ref as R
from tests import selection_ref as S


def r2_of(radius):
    """the package's rule: float32(float64(radius) ** 2)"""
    with np.errstate(over="ignore"):
        return np.float32(np.float64(radius) ** 2)


def count64(q, b, r2, q_group=None, b_group=None):
    D = R.distances64(q, b)
    with np.errstate(invalid="ignore"):
        return ((D <= np.float64(r2)) & ~R.excluded(D, q_group, b_group)).sum(axis=1).astype(np.int64)


def _exclusion(x, r2, key, n, dist, dtype, first_labels=None):
    x = np.asarray(x)
    P = x.shape[0]
    labels = np.full(P, -1, np.int64)
    if P > 0:
        labels[~np.isfinite(x).all(axis=1)] = -2
    key = np.zeros(P, np.int64) if key is None else np.asarray(key, np.int64).reshape(-1)
    assert key.shape == (P,)
    centres, by_index = [], []
    t = 0
    while n is None or t < n:
        idx = np.nonzero(labels == -1)[0]
        if idx.size == 0:
            if n is None:
                break
            centres.append(-1)
            by_index.append(False)
            t += 1
            continue
        k = key[idx]
        c = idx[np.argmax(k)]                                         # the first of equal maxima: the lowest index
        by_index.append(bool((k == k.max()).sum() > 1))
        centres.append(int(c))
        d = dist(x, c).astype(dtype)
        with np.errstate(invalid="ignore"):
            inside = (labels == -1) & (d <= dtype(r2))
        assert inside[c]
        labels[inside] = t
        t += 1
    return dict(labels=labels, centres=np.asarray(centres, np.int64), by_index=np.asarray(by_index, bool))


def exclusion64(x, r2, key=None, n=None):
    """n None: until no row is left at -1 (centres has one entry per cluster); n given: exactly n rounds, padded with -1"""
    return _exclusion(x, r2, key, n, S.dist64, np.float64)


def exclusion32(x, r2, key=None, n=None):
    return _exclusion(x, r2, key, n, S.chain32, np.float32)


def replay64(x, centres, labels, key=None):
    """Walk the GIVEN rounds: (dist64 of every member to its centre [P] (NaN for labels < 0), and per round whether the centre
    held the largest key - ties by the lowest index - among the rows with labels >= t or == -1, i.e. unassigned at round t)"""
    x = np.asarray(x, np.float64)
    P = x.shape[0]
    key = np.zeros(P, np.int64) if key is None else np.asarray(key, np.int64).reshape(-1)
    member_d = np.full(P, np.nan)
    held = np.zeros(len(centres), bool)
    for t, c in enumerate(centres):
        open_ = np.nonzero((labels >= t) | (labels == -1))[0]
        if c < 0:
            held[t] = open_.size == 0
            continue
        best = open_[np.argmax(key[open_])]
        held[t] = best == c
        rows = labels == t
        member_d[rows] = S.dist64(x, c)[rows]
    return member_d, held


def folds_ref(labels, targets, seed):
    """the split rule row by row: clusters by size descending (ties: a seeded permutation's rank), each to the fold with the
    largest remaining deficit against targets[f] * (rows with labels >= 0), ties to the lowest fold; negative labels: -1"""
    labels = np.asarray(labels, np.int64).reshape(-1)
    ids = sorted(set(labels[labels >= 0].tolist()))
    sizes = {c: int((labels == c).sum()) for c in ids}
    rank = np.random.default_rng(int(seed)).permutation(len(ids))
    order = sorted(range(len(ids)), key=lambda j: (-sizes[ids[j]], rank[j]))
    total = float(sum(sizes.values()))
    want = [float(t) * total for t in targets]
    have = [0.0] * len(want)
    fold_of = {}
    for j in order:
        deficit = [w - h for w, h in zip(want, have)]
        f = deficit.index(max(deficit))
        fold_of[ids[j]] = f
        have[f] += sizes[ids[j]]
    return np.asarray([fold_of[c] if c >= 0 else -1 for c in labels.tolist()], np.int64)
