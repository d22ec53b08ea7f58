"""numpy oracle of the greedy k-center selection (reactranker_amd.neighbors.kcenter_greedy / rr_kcenter_f32, DESIGN.md section
4h).  Two restatements of the rounds in include/reactranker_hip.h:

  greedy64   brute-force float64 distances sum_h (x[r,h] - x[c,h])^2: what the selection means
  chain32    the kernel's f32 chain in numpy float32 - columns in groups of four, group g on lane g mod 64, groups and columns
             ascending (acc = acc + t * t, each operation rounded), the 64 chains joined by the butterfly over lane distances
             32, 16, 8, 4, 2, 1 - and greedy32, the rounds on top of it in float32: what the kernel's BITS are
  replay64   the float64 state along a GIVEN sequence of picks: per round the float64 score of the row that was picked and the
             best float64 score any eligible row had (for the bound on random floats)

Both greedy functions return dict(picks [n] int64, gain [n], min_dist [P], assign [P] int64, tied [n] bool); tied[t] says that
more than one eligible row held round t's best score, so that the index decided.  gamma(H) = 2 (H + 3) 2^-24 bounds the
relative error of an f32 score: three roundings per term (difference, square, addition), at most H - 1 more per sum of
non-negative terms in any order, one for the weight; doubled, as tests/neighbors_ref.py doubles its bound."""
import numpy as np

U32 = 2.0 ** -24


def gamma(H):
    return 2.0 * (H + 3) * U32


def dist64(x, c):
    """[P] float64 distances of every row to row c"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((x - x[c][None, :]) ** 2).sum(axis=1)


def chain32(x, c):
    """[P] float32 distances of every row to row c by the kernel's chain"""
    x = np.asarray(x, np.float32)
    P, H = x.shape
    groups = (H + 3) // 4
    lane = np.arange(64)
    acc = np.zeros((P, 64), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range((groups + 63) // 64):
            for e in range(4):
                h = 4 * (lane + 64 * j) + e
                on = h < H
                t = x[:, h[on]] - x[c, h[on]][None, :]
                acc[:, on] = acc[:, on] + t * t
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lane ^ off]
    assert acc.dtype == np.float32
    return acc[:, 0].copy()


def _state(x, init_dist, weight, dtype):
    x = np.asarray(x)
    P = x.shape[0]
    md = np.full(P, np.inf, dtype) if init_dist is None else np.array(init_dist, dtype).reshape(-1)
    assert md.shape == (P,)
    md[~np.isfinite(x).all(axis=1)] = np.nan
    w = None if weight is None else np.array(weight, dtype).reshape(-1)
    ok = np.ones(P, bool) if w is None else (w > 0) & (w < np.inf)
    return md, w, ok


def _greedy(x, n, init_dist, weight, dist, dtype):
    md, w, ok = _state(x, init_dist, weight, dtype)
    P = md.shape[0]
    picks, gain = np.full(n, -1, np.int64), np.full(n, -1.0, dtype)
    assign, taken, tied = np.full(P, -1, np.int64), np.zeros(P, bool), np.zeros(n, bool)
    for t in range(n):
        idx = np.nonzero(~taken & ~np.isnan(md) & ok)[0]
        if idx.size == 0:
            continue
        with np.errstate(invalid="ignore"):
            s = md[idx] if w is None else w[idx] * md[idx]
        assert s.dtype == dtype and not np.isnan(s).any()
        best = idx[np.argmax(s)]                                      # the first of equal maxima: the lowest index
        tied[t] = (s == s.max()).sum() > 1
        picks[t], gain[t], taken[best] = best, s.max(), True
        d = dist(x, best).astype(dtype)
        with np.errstate(invalid="ignore"):
            closer = d < md                                           # false for a NaN on either side
        md[closer] = d[closer]
        assign[closer] = t
    return dict(picks=picks, gain=gain, min_dist=md, assign=assign, tied=tied)


def greedy64(x, n, init_dist=None, weight=None):
    return _greedy(x, n, init_dist, weight, dist64, np.float64)


def greedy32(x, n, init_dist=None, weight=None):
    return _greedy(x, n, init_dist, weight, chain32, np.float32)


def replay64(x, picks, init_dist=None, weight=None):
    """(score64 of the picked row [n], best eligible score64 [n]) along `picks` (which must name eligible rows, -1 only once
    no row is eligible)"""
    md, w, ok = _state(x, init_dist, weight, np.float64)
    taken = np.zeros(md.shape[0], bool)
    got, best = np.full(len(picks), -1.0), np.full(len(picks), -1.0)
    for t, p in enumerate(picks):
        elig = ~taken & ~np.isnan(md) & ok
        if p < 0:
            assert not elig.any(), f"round {t}: padding while rows were eligible"
            continue
        assert elig[p], f"round {t}: row {p} was not eligible"
        with np.errstate(invalid="ignore"):
            s = md if w is None else w * md
        got[t], best[t] = s[p], s[elig].max()
        taken[p] = True
        d = dist64(x, p)
        with np.errstate(invalid="ignore"):
            closer = d < md
        md[closer] = d[closer]
    return got, best
