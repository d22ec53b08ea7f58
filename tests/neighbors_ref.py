"""numpy float64 oracle of the nearest-neighbour search (reactranker_amd.neighbors / rr_knn_f32).

  distances64   D64[m, n] = sum_h (q[m, h] - b[n, h])^2 by brute force, one query row at a time
  excluded      pairs with q_group[m] == b_group[n] >= 0, and pairs whose distance is a NaN
  knn_ref       per row the k smallest non-excluded bank rows under the stable order (D64 ascending, n ascending), the
                remaining slots padded with dist = +inf, idx = -1
  tol           the derived bound on the f32 kernel's distance: 2 (H + 3) 2^-24 (|q|^2 + |b|^2), norms in float64

The bound is the worst-case rounding of three H-term f32 sums of non-negative or norm-bounded products (|q|^2, |b|^2 and
q.b, each within (H + 1) u of its exact value relative to the sum of magnitudes, u = 2^-24, and |2 q.b| <= |q|^2 + |b|^2) plus
the two additions that join them; it holds for every summation order, and clamping at zero only moves a value towards the
truth (the exact distance is >= 0)."""
import numpy as np

U32 = 2.0 ** -24


def distances64(q, b):
    q, b = np.asarray(q, np.float64), np.asarray(b, np.float64)
    D = np.empty((q.shape[0], b.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(q.shape[0]):
            D[m] = ((b - q[m][None, :]) ** 2).sum(axis=1)
    return D


def excluded(D, q_group=None, b_group=None):
    ex = np.isnan(D)
    if q_group is not None:
        qg, bg = np.asarray(q_group, np.int64).reshape(-1), np.asarray(b_group, np.int64).reshape(-1)
        ex |= (qg[:, None] == bg[None, :]) & (qg[:, None] >= 0)
    return ex


def knn_from_distances(D, k, ex=None):
    M, N = D.shape
    dist = np.full((M, k), np.inf, np.float64)
    idx = np.full((M, k), -1, np.int64)
    for m in range(M):
        keep = np.arange(N) if ex is None else np.nonzero(~ex[m])[0]
        order = keep[np.argsort(D[m, keep], kind="stable")][:k]          # stable: ties keep ascending n
        dist[m, :order.size] = D[m, order]
        idx[m, :order.size] = order
    return dist, idx


def knn_ref(q, b, k, q_group=None, b_group=None):
    """(dist [M, k] float64, idx [M, k] int64, D64 [M, N])"""
    D = distances64(q, b)
    dist, idx = knn_from_distances(D, k, excluded(D, q_group, b_group))
    return dist, idx, D


def sqnorm64(x):
    x = np.asarray(x, np.float64)
    return (x * x).sum(axis=1)


def tol(q, b):
    """[M, N] bound on |d_f32(m, n) - D64[m, n]|"""
    H = np.asarray(q).shape[1]
    return 2.0 * (H + 3) * U32 * (sqnorm64(q)[:, None] + sqnorm64(b)[None, :])


def latent_distance_ref(dist, idx):
    """mean of sqrt(d) over the neighbours found; +inf when there are none"""
    out = np.full(dist.shape[0], np.inf)
    for m in range(dist.shape[0]):
        f = idx[m] >= 0
        if f.any():
            out[m] = np.sqrt(dist[m, f]).mean()
    return out
