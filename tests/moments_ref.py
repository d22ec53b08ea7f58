"""numpy restatement of the embedding Gaussian (reactranker_amd.latent_gaussian, rr_col_moments_f64 / rr_center_project_f32,
DESIGN.md section 4j): the row filter, the chunk function, the moments in np.longdouble, the eigen post-processing and both
projections in float64 - and the error bounds the GPU tests hold the kernels to.  Nothing here touches the device or the library.

Bounds (u = 2^-53 for the moments, 2^-24 for the projection; every (1 + u)^k is covered by the factor 1.01, N u << 1):
  mean      the chain of a column is at most N additions of used rows (additions of 0.0 are exact), 16 + C joins and one division:
            |mean' - mean| <= (N + 20) u a_h =: d_h,  a_h = mean |x[n,h]| over the used rows.
  scatter   c'_n = fl(x_n - mean') = (c_n - delta)(1 + e), |delta_h| <= d_h, |e| <= u.  Because sum_n c_n = 0 exactly, the shift by
            delta changes S_ij by exactly N delta_i delta_j.  Rounding of the two factors: 2 u per product; the chain of a tile
            element is at most L products (fused or rounded: 1 or 2 roundings per term) and L + C additions, L <= N, C <= 64:
            |S' - S|_ij <= 1.01 (N + 68) u A_ij + N d_i d_j,
            A_ij = sum_n |c_ni| |c_nj| + d_i sum_n |c_nj| + d_j sum_n |c_ni| + N d_i d_j      (the sum over |c'| bounded by |c| + d)
  project   t = fl(x - center): 1 rounding; product: 1; the chain's additions: at most H (zeros added exactly): (H + 2) u, doubled
            as DESIGN 4g doubles its bound:  |y' - y|_r <= 2 (H + 3) u sum_h |x_h - center_h| |W_hr| =: b_r
  sq        sq' = chain of fl(y'^2): |y'^2 - y^2| <= 2 |y| b + b^2 per term; the square 1 rounding, at most R / 4 + 2 additions per
            chain and join, bounded by R + 2, doubled:  |sq' - sq| <= sum_r (2 |y_r| b_r + b_r^2) + 2 (R + 3) u sum_r (|y_r| + b_r)^2"""
import numpy as np

LD = np.longdouble
U53, U24 = 2.0 ** -53, 2.0 ** -24
MAX_H = 1024
MAX_CHUNKS, CHUNK_ROWS, SLAB_BUDGET, TILE = 64, 1024, 1 << 28, 64


def used_rows(x):
    """mask of the rows every value of which is finite"""
    x = np.asarray(x)
    return np.isfinite(x).all(axis=1) if x.size or x.shape[0] else np.zeros(0, bool)


def chunks(N, H):
    """C = max(1, min(64, ceil(N / 1024), floor(2^28 / (8 Hp^2)))), Hp = H rounded up to a multiple of 64"""
    hp = -(-H // TILE) * TILE
    return int(max(1, min(MAX_CHUNKS, -(-N // CHUNK_ROWS), SLAB_BUDGET // (8 * hp * hp))))


def chunk_boundaries(H, which=(1, 2)):
    """the largest row count that still has `k` chunks, k in `which` (so N and N + 1 lie on either side of a boundary)"""
    out = []
    for k in which:
        n = k * CHUNK_ROWS
        assert chunks(n, H) == k and chunks(n + 1, H) == k + 1, (H, k)
        out.append(n)
    return out


def moments_ref(x):
    """(mean [H], scatter [H, H], n_used) in np.longdouble over the used rows; zeros when there are none"""
    x = np.asarray(x, np.float32)
    H = x.shape[1]
    xu = x[used_rows(x)].astype(LD)
    n = xu.shape[0]
    if n == 0:
        return np.zeros(H, LD), np.zeros((H, H), LD), 0
    mean = xu.sum(axis=0) / LD(n)
    c = xu - mean
    return mean, np.einsum("ni,nj->ij", c, c), n


def cov_ref(x, ddof=1):
    mean, sc, n = moments_ref(x)
    return mean, (sc / LD(n - ddof) if n - ddof > 0 else np.full_like(sc, np.nan)), n


def moments_bounds(x):
    """(bound on |mean' - mean| [H], bound on |S' - S| [H, H]) as the module docstring derives them"""
    x = np.asarray(x, np.float32)
    xu = x[used_rows(x)].astype(np.float64)
    N_all, n = x.shape[0], xu.shape[0]
    H = x.shape[1]
    if n == 0:
        return np.zeros(H), np.zeros((H, H))
    d = 1.01 * (N_all + 20) * U53 * np.abs(xu).mean(axis=0)
    c = np.abs(xu - xu.mean(axis=0))
    s1 = c.sum(axis=0)
    A = c.T @ c + d[:, None] * s1[None, :] + d[None, :] * s1[:, None] + n * np.outer(d, d)
    return d, 1.01 * (N_all + 68) * U53 * A + n * np.outer(d, d)


def eigen_ref(cov, shrinkage=0.0, rank=None, eig_floor=None):
    """latent_gaussian.eigen_model in numpy: eigenvalues descending (clamped at 0, then shrunk), each eigenvector's
    largest-magnitude entry positive (ties: the lower index), the kept rank, the explained variance ratio"""
    cov = np.asarray(cov, np.float64)
    H = cov.shape[0]
    lam, vec = np.linalg.eigh(cov)
    lam, vec = np.maximum(lam[::-1], 0.0), vec[:, ::-1]
    lam = (1.0 - shrinkage) * lam + shrinkage * lam.mean()
    big = np.abs(vec).argmax(axis=0)
    sign = np.sign(vec[big, np.arange(H)])
    sign[sign == 0] = 1.0
    vec = vec * sign
    floor = H * U24 if eig_floor is None else eig_floor
    keep = int((lam > floor * lam[0]).sum()) if lam[0] > 0 else 0
    if rank is not None:
        keep = min(keep, rank)
    total = lam.sum()
    return dict(eigenvalues=lam, components=np.ascontiguousarray(vec), rank=keep,
                explained_variance_ratio=lam / total if total > 0 else np.zeros_like(lam))


def fit_ref(x, shrinkage=0.0, rank=None, eig_floor=None):
    """the fitted model in float64: mean, cov, the eigen model, components [H, r] and whitener [H, r] = components / sqrt(lambda)"""
    mean, cov, n = cov_ref(x, 1)
    e = eigen_ref(cov.astype(np.float64), shrinkage, rank, eig_floor)
    r = e["rank"]
    comp = e["components"][:, :r]
    return dict(e, mean=mean.astype(np.float64), cov=cov.astype(np.float64), n=n, components_r=comp,
                whitener=comp / np.sqrt(e["eigenvalues"][:r]))


def project_ref(x, center, W):
    """(y [N, R], sq [N]) in float64"""
    x = np.asarray(x, np.float64)
    t = x if center is None else x - np.asarray(center, np.float64)
    y = t @ np.asarray(W, np.float64)
    return y, (y * y).sum(axis=1)


def project_bounds(x, center, W):
    """(bound on |y' - y| [N, R], bound on |sq' - sq| [N])"""
    x = np.asarray(x, np.float64)
    t = np.abs(x if center is None else x - np.asarray(center, np.float64))
    W = np.asarray(W, np.float64)
    H, R = W.shape
    b = 2 * (H + 3) * U24 * (t @ np.abs(W))
    y = np.abs(project_ref(x, center, W)[0])
    return b, (2 * y * b + b * b).sum(axis=1) + 2 * (R + 3) * U24 * ((y + b) ** 2).sum(axis=1)


def sq_chain32(y):
    """sq of rr_center_project_f32 from a float32 y, bit for bit: chain q owns the columns r with (r mod 16) // 4 == q, ascending,
    acc = acc + fl(y * y); sq = (chain 0 + chain 2) + (chain 1 + chain 3)"""
    y = np.asarray(y, np.float32)
    N, R = y.shape
    acc = np.zeros((4, N), np.float32)
    for r in range(R):
        q = (r % 16) // 4
        acc[q] = (acc[q] + (y[:, r] * y[:, r]).astype(np.float32)).astype(np.float32)
    return ((acc[0] + acc[2]).astype(np.float32) + (acc[1] + acc[3]).astype(np.float32)).astype(np.float32)


def mahalanobis_ref(x, fit):
    return project_ref(x, fit["mean"], fit["whitener"])[1]
