"""float64 restatement of the LambdaRank loss (include/reactranker_hip.h: rr_lambdarank_fwd_f32), used by the
LambdaRank tests.  Written with torch so that autograd gives the gradient; the |delta NDCG| weights are built under no_grad:
they are constants.  A list is evaluated in row blocks, so one of 8192 candidates needs a few hundred MB, not several GB.

Per query, with k = C for ndcg_k == 0 and min(ndcg_k, C) otherwise:
  r_i     1-based rank of i by score, descending, ties by list position; the comparison is exact on the float32 scores
  D_i     1 / log2(1 + r_i) for r_i <= k, else 0
  g_i     exp(t_i - max_j t_j)
  maxDCG  sum_{p = 1..k} g_(p) / log2(1 + p), g_(p) the p-th largest gain
  w_ij    |g_i - g_j| |D_i - D_j| / maxDCG
  C_ij    softplus(-sigma (s_i - s_j)) for t_i > t_j, softplus(sigma (s_i - s_j)) for t_i < t_j, 0 for t_i == t_j
  loss_sum_q = sum_{i != j} w_ij C_ij,  pairs_q = 2 #{(i, j): t_i > t_j};  a query with pairs_q == 0 adds nothing."""
import numpy as np
import torch


def _softplus(x):
    """max(x, 0) + log1p(exp(-|x|)), which is what logaddexp(x, 0) evaluates - through logaddexp because autograd's
    derivative of the written-out form is wrong at x == 0 exactly (clamp passes 1, |x| passes 0: 1 instead of 1 / 2), and
    tied scores put every pair there."""
    return torch.logaddexp(x, torch.zeros_like(x))


def window(seed, scope):
    """Scores 2 * N(0, 1) in float32 and z-scored permutations as targets (the random windows of tests/test_gpu_losses.py)."""
    rng = np.random.default_rng(seed)
    m = sum(scope)
    score = (rng.standard_normal(m) * 2).astype(np.float32)
    targets = np.concatenate([rng.permutation(c) for c in scope]).astype(np.float32) if m else np.zeros(0, np.float32)
    targets = ((targets - targets.mean()) / (targets.std() + 1e-6)).astype(np.float32)
    return score, targets


def query_terms(score32, targets32, ndcg_k):
    """(D, g / maxDCG) of one query as float64 tensors; score32 / targets32 are float32 numpy vectors."""
    C = len(score32)
    k = C if ndcg_k == 0 else min(int(ndcg_k), C)
    order = np.argsort(-score32, kind="stable")                     # descending, ties by list position, exact on float32
    rank = np.empty(C, np.int64)
    rank[order] = np.arange(1, C + 1)
    D = np.where(rank <= k, 1.0 / np.log2(1.0 + rank.astype(np.float64)), 0.0)
    t = targets32.astype(np.float64)
    g = np.exp(t - t.max())
    ideal = np.sort(g)[::-1][:k]
    max_dcg = float(np.sum(ideal / np.log2(1.0 + np.arange(1, k + 1, dtype=np.float64))))
    return torch.from_numpy(D), torch.from_numpy(g / max_dcg)


def lambdarank(score, scope, targets, sigma=1.0, ndcg_k=0, block=256, dtype=torch.float64):
    """(loss_sum, pairs, d loss_sum / d score) over a window: python float, python int, float64 numpy vector.
    score / targets: float32 vectors (numpy or tensors) of sum(scope) entries.  dtype: the type the pair terms are evaluated
    and summed in (float32 shows what plain float32 arithmetic does to the same formulas)."""
    score32, targets32 = (np.array(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float32).reshape(-1)
                          for x in (score, targets))
    assert len(score32) == len(targets32) == sum(scope)
    total, pairs = 0.0, 0
    grad = np.zeros(len(score32), np.float64)
    off = 0
    for C in scope:
        C = int(C)
        s32, t32 = score32[off:off + C], targets32[off:off + C]
        t64 = torch.from_numpy(t32.astype(np.float64))
        npos = 0
        for r0 in range(0, C, block):
            npos += int((t64[r0:r0 + block, None] > t64[None, :]).sum())
        if npos > 0:
            with torch.no_grad():
                D, gn = query_terms(s32, t32, ndcg_k)
                D, gn = D.to(dtype), gn.to(dtype)
            t = t64.to(dtype)
            s = torch.from_numpy(s32.astype(np.float64)).to(dtype).requires_grad_(True)
            for r0 in range(0, C, block):
                sl = slice(r0, min(r0 + block, C))
                with torch.no_grad():
                    w = (gn[sl, None] - gn[None, :]).abs() * (D[sl, None] - D[None, :]).abs()
                    up = (t[sl, None] > t[None, :]).to(dtype)
                    down = (t[sl, None] < t[None, :]).to(dtype)
                x = sigma * (s[sl, None] - s[None, :])
                part = (w * (up * _softplus(-x) + down * _softplus(x))).sum()
                g, = torch.autograd.grad(part, s)
                total += float(part.detach().double())
                grad[off:off + C] += g.double().numpy()
            pairs += 2 * npos
        off += C
    return total, pairs, grad
