"""float64 restatement of the soft ranks and of ApproxNDCG (include/reactranker_hip.h: rr_soft_rank_fwd_f32,
rr_approx_ndcg_fwd_f32), used by the ApproxNDCG tests.  There is no reference code for this loss: the definitions below are
the specification.  Written with torch so that autograd gives the gradient; a list is evaluated in row blocks, so one of 8192
candidates needs a few hundred MB, not several GB.

Per query of C candidates with float32 scores s, targets t and a temperature T > 0; k = C for ndcg_k == 0, else min(ndcg_k, C):
  u_ij    (s_j - s_i) / T
  r_i     1 + sum_{j != i} sigmoid(u_ij)
  g_i     exp(t_i - max_j t_j);  maxDCG = sum_{p = 1..k} g_(p) / log2(1 + p);  G_i = g_i / maxDCG   (lambdarank_ref.query_terms)
  psi(r)  1 / log2(1 + r) for k == C, sigmoid(k + 1/2 - r) / log2(1 + r) for k < C
  loss_q  1 - sum_i G_i psi(r_i);  a query is ranked when two of its targets differ, an unranked one adds nothing.
The closed form (closed=True, and what any dtype but float64 evaluates) is the one the kernels use:
  a_i = -G_i psi'(r_i),   d loss_q / d s_k = (1 / T) sum_{j != k} sigmoid'(u_kj) (a_j - a_k),
with sigmoid and sigmoid' from e = exp(-|u|): 1 / (1 + e) or e / (1 + e) by the sign of u, and e / (1 + e)^2.  `dtype` is the
type of the per-pair terms; the sums over j and every O(C) quantity stay float64 (what the kernels do in float32)."""
import numpy as np
import torch

from tests.lambdarank_ref import query_terms, window  # noqa: F401  (window: the tests' random windows)

LN2 = float(np.log(2.0))


def _sigmoid_e(u):
    e = torch.exp(-u.abs())
    return torch.where(u >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _dsigmoid_e(u):
    e = torch.exp(-u.abs())
    return e / (1.0 + e) ** 2


def _vec32(x):
    return np.array(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float32).reshape(-1)


def _offdiag(sl, C, dtype):
    m = torch.ones(sl.stop - sl.start, C, dtype=dtype)
    m[torch.arange(sl.stop - sl.start), torch.arange(sl.start, sl.stop)] = 0
    return m


def _blocks(C, block):
    return [slice(r0, min(r0 + block, C)) for r0 in range(0, C, block)]


def _psi(r, k, C):
    """psi(r_i) on a float64 tensor, written from the definition (differentiable)"""
    gate = torch.sigmoid(k + 0.5 - r) if k < C else torch.ones_like(r)
    return gate / torch.log2(1.0 + r)


def _dpsi(r, k, C):
    """psi'(r) in closed form, float64"""
    l2 = torch.log2(1.0 + r)
    dl2 = 1.0 / ((1.0 + r) * LN2)
    if k < C:
        z = k + 0.5 - r
        return -_dsigmoid_e(z) / l2 - _sigmoid_e(z) * dl2 / l2 ** 2
    return -dl2 / l2 ** 2


def _ranks_closed(s, T, block, dtype):
    """r_i (float64) with the pair terms in `dtype` and the e form"""
    C = len(s)
    sd = s.to(dtype)
    r = torch.ones(C, dtype=torch.float64)
    for sl in _blocks(C, block):
        u = (sd[None, :] - sd[sl, None]) / T
        r[sl] += (_sigmoid_e(u) * _offdiag(sl, C, dtype)).double().sum(1)
    return r


def _rank_grad_closed(s, a, T, block, dtype):
    """(1 / T) sum_j sigmoid'(u_kj) (a_j - a_k), float64, pair terms in `dtype`"""
    C = len(s)
    sd, ad = s.to(dtype), a.to(dtype)
    out = torch.zeros(C, dtype=torch.float64)
    for sl in _blocks(C, block):
        u = (sd[None, :] - sd[sl, None]) / T
        out[sl] = (_dsigmoid_e(u) * (ad[None, :] - ad[sl, None])).double().sum(1) / T
    return out


def soft_rank(score, scope, temperature=1.0, upstream=None, block=256, dtype=torch.float64, closed=False):
    """(r, d L / d score for `upstream` = d L / d r, or None): float64 numpy vectors over the window.  float64 and not `closed`:
    the forward from the definition and autograd's gradient; otherwise the closed form with the pair terms in `dtype`."""
    s32 = _vec32(score)
    assert len(s32) == sum(scope)
    T = float(temperature)
    ranks = np.zeros(len(s32), np.float64)
    grad = None if upstream is None else np.zeros(len(s32), np.float64)
    off = 0
    for C in (int(c) for c in scope):
        s = torch.from_numpy(s32[off:off + C].astype(np.float64))
        up = None if upstream is None else torch.from_numpy(np.asarray(upstream, np.float64).reshape(-1)[off:off + C].copy())
        if closed or dtype != torch.float64:
            ranks[off:off + C] = _ranks_closed(s, T, block, dtype).numpy()
            if up is not None and C:
                grad[off:off + C] = _rank_grad_closed(s, up, T, block, dtype).numpy()
        else:
            s.requires_grad_(True)
            for sl in _blocks(C, block):
                r = 1.0 + (torch.sigmoid((s[None, :] - s[sl, None]) / T) * _offdiag(sl, C, torch.float64)).sum(1)
                ranks[off + sl.start:off + sl.stop] = r.detach().numpy()
                if up is not None:
                    g, = torch.autograd.grad((r * up[sl]).sum(), s)
                    grad[off:off + C] += g.numpy()
        off += C
    return ranks, grad


def approx_ndcg(score, scope, targets, temperature=1.0, ndcg_k=0, block=256, dtype=torch.float64, closed=False, terms=False):
    """(loss_sum, ranked, d loss_sum / d score) over a window: python float, python int, float64 numpy vector; with `terms`
    also a, the gradient of loss_sum in the soft ranks (zeros for an unranked query).  score / targets: float32 vectors (numpy
    or tensors) of sum(scope) entries.  float64 and not `closed`: forward from the definitions, gradient from autograd;
    otherwise the closed form with the per-pair terms in `dtype`."""
    s32, t32 = _vec32(score), _vec32(targets)
    assert len(s32) == len(t32) == sum(scope)
    T = float(temperature)
    total, ranked = 0.0, 0
    grad = np.zeros(len(s32), np.float64)
    a_all = np.zeros(len(s32), np.float64)
    off = 0
    for C in (int(c) for c in scope):
        sq, tq = s32[off:off + C], t32[off:off + C]
        if C > 1 and tq.max() > tq.min():
            ranked += 1
            k = C if ndcg_k == 0 else min(int(ndcg_k), C)
            G = query_terms(sq, tq, ndcg_k)[1]
            s = torch.from_numpy(sq.astype(np.float64))
            if closed or dtype != torch.float64:
                r = _ranks_closed(s, T, block, dtype)
                total += 1.0 - float((G * _psi(r, k, C)).sum())
                a = -G * _dpsi(r, k, C)
                grad[off:off + C] = _rank_grad_closed(s, a, T, block, dtype).numpy()
                a_all[off:off + C] = a.numpy()
            else:
                s.requires_grad_(True)
                dot = 0.0
                for sl in _blocks(C, block):
                    r = 1.0 + (torch.sigmoid((s[None, :] - s[sl, None]) / T) * _offdiag(sl, C, torch.float64)).sum(1)
                    r.retain_grad()
                    part = (G[sl] * _psi(r, k, C)).sum()
                    part.backward()
                    dot += float(part.detach())
                    a_all[off + sl.start:off + sl.stop] = -r.grad.numpy()
                total += 1.0 - dot
                grad[off:off + C] = -s.grad.numpy()
        off += C
    return (total, ranked, grad, a_all) if terms else (total, ranked, grad)
