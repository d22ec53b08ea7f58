"""float64 restatements used by the pairwise-variant tests: the two C x C losses of the reference's beta loops
(train/train_pairwise.py:189-226, 276-307) written as the reference writes them, with gradients from autograd in float64;
pairwise_acc / eval_cross_entropy_loss (train/eval.py:180-224, 15-73) and the baseline pair loss / accuracy
(train_pairwise.py:33-59, eval.py:246-266) in numpy; the pair order of generate_query_pairs (data/load_reactions.py:470-496).
tests/test_pairwise_variants_cpu.py checks each of them against tests/golden/pairwise_variants.npz."""
import numpy as np
import torch


def _segments(scope):
    off = np.concatenate([[0], np.cumsum(np.asarray(scope, np.int64))])
    return [(int(off[i]), int(off[i + 1])) for i in range(len(scope))]


def _pair_grids(x, rows):
    """(a, b) with a[i, j] = x[j] and b[i, j] = x[i] for the rows i of `rows` (None: all of them, b = a.t() as the reference
    writes it)"""
    if rows is None:
        a = torch.ones_like(x).unsqueeze(1) * x
        return a, a.t()
    return torch.ones_like(x[rows]).unsqueeze(1) * x, x[rows].unsqueeze(1) * torch.ones_like(x)


def _betanet_query(t, s, alpha0, rows=None):
    tau = torch.sigmoid(t)
    alpha_ini, beta_ini = _pair_grids(tau, rows)                           # [i, j] = tau[j], tau[i]
    x1 = alpha_ini / (alpha_ini + beta_ini)
    x2 = beta_ini / (alpha_ini + beta_ini)
    aT, bT = x1 * alpha0, x2 * alpha0
    pi = torch.sigmoid(s)
    pa, pb = _pair_grids(pi, rows)
    aP, bP = pa / (pa + pb) * alpha0, pb / (pa + pb) * alpha0
    lnB_t = torch.lgamma(aT) + torch.lgamma(bT) - torch.lgamma(aT + bT)
    lt = (aT - 1) * torch.log(x1) + (bT - 1) * torch.log(x2) - lnB_t
    lnB_p = torch.lgamma(aP) + torch.lgamma(bP) - torch.lgamma(aP + bP)
    lp = (aP - 1) * torch.log(x1) + (bP - 1) * torch.log(x2) - lnB_p
    return torch.sum(torch.exp(lt) * (lt - lp))


def _beta_evi_query(t, p, coef, rows=None):
    tau = torch.sigmoid(t)
    alpha_ini, beta_ini = _pair_grids(tau, rows)
    T1, T2 = alpha_ini / (alpha_ini + beta_ini), beta_ini / (alpha_ini + beta_ini)
    pa, pb = _pair_grids(p, rows)
    P1, P2 = pa / (pa + pb), pb / (pa + pb)
    err = (T1 - P1) ** 2 + (T2 - P2) ** 2
    var = P1 * (1 - P1) / (pa + pb + 1) + P2 * (1 - P2) / (pa + pb + 1)
    pen1 = torch.abs(torch.log(T1 / P1) * (pa - 1))
    pen2 = torch.abs(torch.log(T1 / P1) * (pa - 1))                        # the reference repeats the first component
    return torch.sum(err + var + coef * (pen1 + pen2))


def sq_loss(kind, scores, scope, targets, param, dtype=torch.float64, block=None):
    """(loss_sum, pairs, d loss_sum / d scores) of 'betanet' (param = alpha0) or 'beta_evidential' (param = coef) over a
    window, evaluated in `dtype` from float32 inputs.  block: None builds every query's C x C tensors whole, as the reference
    does; a row count evaluates them `block` rows at a time, each block's share back-propagated on its own (the same sums;
    a query of 5462 candidates would otherwise hold several GB of float64 under autograd)."""
    s = torch.tensor(np.asarray(scores, np.float32)).to(dtype).requires_grad_(True)
    t = torch.tensor(np.asarray(targets, np.float32)).to(dtype)
    fn = _betanet_query if kind == "betanet" else _beta_evi_query
    pairs = 0
    if block is not None:
        total = 0.0
        for lo, hi in _segments(scope):
            pairs += (hi - lo) ** 2 - (hi - lo)
            for r0 in range(0, hi - lo, block):
                part = fn(t[lo:hi], s[lo:hi], param, slice(r0, min(r0 + block, hi - lo)))
                part.backward()
                total += float(part.detach())
        g = s.grad if s.grad is not None else torch.zeros_like(s)
        return total, pairs, g.numpy().astype(np.float64)
    total = torch.zeros((), dtype=dtype)
    for lo, hi in _segments(scope):
        if hi > lo:
            total = total + fn(t[lo:hi], s[lo:hi], param)
            pairs += (hi - lo) ** 2 - (hi - lo)
    if s.numel() and total.requires_grad:
        g, = torch.autograd.grad(total, [s])
    else:
        g = torch.zeros_like(s)
    return float(total.detach()), pairs, g.detach().numpy().astype(np.float64)


def pairwise_stats(scores, scope, targets, sigma=1.0, block=None):
    """(pairwise_acc, eval_cross_entropy_loss, per-query [npos, mismatches, ce]) in float64; the score differences are formed
    in float32 as the reference's tensors are.  block: rows of a query's C x C arrays evaluated at a time (None: all)."""
    s = np.asarray(scores, np.float32)
    t = np.asarray(targets, np.float32)
    accs, ce_sum, n_pairs, rows = [], 0.0, 0.0, []
    for lo, hi in _segments(scope):
        sq, tq = s[lo:hi], t[lo:hi]
        npos, mism, ce = 0.0, 0.0, 0.0
        step = block or max(hi - lo, 1)
        for r0 in range(0, hi - lo, step):
            sr, tr = sq[r0:r0 + step], tq[r0:r0 + step]
            tp = tr[:, None] > tq[None, :]
            sp = sr[:, None] > sq[None, :]
            npos += float(tp.sum())
            mism += float((tp != sp).sum())
            x = (np.float32(sigma) * (sr[:, None] - sq[None, :])).astype(np.float64)
            softplus = np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
            S = np.sign(tr[:, None].astype(np.float64) - tq[None, :])
            C = 0.5 * (1.0 - S) * x + softplus                            # -logsigmoid(-x) = softplus(x)
            ce += float((C * (S != 0)).sum())
        rows.append([npos, mism, ce])
        if npos > 0:
            accs.append(1.0 - mism / (2.0 * npos))
            ce_sum += ce
            n_pairs += 2.0 * npos
    acc = float(np.mean(accs)) if accs else float("nan")
    return acc, (ce_sum / n_pairs if n_pairs else float("nan")), np.asarray(rows, np.float64).reshape(-1, 3)


def pair_softmax_mse(y, targets):
    """(loss, d loss / d y) of mean_b sum_k (softmax(t_b)_k - y_bk / sum_k y_bk)^2 in float64."""
    yy = torch.tensor(np.asarray(y, np.float32)).double().requires_grad_(True)
    tt = torch.tensor(np.asarray(targets, np.float32)).double()
    tp = torch.softmax(tt, dim=1)
    pp = yy / yy.sum(dim=1, keepdim=True)
    loss = ((tp - pp) ** 2).sum(dim=1).mean()
    g, = torch.autograd.grad(loss, [yy])
    return float(loss.detach()), g.numpy()


def pair_acc(y, targets):
    y, t = np.asarray(y, np.float32), np.asarray(targets, np.float32)
    return 1.0 - float(np.mean((y[:, 0] > y[:, 1]) != (t[:, 0] > t[:, 1])))


def query_pair_order(targets):
    """(i, j) row indices of generate_query_pairs for one query: for every distinct target value in order of first
    appearance, each row holding it (in row order) against each row holding another value (in row order)."""
    t = np.asarray(targets)
    seen, vals = set(), []
    for v in t.tolist():
        if v not in seen:
            seen.add(v)
            vals.append(v)
    ii, jj = [], []
    for v in vals:
        a = [k for k in range(len(t)) if t[k] == v]
        b = [k for k in range(len(t)) if t[k] != v]
        for x in a:
            for y in b:
                ii.append(x)
                jj.append(y)
    return np.asarray(ii, np.int32), np.asarray(jj, np.int32)
