"""Restatements of the reference trainer's six listwise variants (train/loss.py: MLEDisLoss :102-141, Listnet_For_Gauss
:233-272, Listnetlognorm :275-314, Listnet_For_evidential :187-230, Listnet_with_uq :355-399, Dirichlet_uq :440-474), written
as the reference writes them: the C x C pair sums of the first three stay pair sums (not the per-element factorisation of
csrc/loss_list.h), evaluated in `dtype` (float64 by default) from float32 inputs, gradients from autograd.

A C x C float64 tensor is 512 MiB at C = 8192, so the pair forms are evaluated in blocks of `block` rows (columns for
MLEDis, whose sum runs down the columns): every block's share of the loss is back-propagated on its own and the gradients
accumulate in the leaves, which is the same sum.

One deliberate difference: a query without candidates adds zero and still counts in len(scope) - the kernels' rule
(tests/test_gpu_loss_variants.py: test_empty_and_one_candidate_queries); the reference's torch.mean of nothing is NaN.
tests/test_loss_variants_cpu.py checks every function against tests/golden/loss_variants.npz."""
import numpy as np
import torch
import torch.nn.functional as F

KINDS = ("mledis", "listnet_gauss", "listnet_lognorm", "listnet_evidential", "listnet_uq", "dirichlet_uq")
N_COLS = {"mledis": 2, "listnet_gauss": 2, "listnet_lognorm": 2, "listnet_evidential": 3, "listnet_uq": 1, "dirichlet_uq": 1}


def _blocks(C, block):
    return [slice(a, min(a + block, C)) for a in range(0, C, block)]


def _pair_softmax(t, block):
    """targ = 1 / torch.sum(torch.exp(z1 - z2), dim=1) with z1[i, j] = t[j], z2 = z1.t() (loss.py:263-265), no gradient"""
    with torch.no_grad():
        return torch.cat([1 / torch.sum(torch.exp(t[None, :] - t[b, None]), dim=1) for b in _blocks(t.shape[0], block)])


def _mledis(cols, t, scale, coef, block):
    s, v = cols
    idx = torch.argsort(t, descending=True, stable=True)                   # :126 (ties by position, as the kernels rank)
    C = t.shape[0]
    rows = torch.arange(C)
    total = 0.0
    for b in _blocks(C, block):                                            # a block of COLUMNS j of the [i, j] matrix
        ss, sv = torch.index_select(s, 0, idx), torch.index_select(v, 0, idx)     # :131 (per block: each has its own graph)
        # x1[i, j] = -ss[j], x2[i, j] = ss[i], y1[i, j] = sv[j], y2[i, j] = sv[i]  (:132-135)
        e = torch.exp(-ss[None, b] + ss[:, None] + (sv[None, b] + sv[:, None]) / 2)
        e = torch.where(rows[:, None] >= rows[None, b], e, torch.zeros((), dtype=e.dtype))     # torch.tril
        part = torch.sum(-torch.log(1 / torch.sum(e, 0))) * (scale / C)    # :136 (its mean, one block of it)
        if part.requires_grad:
            part.backward()
        total += float(part.detach())
    return total


def _listnet_pair(cols, t, scale, coef, block, lognorm):
    x, y = cols
    C = t.shape[0]
    targ = _pair_softmax(t, block)
    total = 0.0
    for b in _blocks(C, block):                                            # a block of ROWS i: x1[i, j] = x[j], x2[i, j] = x[i]
        if lognorm:
            pred = 1 / torch.sum(x[None, :] / x[b, None] * torch.exp((y[None, :] + y[b, None]) / 2), dim=1)     # :304
        else:
            pred = 1 / torch.sum(torch.exp(x[None, :] - x[b, None] + (y[None, :] + y[b, None]) / 2), dim=1)    # :262
        part = -torch.sum(targ[b] * torch.log(pred)) * (scale / C)          # :266 / :308
        if part.requires_grad:
            part.backward()
        total += float(part.detach())
    return total


def _whole(loss, scale):
    part = loss * scale
    if part.requires_grad:
        part.backward()
    return float(part.detach())


def _listnet_evidential(cols, t, scale, coef, block):
    s, v, a = cols
    pred = torch.log_softmax(s, dim=0)                                     # :222
    targ = torch.softmax(t, dim=0)                                         # :223
    return _whole(-torch.mean(targ * pred * (2 * v + a)), scale)           # :224


def _listnet_uq(cols, t, scale, coef, block):
    item, = cols
    pred_p = item / torch.sum(item)                                        # :381
    targ_p = F.softmax(t, dim=0)
    real_loss = torch.nn.KLDivLoss(reduction="batchmean")(torch.log(pred_p), targ_p)     # :386
    consist = torch.log(targ_p / pred_p)
    residue = consist * (item - torch.ones(len(item), dtype=item.dtype))   # :389-390
    loss = real_loss + coef * torch.abs(residue)                           # :391-393
    return _whole(torch.mean(loss), scale)


def _dirichlet_uq(cols, t, scale, coef, block):
    alpha, = cols
    pred_p = alpha / torch.sum(alpha)                                      # :460
    targ_p = F.softmax(t, dim=0)
    err = (pred_p - targ_p) ** 2
    var = pred_p * (1 - pred_p) / (torch.sum(alpha) + 1)                   # :463
    consist = torch.log(targ_p / pred_p)
    residue = consist * (alpha - 1)
    return _whole(torch.mean(err + var + coef * torch.abs(residue)), scale)     # :466-468


_QUERY = {
    "mledis": _mledis,
    "listnet_gauss": lambda *a: _listnet_pair(*a, lognorm=False),
    "listnet_lognorm": lambda *a: _listnet_pair(*a, lognorm=True),
    "listnet_evidential": _listnet_evidential,
    "listnet_uq": _listnet_uq,
    "dirichlet_uq": _dirichlet_uq,
}


def variant_loss(kind, cols, scope, targets, coef=0.0, dtype=torch.float64, block=1024):
    """(loss, [d loss / d column, ...]) of the listwise variant `kind` over a window: loss = sum over the queries of the
    reference's per-query value / len(scope); cols are its N_COLS[kind] per-candidate input columns (float32 arrays), coef
    the annealing coefficient of the two *_uq losses.  The gradients are float64 arrays whatever `dtype` is."""
    assert len(cols) == N_COLS[kind], (kind, len(cols))
    leaves = [torch.tensor(np.asarray(c, np.float32)).to(dtype).requires_grad_(True) for c in cols]
    t = torch.tensor(np.asarray(targets, np.float32)).to(dtype)
    Q = len(scope)
    total, lo = 0.0, 0
    for c in scope:
        hi = lo + int(c)
        if hi > lo:                                                        # (an empty query adds zero and counts in Q)
            total += _QUERY[kind]([x[lo:hi] for x in leaves], t[lo:hi], 1.0 / Q, coef, block)
        lo = hi
    grads = [(x.grad if x.grad is not None else torch.zeros_like(x)).double().numpy() for x in leaves]
    return total, grads
