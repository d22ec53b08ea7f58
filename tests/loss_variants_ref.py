"""float64 numpy restatements used by the loss-variant tests: digamma, and evidential_loss_new's M x M cross form with its
gradients (reference train/loss.py:402-437 under torch broadcasting: parameter row i against target j)."""
import math

import numpy as np

PI_F32 = float(np.float32(np.pi))


def digamma(x):
    """psi(x) for x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 6, then the asymptotic series."""
    x = np.array(x, np.float64, copy=True)
    r = np.zeros_like(x)
    while True:
        small = x < 6.0
        if not small.any():
            break
        r[small] -= 1.0 / x[small]
        x[small] += 1.0
    f = 1.0 / (x * x)
    tail = f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132)))))
    return r + np.log(x) - 0.5 / x - tail


def nig_cross(mu, v, alpha, beta, targets, lam, eps=1e-4, block=256):
    """(loss, dmu, dv, dalpha, dbeta) of mean_{i,j} l(params_i, t_j) in float64, rows in blocks to bound memory."""
    mu, v, a, b, t = (np.asarray(x, np.float64) for x in (mu, v, alpha, beta, targets))
    M = t.shape[0]
    lg = np.array([math.lgamma(x) for x in a]) - np.array([math.lgamma(x + 0.5) for x in a])
    psi = digamma(a) - digamma(a + 0.5)
    total = 0.0
    g = [np.zeros(M) for _ in range(4)]
    for r0 in range(0, M, block):
        sl = slice(r0, min(r0 + block, M))
        m_, v_, a_, b_ = mu[sl, None], v[sl, None], a[sl, None], b[sl, None]
        om = 2.0 * b_ * (1.0 + v_)
        d = t[None, :] - m_
        q = v_ * d * d + om
        ad = np.abs(d)
        l = (0.5 * np.log(PI_F32 / v_) - a_ * np.log(om) + (a_ + 0.5) * np.log(q) + lg[sl, None]
             + lam * (ad * (2.0 * v_ + a_) - eps))
        total += l.sum()
        g[0][sl] = (-(2.0 * a_ + 1.0) * v_ * d / q - lam * (2.0 * v_ + a_) * np.sign(d)).sum(1)
        g[1][sl] = (-0.5 / v_ - a_ / (1.0 + v_) + (a_ + 0.5) * (d * d + 2.0 * b_) / q + 2.0 * lam * ad).sum(1)
        g[2][sl] = (-np.log(om) + psi[sl, None] + np.log(q) + lam * ad).sum(1)
        g[3][sl] = (-a_ / b_ + 2.0 * (a_ + 0.5) * (1.0 + v_) / q).sum(1)
    n2 = float(M) * float(M)
    return (total / n2,) + tuple(x / n2 for x in g)
