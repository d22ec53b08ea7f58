"""Numpy restatement of the per-query rank correlation (include/reactranker_hip.h, rr_rank_correlation_f32),
shared by tests/test_rank_correlation_cpu.py and tests/test_gpu_rank_correlation.py.

Written from the definitions, not from the kernel: the pair classes are counted on boolean C x C comparisons, the Spearman
ranks are the centred, doubled tie-averaged ranks a_i = 2 (1 + #greater) + #tied others - (C + 1) as the header states them,
and the first maximum of a key is rank 0 of the stable descending order.  Every count and sum is an integer (numpy int64 and
python ints); only the final quotients and square roots are float64.  The comparisons are evaluated 512 rows at a time, so
a list of 8192 candidates needs a few tens of MB."""
import numpy as np

NSTATS = 8
BLOCK = 512
TIE_LEVELS = (0, 1, 2)      # 0: none; 1: targets rounded to halves; 2: targets to halves and scores to quarters


def window(seed, scope, ties=0):
    """(score, targets) float32 over sum(scope) candidates: scores 2 * N(0, 1), targets z-scored permutations (the random windows
    of tests/lambdarank_ref.py), then rounded as the tie level says."""
    rng = np.random.default_rng(seed)
    m = int(sum(scope))
    score = (rng.standard_normal(m) * 2).astype(np.float32)
    targets = np.concatenate([rng.permutation(c) for c in scope]).astype(np.float32) if m else np.zeros(0, np.float32)
    targets = ((targets - targets.mean()) / (targets.std() + 1e-6)).astype(np.float32) if m else targets
    if ties >= 1:
        targets = (np.round(targets * 2) / 2).astype(np.float32)
    if ties >= 2:
        score = (np.round(score * 4) / 4).astype(np.float32)
    return score, targets


def query_stats(s, t):
    """The eight statistics of one list as a float64 vector; s and t are float32 vectors of the same length."""
    s, t = np.asarray(s, np.float32).reshape(-1), np.asarray(t, np.float32).reshape(-1)
    C = len(s)
    assert len(t) == C
    out = np.zeros(NSTATS, np.float64)
    if C == 0:
        out[:4] = np.nan
        return out
    P2 = D2 = X2 = Y2 = 0                                      # ordered pairs: twice the unordered counts
    gs, es, gt, et, rp, rt = (np.zeros(C, np.int64) for _ in range(6))
    pos = np.arange(C)
    for lo in range(0, C, BLOCK):
        hi = min(C, lo + BLOCK)
        si, ti = s[lo:hi, None], t[lo:hi, None]
        sg, sl = s[None, :] > si, s[None, :] < si             # a NaN is in neither: tied with everything
        tg, tl = t[None, :] > ti, t[None, :] < ti
        s_ord, t_ord = sg | sl, tg | tl
        P2 += int(((sg & tg) | (sl & tl)).sum())
        D2 += int(((sg & tl) | (sl & tg)).sum())
        X2 += int((~s_ord & t_ord).sum())
        Y2 += int((s_ord & ~t_ord).sum())
        gs[lo:hi], gt[lo:hi] = sg.sum(1), tg.sum(1)
        es[lo:hi], et[lo:hi] = (~s_ord).sum(1) - 1, (~t_ord).sum(1) - 1          # the others: not i itself
        before = pos[None, :] < pos[lo:hi, None]
        rp[lo:hi] = (sg | ((s[None, :] == si) & before)).sum(1)                  # stable descending, ties by position
        rt[lo:hi] = (tg | ((t[None, :] == ti) & before)).sum(1)
    assert P2 % 2 == D2 % 2 == X2 % 2 == Y2 % 2 == 0
    P, D, X, Y = P2 // 2, D2 // 2, X2 // 2, Y2 // 2
    assert 0 <= C * (C - 1) // 2 - (P + D + X + Y)                               # the rest is tied in both keys
    a = 2 * (1 + gs) + es - (C + 1)
    b = 2 * (1 + gt) + et - (C + 1)
    assert int(a.sum()) == 0 and int(b.sum()) == 0
    sab, saa, sbb = int((a * b).sum()), int((a * a).sum()), int((b * b).sum())
    den_t = (P + D + X) * (P + D + Y)                                            # a python int, below 2^53
    out[0] = np.float64(P - D) / np.sqrt(np.float64(den_t)) if den_t > 0 else np.nan
    den_r = np.float64(saa) * np.float64(sbb)
    out[1] = np.float64(sab) / np.sqrt(den_r) if den_r > 0 else np.nan
    it, is_ = int(np.flatnonzero(rt == 0)[0]), int(np.flatnonzero(rp == 0)[0])   # the first maxima
    out[2] = 1.0 / (1.0 + np.float64(rp[it]))
    out[3] = np.float64(t[it]) - np.float64(t[is_])
    out[4:] = P, D, X, Y
    return out


def window_stats(score, scope, targets):
    """[Q, 8] float64: query_stats of every list of the window."""
    score, targets = np.asarray(score, np.float32).reshape(-1), np.asarray(targets, np.float32).reshape(-1)
    assert len(score) == len(targets) == sum(scope)
    rows, off = [], 0
    for c in scope:
        rows.append(query_stats(score[off:off + c], targets[off:off + c]))
        off += c
    return np.stack(rows) if rows else np.zeros((0, NSTATS), np.float64)


def nanmean_stats(stats):
    """float64 restatement of reactranker_amd.eval._nanmean_stats: per column (the sum of the entries that are not NaN, their
    count)."""
    stats = np.asarray(stats, np.float64).reshape(-1, NSTATS)
    ok = ~np.isnan(stats)
    return np.where(ok, stats, 0.0).sum(0), ok.sum(0).astype(np.float64)


def summary(sums, counts):
    """The dict of reactranker_amd.eval.rank_correlation_from_scores from the column sums and counts."""
    mean = [sums[k] / counts[k] if counts[k] > 0 else float("nan") for k in range(4)]
    P, D, X, Y = (float(x) for x in sums[4:8])
    den = (P + D + X) * (P + D + Y)
    return dict(kendall_tau=float(mean[0]), spearman=float(mean[1]), mrr=float(mean[2]), regret=float(mean[3]),
                n_defined=int(counts[0]), kendall_tau_pooled=float((P - D) / np.sqrt(den)) if den > 0 else float("nan"),
                pairs=[P, D, X, Y])
