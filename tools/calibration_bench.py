"""Isolated timing of the two calibration entries on windows of 64 x 64, 256 x 64 and 1 x 8192 candidates:
  - rr_top1_sets_f32 (rank, mass ahead, prediction set and the nine per-query statistics of every list in one launch), and
  - rr_gauss_calibration_f64 (the eight sums and a 20-bin PIT histogram of the window's Q * C rows in two launches),
each next to a torch restatement on the device that uses the same definitions in float64: the top-1 sets as a [Q, C, C]
comparison cube (`before` as a masked torch.sum, so equal to the library's ordered sum to rounding only), the pointwise sums
with torch.special.erfc and torch.bincount.
    python tools/calibration_bench.py [--out profiles/calibration_bench.txt]
Timed with device events around back-to-back calls, enough of them for a window of about 0.1 s, after a warm-up of the same
shape; each figure is the median of five such windows with the lowest and highest next to it.  The tool also checks the two
forms against each other on the timed window.  No threshold: the numbers are recorded, not asserted.  Needs a GPU: without
one the first device call raises."""
import argparse, math, os, sys, statistics
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from reactranker_amd._lib import lib, ptr, stream, check
dev = "cuda"
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
ARGS = ap.parse_args()
LINES = []
TAU, BINS = 0.9, 20


def say(line):
    print(line, flush=True)
    LINES.append(line)


def sync_time(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                              # microseconds per call


def t_device(fn, reps=5, window_us=1e5):
    for _ in range(5):
        fn()
    n = int(min(4000, max(5, window_us / max(sync_time(fn, 5), 1.0))))
    out = [sync_time(fn, n) for _ in range(reps)]
    return statistics.median(out), min(out), max(out), n


def window(Q, C, seed=0):
    """p = softmax of 2 * N(0, 1) per list (float64, rounded to float32), targets N(0, 1) (no ties: torch.argmax names no
    tie rule); and the pointwise triple mean ~ N(0, 1), std ~ U(0.05, 3), target = mean + 1.3 std N(0, 1)"""
    rng = np.random.default_rng(seed)
    x = 2 * rng.standard_normal((Q, C))
    e = np.exp(x - x.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(np.float32).reshape(-1)
    targets = rng.standard_normal(Q * C).astype(np.float32)
    seg = (np.arange(Q + 1) * C).astype(np.int32)
    mean, std = rng.standard_normal(Q * C), rng.uniform(0.05, 3.0, Q * C)
    y = mean + 1.3 * std * rng.standard_normal(Q * C)
    return [torch.tensor(np.asarray(v)).to(dev) for v in (p, targets, seg, mean.astype(np.float32), std.astype(np.float32),
                                                          y.astype(np.float32))]


def torch_top1(p, t, Q, C, tau):
    p2, t2 = p.view(Q, C), t.view(Q, C)
    pos = torch.arange(C, device=dev)
    pj, pi = p2[:, None, :], p2[:, :, None]
    ahead = (pj > pi) | ((pj == pi) & (pos[None, None, :] < pos[None, :, None]))
    rank = 1 + ahead.sum(-1)
    before = torch.where(ahead, pj.double(), torch.zeros((), dtype=torch.float64, device=dev)).sum(-1)
    inside = before <= tau
    it = torch.argmax(t2, dim=1, keepdim=True)                        # (the window's targets have no ties)
    is_ = torch.argmin(rank, dim=1, keepdim=True)
    p64 = p2.double()
    onehot = torch.zeros_like(p64).scatter_(1, it, 1.0)
    stats = torch.stack([(is_ == it).double()[:, 0], p64.gather(1, is_)[:, 0], p64.gather(1, it)[:, 0],
                         rank.gather(1, it)[:, 0].double(), ((p64 - onehot) ** 2).sum(1), before.gather(1, it)[:, 0],
                         inside.sum(1).double(), inside.gather(1, it)[:, 0].double(), p64.sum(1)], 1)
    return rank.int().view(-1), before.view(-1), inside.view(-1), stats


def torch_gauss(mean, std, y, scale, bins):
    m, s, t = mean.double(), std.double(), y.double()
    ok = torch.isfinite(m) & torch.isfinite(t) & torch.isfinite(s) & (s > 0)
    m, s, t = m[ok], s[ok], t[ok]
    sigma = scale * s
    err = t - m
    z = err / sigma
    pit = 0.5 * torch.special.erfc(-z / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    crps = sigma * (z * (2 * pit - 1) + 2 * pdf - 1 / math.sqrt(math.pi))
    b = torch.clamp(torch.floor(pit * bins).long(), max=bins - 1)
    n = torch.tensor(float(m.numel()), dtype=torch.float64, device=dev)
    sums = torch.stack([n, mean.numel() - n, z.sum(), (z * z).sum(), torch.log(sigma).sum(), (sigma * sigma).sum(),
                        (err * err).sum(), crps.sum()])
    return torch.cat([sums, torch.bincount(b, minlength=bins).double()])


def main():
    L = lib()
    say(f"torch {torch.__version__}; tau {TAU}, {BINS} PIT bins")
    for Q, C in ((64, 64), (256, 64), (1, 8192)):
        p, tg, seg, mean, std, y = window(Q, C)
        M = Q * C
        rank = torch.empty(M, dtype=torch.int32, device=dev)
        before = torch.empty(M, dtype=torch.float64, device=dev)
        inside = torch.empty(M, dtype=torch.uint8, device=dev)
        stats = torch.empty(Q, 9, dtype=torch.float64, device=dev)
        nv = 8 + BINS
        ws = torch.empty(((M + 255) // 256) * nv, dtype=torch.float64, device=dev)
        out = torch.empty(nv, dtype=torch.float64, device=dev)

        def top1():
            check(L.rr_top1_sets_f32(ptr(p), 1, ptr(tg), ptr(seg), Q, C, TAU, ptr(rank), ptr(before), ptr(inside), ptr(stats),
                                     stream()))

        def gauss():
            check(L.rr_gauss_calibration_f64(ptr(mean), ptr(std), ptr(y), M, 1.0, BINS, ptr(ws), ws.numel() * 8, ptr(out), stream()))

        say(f"window {Q} x {C}")
        us, lo, hi, n = t_device(top1)
        say(f"  {'rr_top1_sets_f32':44s} {us:10.1f} us  (min {lo:.1f}, max {hi:.1f}; {n} calls per window)   {Q * C * C / us * 1e-3:8.2f} G steps/s")
        us_t, lo, hi, n = t_device(lambda: torch_top1(p, tg, Q, C, TAU))
        say(f"  {'torch restatement, [Q, C, C] cube':44s} {us_t:10.1f} us  (min {lo:.1f}, max {hi:.1f}; {n} calls per window)   {us_t / us:8.1f}x the launch")
        top1()
        r, b, s, st = torch_top1(p, tg, Q, C, TAU)
        err_b = float((b - before).abs().max())
        near = (b - TAU).abs() <= 1e-12                               # (the two sums may fall on either side of tau)
        same_set = bool(((s == inside.bool()) | near).all())
        err_s = float((st[:, [1, 2, 4, 8]] - stats[:, [1, 2, 4, 8]]).abs().max())
        say(f"  library against torch on this window: ranks {'equal' if torch.equal(r, rank) else 'DIFFER'}, sets "
            f"{'equal' if same_set else 'DIFFER'}, max |before difference| {err_b:.2e}, max |confidence, p, Brier, mass difference| {err_s:.2e}")
        assert torch.equal(r, rank) and same_set and err_b <= 1e-12 and err_s <= 1e-12

        say(f"  rows {M}")
        us, lo, hi, n = t_device(gauss)
        say(f"  {'rr_gauss_calibration_f64 (two launches)':44s} {us:10.1f} us  (min {lo:.1f}, max {hi:.1f}; {n} calls per window)")
        us_t, lo, hi, n = t_device(lambda: torch_gauss(mean, std, y, 1.0, BINS))
        say(f"  {'torch restatement':44s} {us_t:10.1f} us  (min {lo:.1f}, max {hi:.1f}; {n} calls per window)   {us_t / us:8.1f}x the launches")
        gauss()
        want = torch_gauss(mean, std, y, 1.0, BINS)
        rel = float(((want[:8] - out[:8]).abs() / want[:8].abs().clamp_min(1.0)).max())
        moved = int((want[8:] - out[8:]).abs().sum())
        say(f"  library against torch on these rows: max sum difference {rel:.2e} (relative, floor 1), histogram rows moved {moved}")
        assert rel <= 1e-10 and moved <= 2
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


main()
