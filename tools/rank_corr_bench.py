"""Isolated timing of the per-query rank correlation launch (rr_rank_correlation_f32: Kendall tau-b, Spearman rho, reciprocal
rank, regret and the pair counts of every list in one launch) on windows of 64 x 64, 256 x 64 and 8 x 8192 candidates, next to
  - one rr_ranking_metrics_f32 launch on the same window, a yardstick of known cost (what validation already pays), and
  - the path it replaces: the scores copied to the host, then scipy.stats.kendalltau and spearmanr per query, on 16 threads at
    most.
    python tools/rank_corr_bench.py [--out profiles/rank_correlation_bench.txt]
The two launches are timed with device events around back-to-back calls, enough of them for a window of about 0.1 s, after a
warm-up of the same shape; the host path with a host clock from the synchronise before the copy to the last query's result.
Each figure is the median of five such windows (three for the host path) with the lowest and highest next to it.  The tool also
checks that the device's tau and rho are scipy's on the timed window (1e-14).  No threshold: the numbers are recorded, not
asserted.  Needs a GPU: without one the first device call raises."""
import argparse, os, sys, statistics, time, warnings
from concurrent.futures import ThreadPoolExecutor
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from reactranker_amd._lib import lib, ptr, stream, check
dev = "cuda"
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
ARGS = ap.parse_args()
LINES = []
THREADS = min(16, os.cpu_count() or 1)


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
    rng = np.random.default_rng(seed)
    score = (rng.standard_normal(Q * C) * 2).astype(np.float32)
    targets = np.concatenate([rng.permutation(C) for _ in range(Q)]).astype(np.float32)
    targets = np.round((targets - targets.mean()) / (targets.std() + 1e-6) * 8) / 8       # rounded to eighths: ties
    seg = (np.arange(Q + 1) * C).astype(np.int32)
    return torch.tensor(score).to(dev), torch.tensor(targets.astype(np.float32)).to(dev), torch.tensor(seg).to(dev)


def main():
    from scipy import stats as S
    L = lib()
    say(f"scipy {__import__('scipy').__version__}, host path on {THREADS} threads")
    for Q, C in ((64, 64), (256, 64), (8, 8192)):
        s, tg, seg = window(Q, C)
        n_pairs = Q * C * (C - 1) // 2
        corr = torch.empty(Q, 8, dtype=torch.float64, device=dev)
        order = torch.empty(Q * C, dtype=torch.int32, device=dev)
        stats = torch.empty(Q, 12, dtype=torch.float64, device=dev)
        t_host = tg.cpu().numpy()                                     # the targets come from the host in the first place

        def rank_corr():
            check(L.rr_rank_correlation_f32(ptr(s), 1, ptr(tg), ptr(seg), Q, C, ptr(corr), stream()))

        def metrics():
            check(L.rr_ranking_metrics_f32(ptr(s), 1, ptr(tg), ptr(seg), Q, C, 0.25, 0.5, ptr(order), ptr(stats), stream()))

        def one(q):
            a, b = HOST[q * C:(q + 1) * C], t_host[q * C:(q + 1) * C]
            return float(S.kendalltau(a, b).statistic), float(S.spearmanr(a, b).statistic)

        def host():
            global HOST
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            HOST = s.cpu().numpy()                                    # the device-to-host copy (synchronises)
            with ThreadPoolExecutor(THREADS) as pool:
                res = list(pool.map(one, range(Q)))
            return (time.perf_counter() - t0) * 1e6, res

        say(f"window {Q} x {C} ({n_pairs} pairs)")
        us, lo, hi, n = t_device(rank_corr)
        say(f"  {'rr_rank_correlation_f32':44s} {us:10.1f} us  (min {lo:.1f}, max {hi:.1f}; {n} calls per window)   {n_pairs / us * 1e-3:8.2f} G pairs/s")
        us_m, lo, hi, n = t_device(metrics)
        say(f"  {'rr_ranking_metrics_f32 (yardstick)':44s} {us_m:10.1f} us  (min {lo:.1f}, max {hi:.1f}; {n} calls per window)")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            host()                                                     # warm-up
            runs = [host() for _ in range(3)]
        hs = sorted(r[0] for r in runs)
        say(f"  {'copy + scipy kendalltau, spearmanr per query':44s} {hs[1]:10.1f} us  (min {hs[0]:.1f}, max {hs[2]:.1f})   {hs[1] / us:8.1f}x the launch")
        rank_corr()
        got, want = corr.cpu().numpy(), np.array(runs[0][1])
        err = float(np.nanmax(np.abs(got[:, :2] - want)))
        say(f"  device against scipy on this window: max |tau, rho difference| {err:.2e}")
        assert err <= 1e-14 and np.array_equal(np.isnan(got[:, :2]), np.isnan(want))
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


HOST = None
main()
