"""Timing of the neighbour count and of the sphere-exclusion rounds against the existing code they are built
from, in the same process: rr_radius_count_f32 beside rr_knn_f32 at k = 1, and an exclusion round beside a k-center pick.
    python tools/cluster_bench.py [--out profiles/cluster_bench.txt] [--pools 10000,100000,1000000] [--hidden 300] [--rounds 256]
Per pool size P (rows x, standard normal):
  count     radius_count(x, x) and knn(x, x, k = 1), each the whole call; the implied rate is that of the 4 P H bytes of the bank
            per row tile of 64 queries (what the tile walk reads through LDS), 4 P H * ceil(P / 64).  Skipped above
            --count-limit rows (at P = 10^6 the [P, P] walk takes minutes): there only the rounds are timed.
  rounds    microseconds per exclusion round over --rounds rounds of one call (order 'index': no [P, P] pass; the initial pass is
            included, as kcenter's is) at a radius so small that almost nothing is assigned - every round streams the whole pool,
            the case that compares with a k-center pick - beside rr_kcenter_f32's microseconds per pick over as many picks, and
            the rate against the 4 P H bytes such a round has to read;
            the same at a radius from suggest_radius (on the first --suggest-rows rows), with the clusters it produced in those
            rounds and the rows still unassigned: later rounds read only what is left.
Every figure is min / median / max of --repeats calls after --warmup calls of the same shape, each between two device events;
the two sides alternate call by call.  No threshold: the numbers are recorded, not asserted.  Needs a GPU."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import clusters as K, neighbors as N      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
ap.add_argument("--pools", default="10000,100000,1000000")
ap.add_argument("--hidden", type=int, default=300)
ap.add_argument("--rounds", type=int, default=256)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--count-limit", type=int, default=100000, help="largest pool whose [P, P] count / knn is timed")
ap.add_argument("--suggest-rows", type=int, default=20000)
ARGS = ap.parse_args()
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def fmt(ts, per=1.0):
    return f"{statistics.median(ts) / per:9.2f} (min {min(ts) / per:.2f}, max {max(ts) / per:.2f})"


def pair(mine, ref):
    """the two sides alternating call by call -> (times of mine, times of ref, last results)"""
    ta, tb, out_a, out_b = [], [], None, None
    for r in range(ARGS.warmup + ARGS.repeats):
        a, out_a = once(mine)
        b, out_b = once(ref)
        if r >= ARGS.warmup:
            ta.append(a)
            tb.append(b)
    return ta, tb, out_a, out_b


def main():
    torch.cuda.set_device(0)
    H, n = ARGS.hidden, ARGS.rounds
    g = torch.Generator(device="cuda").manual_seed(1)
    say(f"torch {torch.__version__}; H {H}, {n} rounds / picks per call; {ARGS.warmup} warm-up + {ARGS.repeats} timed calls per figure "
        f"(median, min, max); us per round = the call's time / {n}")
    for P in [int(p) for p in ARGS.pools.split(",")]:
        x = torch.randn(P, H, device="cuda", generator=g)
        need = 4.0 * P * H
        radius = K.suggest_radius(x[:ARGS.suggest_rows], k=8, quantile=0.5)
        if P <= ARGS.count_limit:
            ta, tb, cnt, _ = pair(lambda: K.radius_count(x, x, radius), lambda: N.knn(x, x, 1))
            walked = need * ((P + 63) // 64)
            ma, mb = statistics.median(ta), statistics.median(tb)
            say(f"P {P:8d} count : radius_count(x, x) {fmt(ta)} ms = {walked / ma / 1e9:6.2f} TB/s through LDS | knn(x, x, k=1) {fmt(tb)} ms = "
                f"{walked / mb / 1e9:6.2f} TB/s | knn / count {mb / ma:.2f}x | radius {radius:.3f}: mean count {float(cnt.double().mean()):.1f}")
        else:
            say(f"P {P:8d} count : not timed above {ARGS.count_limit} rows (the rounds only)")
        for what, r in (("tiny radius   ", 1e-3), ("suggest_radius", radius)):
            ta, tb, res, _ = pair(lambda: K.sphere_exclusion(x, r, order="index", max_clusters=n), lambda: N.kcenter_greedy(x, n))
            ma, mb = statistics.median(ta), statistics.median(tb)
            say(f"P {P:8d} rounds, {what}: rr_sphere_exclusion_f32 {fmt(ta, n * 1e-3)} us per round = {need * n / ma / 1e6:6.0f} GB/s of "
                f"4 P H | rr_kcenter_f32 {fmt(tb, n * 1e-3)} us per pick = {need * n / mb / 1e6:6.0f} GB/s | pick / round {mb / ma:.2f}x | "
                f"radius {r:.3f}: {int(res['n_clusters'])} clusters in {n} rounds, {int(res['n_unassigned'])} rows left")
        del x
        torch.cuda.empty_cache()
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
