"""Timing of the greedy k-center selection: rr_kcenter_f32 through reactranker_amd.neighbors.kcenter_greedy
against the same selection written in torch eager - per pick ((x - x[c]) ** 2).sum(1), torch.minimum, a mask for the rows
already taken and argmax, with no host synchronisation either - in the same process, and against one plain read of the pool.
    python tools/kcenter_bench.py [--out profiles/kcenter_bench.txt] [--pools 10000,100000,1000000] [--hidden 300] [--picks 256]
Per pool size, with and without weights: microseconds per pick (the whole call over n picks: n + 1 launches, the initial pass
included) and the achieved rate against the 4 P H bytes a pick has to read.  Both sides start from the same init_dist (random,
finite: the distance to a labelled set), so that round 0 is not a tie of +inf that torch.argmax breaks in its own way; the
fraction of picks that agree is printed, not asserted (the eager side rounds its distances in another order).  The plain read
is torch.sum over the pool and rr_row_sqnorm_f32, each timed the same way.  Every figure is the median of --repeats calls after
--warmup calls of the same shape, each between two device events, lowest and highest next to it; the two sides alternate call
by call.  --blocks: also time these fixed grid sizes (rr_kcenter_set_blocks).  No threshold: the numbers are recorded, not
asserted.  Needs a GPU."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import _lib, neighbors as N      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
ap.add_argument("--pools", default="10000,100000,1000000")
ap.add_argument("--hidden", type=int, default=300)
ap.add_argument("--picks", type=int, default=256)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--blocks", default="", help="comma-separated fixed grid sizes to time next to the automatic one")
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


def eager_greedy(x, n, init, w):
    """the selection as a user can write it today: five to seven launches and two [P, H] temporaries per pick"""
    md = init.clone()
    taken = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    picks = torch.empty(n, dtype=torch.int64, device=x.device)
    for t in range(n):
        s = md if w is None else w * md
        c = torch.argmax(s.masked_fill(taken, -1.0)).reshape(1)
        picks[t:t + 1] = c
        taken.index_fill_(0, c, True)
        md = torch.minimum(md, ((x - x.index_select(0, c)) ** 2).sum(1))
    return picks, md


def fmt(ts, per=1.0):
    return f"{statistics.median(ts) / per:9.2f} (min {min(ts) / per:.2f}, max {max(ts) / per:.2f})"


def main():
    torch.cuda.set_device(0)
    H, n = ARGS.hidden, ARGS.picks
    reps = ARGS.warmup + ARGS.repeats
    g = torch.Generator(device="cuda").manual_seed(1)
    say(f"torch {torch.__version__}; H {H}, {n} picks per call; {ARGS.warmup} warm-up + {ARGS.repeats} timed calls per figure; "
        f"us per pick = the call's time / {n}")
    for P in [int(p) for p in ARGS.pools.split(",")]:
        x = torch.randn(P, H, device="cuda", generator=g)
        init = (torch.rand(P, device="cuda", generator=g) * 2.5 + 0.5) * H
        weight = torch.rand(P, device="cuda", generator=g) * 1.5 + 0.5
        need = 4.0 * P * H
        t_sum = [once(lambda: torch.sum(x))[0] for _ in range(reps)][ARGS.warmup:]
        t_sq = [once(lambda: N.row_sqnorm(x))[0] for _ in range(reps)][ARGS.warmup:]
        say(f"P {P:8d}: one plain read of the pool ({need / 1e6:.1f} MB): torch.sum {fmt(t_sum, 1e-3)} us = "
            f"{need / statistics.median(t_sum) / 1e6:.0f} GB/s | rr_row_sqnorm_f32 {fmt(t_sq, 1e-3)} us = "
            f"{need / statistics.median(t_sq) / 1e6:.0f} GB/s")
        for w in (None, weight):
            mine, ref = (lambda: N.kcenter_greedy(x, n, init_dist=init, weight=w)), (lambda: eager_greedy(x, n, init, w))
            ta, tb = [], []
            for r in range(reps):
                a, out_a = once(mine)
                b, out_b = once(ref)
                if r >= ARGS.warmup:
                    ta.append(a)
                    tb.append(b)
            agree = float((out_a["picks"] == out_b[0]).float().mean())
            ma, mb = statistics.median(ta), statistics.median(tb)
            say(f"P {P:8d} {'weights' if w is not None else 'plain  '}: rr_kcenter_f32 {fmt(ta, n * 1e-3)} us per pick = "
                f"{need * n / ma / 1e6:6.0f} GB/s | torch eager {fmt(tb, n * 1e-3)} us per pick | ratio {mb / ma:.2f}x | "
                f"per pick / plain read (torch.sum) {ma / n / statistics.median(t_sum):.2f} | same pick in {100 * agree:.1f} % of rounds")
            for b in [int(v) for v in ARGS.blocks.split(",") if v]:
                assert _lib.lib().rr_kcenter_set_blocks(b) == 0
                try:
                    tc = [once(mine)[0] for _ in range(reps)][ARGS.warmup:]
                finally:
                    assert _lib.lib().rr_kcenter_set_blocks(0) == 0
                say(f"      blocks {b:4d}: {fmt(tc, n * 1e-3)} us per pick = {need * n / statistics.median(tc) / 1e6:6.0f} GB/s")
        del x, init, weight
        torch.cuda.empty_cache()
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
