"""Timing of the resampled column means: rr_resample_means_f64 through
reactranker_amd.significance.resample_means against the resampling a user would write in torch eager today - torch.randint,
an index, nanmean, cut into chunks of B so that the [b, Q, M] gather fits memory - in the same process.
    python tools/resample_bench.py [--out profiles/resample_bench.txt] [--shapes 256x12x2000,10000x20x10000,100000x20x10000]
                                   [--blocks 128,256,384,512,768,1024,2048,4096]
Per shape (Q x M x B) and mode: time per call, resamples per second and the effective gather rate B Q M 8 / t (the bytes a
resample adds up, wherever they are served from: the table is Q M 8 bytes and sits in L2 or the Infinity Cache), for the
automatic grid and for every fixed --blocks setting (rr_resample_set_blocks), then the eager form.  Every figure is the median
of --repeats windows after --warmup windows of the same shape, lowest and highest next to it; a window is as many back-to-back
calls as fill about --window-ms between two device events; the settings alternate window by window.  The last line per
shape and mode says whether the lowest-to-highest ranges of the automatic grid and of the best fixed setting overlap.  The eager
side draws from torch's generator, so it computes other resamples of the same distribution: its time is compared, not its
values.  No threshold: the numbers are recorded, not asserted.  Needs a GPU."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import _lib, significance as S      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
ap.add_argument("--shapes", default="256x12x2000,10000x20x10000,100000x20x10000")
ap.add_argument("--blocks", default="128,256,384,512,768,1024,2048,4096")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--window-ms", type=float, default=20.0)
ap.add_argument("--eager-bytes", type=float, default=1e9, help="largest [b, Q, M] gather of the eager form")
ARGS = ap.parse_args()
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def calls_for(fn):
    fn()
    t = window(fn, 1)
    return max(1, min(500, int(ARGS.window_ms / max(t, 1e-3))))


def eager(x, B, mode):
    """the resampling in torch eager, chunked over B"""
    Q, M = x.shape
    step = max(1, int(ARGS.eager_bytes // (Q * M * 8)))
    out = []
    for b0 in range(0, B, step):
        b = min(step, B - b0)
        if mode == "bootstrap":
            v = x[torch.randint(Q, (b, Q), device=x.device)]
        else:
            v = x[None] * (torch.randint(0, 2, (b, Q, 1), device=x.device, dtype=torch.float64) * 2.0 - 1.0)
        out.append(torch.nanmean(v, dim=1))
    return torch.cat(out)


def fmt(ts):
    return f"{statistics.median(ts):10.4f} ms (min {min(ts):.4f}, max {max(ts):.4f})"


def main():
    torch.cuda.set_device(0)
    fixed = [int(v) for v in ARGS.blocks.split(",") if v]
    prop = torch.cuda.get_device_properties(0)
    say(f"{prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory >> 30} GiB); torch {torch.__version__}; {ARGS.warmup} warm-up + {ARGS.repeats} timed windows per figure, "
        f"a window = back-to-back calls for about {ARGS.window_ms:.0f} ms between two device events, settings alternating; "
        f"ms per call, median (min, max); GB/s = B Q M 8 / t")
    g = torch.Generator(device="cuda").manual_seed(1)
    for shape in ARGS.shapes.split(","):
        Q, M, B = (int(v) for v in shape.split("x"))
        x = torch.randn(Q, M, device="cuda", dtype=torch.float64, generator=g)
        x[torch.rand(Q, M, device="cuda", generator=g) < 0.02] = float("nan")
        work = 8.0 * B * Q * M
        for mode in ("bootstrap", "signflip"):
            mine = lambda: S.resample_means(x, B, seed=1, mode=mode)      # noqa: E731
            settings = [0] + fixed
            times = {b: [] for b in settings}
            calls = calls_for(mine)
            for r in range(ARGS.warmup + ARGS.repeats):
                for b in settings:
                    assert _lib.lib().rr_resample_set_blocks(b) == 0
                    try:
                        t = window(mine, calls)
                    finally:
                        assert _lib.lib().rr_resample_set_blocks(0) == 0
                    if r >= ARGS.warmup:
                        times[b].append(t)
            for b in settings:
                med = statistics.median(times[b])
                say(f"Q {Q:6d} M {M:2d} B {B:5d} {mode:9s} blocks {'auto' if b == 0 else b:>5}: {fmt(times[b])} = "
                    f"{B / med / 1e3:8.2f} M resamples/s = {work / med / 1e6:8.0f} GB/s  ({calls} calls per window)")
            best = min(fixed, key=lambda b: statistics.median(times[b]))
            a = statistics.median(times[0])
            inside = min(times[0]) <= max(times[best])                    # the two lowest-to-highest ranges overlap
            say(f"Q {Q:6d} M {M:2d} B {B:5d} {mode:9s} automatic {a:.4f} ms against the best fixed setting ({best}) "
                f"{statistics.median(times[best]):.4f} ms, ranges {min(times[0]):.4f} .. {max(times[0]):.4f} and "
                f"{min(times[best]):.4f} .. {max(times[best]):.4f}: "
                f"{'within' if inside else 'OUTSIDE'} its run-to-run range")
            ref = lambda: eager(x, B, mode)                               # noqa: E731
            ref()
            te = [window(ref, 1) for _ in range(1 + 3)][1:]
            say(f"Q {Q:6d} M {M:2d} B {B:5d} {mode:9s} torch eager (randint + index + nanmean, chunks of "
                f"{max(1, int(ARGS.eager_bytes // (Q * M * 8)))} resamples): {fmt(te)} = {work / statistics.median(te) / 1e6:8.0f} GB/s | "
                f"ratio {statistics.median(te) / a:.1f}x")
        del x
        torch.cuda.empty_cache()
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
