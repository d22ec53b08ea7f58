"""Timing of the nearest-neighbour search: rr_knn_f32 through reactranker_amd.neighbors.knn (bank norms
kept, as a ReactionBank keeps them) against the only other way to get the answer today - torch.cdist(q, chunk).pow(2) and
topk(k, largest=False) over bank chunks that fit in memory, merged with a second topk - in the same process.
    python tools/knn_bench.py [--out profiles/neighbors_bench.txt] [--bank 1000000] [--hidden 300] [--resources FILE]
Shapes: M = 4096 with k in {1, 16, 64}, then M = 64, all against the same bank of standard-normal rows.  Every figure is the
median of --repeats single calls (after --warmup calls of the same shape), each between two device events, with the lowest
and highest next to it; the two sides alternate call by call.  The achieved matrix rate uses the flops the definition needs,
2 M N H, against the 157.3 TFLOP/s f32-matrix peak.  The comparator's indices are compared with the kernel's (they may differ
where two f32 distances tie or cross within rounding: the fraction that agrees is printed, not asserted).  --resources: a file
of `tools/kernel_resources.py` lines (registers, spills, LDS per kernel) to record next to the times.  No threshold: the
numbers are recorded, not asserted.  Needs a GPU."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import _lib, neighbors as N      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
ap.add_argument("--bank", type=int, default=1_000_000)
ap.add_argument("--hidden", type=int, default=300)
ap.add_argument("--chunk", type=int, default=65536, help="bank rows per cdist call of the comparator")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--resources", default=None)
ARGS = ap.parse_args()
LINES = []
PEAK_TF = 157.3


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


def cdist_topk(q, bank, k, chunk):
    best_d = best_i = None
    for n0 in range(0, bank.shape[0], chunk):
        d = torch.cdist(q, bank[n0:n0 + chunk]).pow(2)
        dd, ii = d.topk(min(k, d.shape[1]), dim=1, largest=False)
        ii = ii + n0
        if best_d is None:
            best_d, best_i = dd, ii
        else:
            cd, ci = torch.cat([best_d, dd], 1), torch.cat([best_i, ii], 1)
            best_d, sel = cd.topk(k, dim=1, largest=False)
            best_i = ci.gather(1, sel)
    return best_d, best_i


def fmt(ts):
    return f"{statistics.median(ts):9.2f} ms (min {min(ts):.2f}, max {max(ts):.2f})"


def main():
    torch.cuda.set_device(0)
    H, NB = ARGS.hidden, ARGS.bank
    g = torch.Generator(device="cuda").manual_seed(1)
    bank = torch.randn(NB, H, device="cuda", generator=g)
    bn = N.row_sqnorm(bank)
    t_norm = [once(lambda: N.row_sqnorm(bank))[0] for _ in range(ARGS.warmup + ARGS.repeats)][ARGS.warmup:]
    rt, bt, mk = N.geometry()
    say(f"torch {torch.__version__}; bank {NB} x {H} f32 ({NB * H * 4 / 1e9:.2f} GB), query tile {rt} rows, bank tile {bt} rows, "
        f"k <= {mk}; {ARGS.warmup} warm-up + {ARGS.repeats} timed calls per figure")
    say(f"rr_row_sqnorm_f32 of the bank: {fmt(t_norm)}  ({NB * H * 4 / statistics.median(t_norm) / 1e9:.2f} TB/s read)")
    for M, ks in ((4096, (1, 16, 64)), (64, (1, 16, 64))):
        q = torch.randn(M, H, device="cuda", generator=g)
        for k in ks:
            mine, ref = (lambda: N.knn(q, bank, k, bank_sqnorm=bn)), (lambda: cdist_topk(q, bank, k, ARGS.chunk))
            ta, tb = [], []
            for r in range(ARGS.warmup + ARGS.repeats):
                a, out_a = once(mine)
                b, out_b = once(ref)
                if r >= ARGS.warmup:
                    ta.append(a)
                    tb.append(b)
            agree = float((out_a[1] == out_b[1]).float().mean())
            worst = float((out_a[0] - out_b[0]).abs().max())
            ws = _lib.C.c_size_t()
            _lib.lib().rr_knn_workspace_bytes(M, NB, k, _lib.C.byref(ws))
            ma = statistics.median(ta)
            flops = 2.0 * M * NB * H
            say(f"M {M:5d} k {k:2d}: rr_knn_f32 {fmt(ta)} = {flops / ma / 1e9:6.1f} TFLOP/s, {100 * flops / ma / 1e9 / PEAK_TF:4.1f} % of "
                f"the f32-matrix peak (floor {flops / PEAK_TF / 1e9:.2f} ms), workspace {ws.value / 1e6:.1f} MB | cdist + topk "
                f"{fmt(tb)} | ratio {statistics.median(tb) / ma:.2f}x | same index {100 * agree:.2f} % of slots, "
                f"max |dist difference| {worst:.2e}")
    if ARGS.resources and os.path.exists(ARGS.resources):
        say("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py):")
        for ln in open(ARGS.resources):
            if ln.strip():
                say("  " + ln.rstrip())
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
