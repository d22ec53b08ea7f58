"""Timing of the embedding Gaussian: reactranker_amd.latent_gaussian.scatter (rr_col_moments_f64) and
EmbeddingGaussian.mahalanobis (rr_center_project_f32 with y == NULL) against what a user would write today in torch eager on the
same card, in the same process:
    torch.cov(x.double().T)                      and                      ((x - mu) @ W).square().sum(1)
    python tools/moments_bench.py [--out profiles/moments_bench.txt] [--rows 100000,1000000] [--hidden 300,600] [--bank 6400000]
There is no parent-commit time: the functions did not exist.  Every figure is the median of --repeats calls after --warmup calls
of the same shape, each between two device events, lowest and highest next to it; the two sides alternate call by call.  Rates:
  moments      N H (H + 1) flops (the lower triangle, one multiply-add per row and element) against the 78.6 TFLOP/s FP64 matrix
               figure AMD publishes for the MI355X, and 8 N H bytes (two reads of the rows: the mean, then the centred products)
               against the 8 TB/s HBM figure
  mahalanobis  2 N H R flops against the 157.3 TFLOP/s f32-matrix peak, and 4 N H + 4 N bytes against 8 TB/s
and the largest difference from the comparator relative to the largest value.  --bank: one more row count at the first hidden
size, run only if the rows and the comparator's temporaries fit in free memory, else named as not run.  No threshold: the
numbers are recorded, not asserted.  Needs a GPU."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import latent_gaussian as G      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
ap.add_argument("--rows", default="100000,1000000")
ap.add_argument("--hidden", default="300,600")
ap.add_argument("--bank", type=int, default=6400000)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=5)
ARGS = ap.parse_args()
LINES = []
F64_TF, F32_TF, HBM_GBS = 78.6, 157.3, 8000.0


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


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"


def pair(mine, ref, reps, warmup):
    ta, tb, a, b = [], [], None, None
    for r in range(reps):
        x, a = once(mine)
        y, b = once(ref)
        if r >= warmup:
            ta.append(x)
            tb.append(y)
    return ta, tb, a, b


def shape(N, H, g, warmup, repeats):
    reps = warmup + repeats
    x = torch.randn(N, H, device="cuda", generator=g) * (torch.rand(H, device="cuda", generator=g) * 3 + 0.1) + 1.0
    ta, tb, a, b = pair(lambda: G.scatter(x), lambda: torch.cov(x.double().T), reps, warmup)
    cov = a[1] / (N - 1)
    diff = float((cov - b).abs().max() / b.abs().max())
    ma, mb = statistics.median(ta), statistics.median(tb)
    flops, need = float(N) * H * (H + 1), 8.0 * N * H
    say(f"N {N:8d} H {H:4d} moments    : rr_col_moments_f64 {fmt(ta)} = {N / ma / 1e3:8.1f} M rows/s, "
        f"{100 * flops / ma / 1e9 / F64_TF:5.1f} % of the FP64 matrix figure, {100 * need / ma / 1e6 / HBM_GBS:5.1f} % of HBM | "
        f"torch.cov(x.double().T) {fmt(tb)} | ratio {mb / ma:.2f}x | chunks {G.chunks(N, H)} | max |cov - torch.cov| / max |cov| = {diff:.2e}")
    del a, b, cov
    gm = G.EmbeddingGaussian.fit(x)
    mu, W = gm.center_, gm.whitener_
    R = W.shape[1]
    ta, tb, a, b = pair(lambda: gm.mahalanobis(x), lambda: ((x - mu) @ W).square().sum(1), reps, warmup)
    diff = float((a - b).abs().max() / b.abs().max())
    ma, mb = statistics.median(ta), statistics.median(tb)
    flops, need = 2.0 * N * H * R, 4.0 * N * H + 4.0 * N
    say(f"N {N:8d} H {H:4d} mahalanobis: rr_center_project_f32 (R {R}) {fmt(ta)} = {N / ma / 1e3:8.1f} M rows/s, "
        f"{100 * flops / ma / 1e9 / F32_TF:5.1f} % of the f32-matrix peak, {100 * need / ma / 1e6 / HBM_GBS:5.1f} % of HBM | "
        f"((x - mu) @ W).square().sum(1) {fmt(tb)} | ratio {mb / ma:.2f}x | max |d - eager| / max |d| = {diff:.2e}")
    del x, a, b, gm
    torch.cuda.empty_cache()


def main():
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    say(f"torch {torch.__version__}; {ARGS.warmup} warm-up + {ARGS.repeats} timed calls per figure, the two sides alternating; "
        f"rates against {F64_TF} TFLOP/s (FP64 matrix, published), {F32_TF} TFLOP/s (f32 matrix) and {HBM_GBS / 1e3:.0f} TB/s (HBM)")
    hidden = [int(h) for h in ARGS.hidden.split(",")]
    for H in hidden:
        for N in [int(n) for n in ARGS.rows.split(",")]:
            shape(N, H, g, ARGS.warmup, ARGS.repeats)
    if ARGS.bank > 0:
        N, H = ARGS.bank, hidden[0]
        free = torch.cuda.mem_get_info()[0]
        need = N * H * (4 + 4 + 8 + 8) + (1 << 30)                 # the rows, x - mu, x.double() and its transpose's copy, the slabs
        if need <= free:
            shape(N, H, g, 1, 3)
        else:
            say(f"N {N:8d} H {H:4d}: not run ({need / 2 ** 30:.1f} GiB needed, {free / 2 ** 30:.1f} GiB free)")
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
