"""dw and dbias of Fn.wgrad over every instantiation of the three weight-gradient kernels of csrc/wgrad.hip, as one .npz - to be
run with two builds of the library (RR_LIB_PATH) on one MI355X and compared byte for byte:
    python tools/wgrad_bits.py --out A.npz
    python tools/wgrad_bits.py --compare A.npz B.npz    (prints the array count and the names that differ; status 1 on any)
Seeded inputs, Fn.SPLIT_MIN_ROWS = 1.  Three arithmetic forms (exact f32 MFMA, three bf16 terms, two f16 terms), each crossed
with mask on/off, subtract on/off, gathered or direct x1 (indices -1 in row 0 and in the middle; the subtract source is
gathered when x1 is) over
    (k1, k2): (1,0) (91,0) (95,0) (127,0): k-blocks of 96 / 128 / 160 columns and k1 % 4 != 0; (133,300): the ones column
              starts a chunk; (300,83): it shares one; (0,300): no segment 1; (319,0): three k-blocks
    M:        1, 31, 33, 65, 4097: one short tile, both sides of the 32-row tile, two M-chunks, many chunks with a short last one
    N:        4, 164, 300: one n-block with a tail, two n-blocks
while dbias given / None, fresh / accumulate=True into a non-zero dw, and ld_dw = K / K + 3 cycle through their eight
combinations from case to case (they only reach the reduction).  A fresh dw starts as NaN, its padding columns included.
Then the scalar-load kernel: N = 2, and an x1 whose leading dimension is 33, with SplitGemm off and on."""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import functions as Fn  # noqa: E402
from tools.window_loss_bits import compare  # noqa: E402

FORMS = {"f32": (False, False), "bf16x3": (True, False), "f16x2": (True, True)}      # name -> SplitGemm.enabled, .f16
SHAPES = ((1, 0), (91, 0), (95, 0), (127, 0), (133, 300), (300, 83), (0, 300), (319, 0))
MS = (1, 31, 33, 65, 4097)
NS = (4, 164, 300)
M_MAX, N_MAX, W1, W2 = max(MS), max(NS), 320, 304       # pool widths: row pitches that keep every slice 16-byte aligned
OUT = {}


def tails():
    return itertools.cycle(itertools.product((True, False), repeat=3))               # (dbias, accumulate, ld_dw > K)


def put(name, x):
    assert name not in OUT, name
    OUT[name] = x.detach().cpu().numpy()


def pools():
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    P = dict(dy=f(M_MAX, N_MAX) * np.exp(2 * f(M_MAX, 1)),    # rows of very different size (the f16 form scales by the tensor's bound)
             mask=np.maximum(f(M_MAX, N_MAX), 0), x1=f(M_MAX, W1), table=f(M_MAX // 2 + 5, W1), sub=np.maximum(f(M_MAX, W1), 0),
             x2=f(M_MAX, W2), dw0=f(N_MAX, 440), db0=f(N_MAX), x33=f(M_MAX, 33), sub33=f(M_MAX, 33))
    P = {k: torch.tensor(v).cuda() for k, v in P.items()}
    for name, rows in (("idx", M_MAX // 2 + 5), ("rev", M_MAX)):
        P[name] = torch.tensor(rng.integers(0, rows, M_MAX).astype(np.int32)).cuda()
    return P


def index(P, name, M):
    idx = P[name][:M].clone()
    idx[0] = -1
    idx[M // 2] = -1
    return idx


def case(P, tail, tag, M, N, k1, k2, mask, sub, gather, x1="x1", x1_sub="sub"):
    """one call; x1 / x1_sub name the pools read directly (rows [0, M)) or, where gathered, through "idx" / "rev" (whose
    values stay below the row count of "table", the gathered x1 of the main cases, and of every other pool)"""
    has_bias, acc, wide = next(tail)
    K = k1 + k2
    ld = K + 3 if wide else K
    dw = P["dw0"][:N, :ld].contiguous() if acc else torch.full((N, ld), float("nan"), device="cuda")
    db = (P["db0"][:N].clone() if acc else torch.full((N,), float("nan"), device="cuda")) if has_bias else None
    kw = dict(dbias=db, accumulate=acc, ld_dw=ld, k1=k1, k2=k2)
    if mask:
        kw.update(mask=P["mask"][:M, :N], mask_scale=1.25)
    if k1:
        kw["x1"] = P["table" if x1 == "x1" else x1] if gather else P[x1][:M]
        if gather:
            kw["x1_idx"] = index(P, "idx", M)
        if sub:
            kw["x1_sub"] = P[x1_sub] if gather else P[x1_sub][:M]
            if gather:
                kw["x1_sub_idx"] = index(P, "rev", M)
    if k2:
        kw["x2"] = P["x2"][:M]
    Fn.wgrad(M, N, P["dy"][:M, :N], dw[:, :K], **kw)
    tag = f"{tag}/k{k1}_{k2}/M{M}/N{N}/mask{int(mask)}sub{int(sub)}gather{int(gather)}/bias{int(has_bias)}acc{int(acc)}wide{int(wide)}"
    put(tag + "/dw", dw)
    if has_bias:
        put(tag + "/dbias", db)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar="NPZ", default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    Fn.SPLIT_MIN_ROWS = 1
    P = pools()
    flags = list(itertools.product((False, True), repeat=3))                          # (mask, sub, gather)
    for form, (enabled, f16) in FORMS.items():
        Fn.SplitGemm.enabled, Fn.SplitGemm.f16 = enabled, f16
        tail = tails()                                                                # the same cases in every form
        for (k1, k2), M, N in itertools.product(SHAPES, MS, NS):
            next(tail)                                                                # eight flag sets: shift the cycle against them
            for mask, sub, gather in flags:
                if k1 or not (sub or gather):
                    case(P, tail, form, M, N, k1, k2, mask, sub, gather)
    Fn.SplitGemm.f16 = False
    for enabled in (False, True):                                                     # both land on wgrad_kernel
        Fn.SplitGemm.enabled = enabled
        tag = f"scalar/split{int(enabled)}"
        tail = tails()
        for M in (33, 4097):
            next(tail)
            for mask, sub, gather in flags:
                case(P, tail, tag + "/n2", M, 2, 133, 300, mask, sub, gather)
                case(P, tail, tag + "/ld33", M, 164, 31, 83, mask, sub, gather, x1="x33", x1_sub="sub33")
    np.savez(args.out, **OUT)
    print(f"{len(OUT)} arrays -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
