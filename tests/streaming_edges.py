"""Case table, inputs and references of the streaming-kernel edge tests (tests/test_streaming_edges_cpu.py,
tests/test_gpu_streaming_edges.py).  Nothing here touches the device or the library.

Entry points (ENTRY_POINTS).  The grid-stride kernels of csrc/elementwise.hip (relu_bwd, relu_bwd_sum, axpby, dropout, the
seven heads, Adam), rr_amax_f32 of csrc/pack_weights.hip, and the pointwise losses, the elementwise NIG loss and rr_digamma_f32
of csrc/loss.hip.

Size classes.  Every size is derived from the grid rule, whose constants are READ from the sources as text (constants()):
a streaming launch is min(ceil(work / 256), RR_GRID_CAP) workgroups of 256 threads, so its loop wraps above
RR_GRID_CAP * 256 work items - elements for the scalar kernels, 16-byte groups for the vector ones; the losses and digamma
cap at pointwise_blocks' 1,024 workgroups, rr_amax_f32 at 1,024 workgroups of (total + 3) / 4 items.
  zero   n = 0: RR_OK and nothing written (a loss forward writes the mean of nothing, NaN, into `loss` and nothing else)
  tiny   TINY: around the 4-element vector, the 256-thread workgroup and Adam's 1,024-element block
  today  30,030, the one size the suite ran before
  wrap   past one pass: WRAP_SCALAR = 2 * one pass + 77 (three passes, the last partial), WRAP_VEC = 4 * (one pass + 1000) + 3
         (a partial second pass and a 3-element tail), POINTWISE for the losses and digamma (256 partials, exactly one pass,
         one element over, three passes), HEAD_WRAP, AMAX_SHAPES

Alignment classes (the four kernels with a 16-byte and a scalar form, and amax): every operand is cut out of a larger buffer
at an element offset 0 .. 3: all aligned; each operand in turn off by one element; all off by 1, 2, 3; for amax also a leading
dimension that is no multiple of 4.  At the wrap sizes only "aligned" and "all_off_1" (the references there run on the device).

References.  The build has -ffp-contract=off, so relu_bwd, relu_bwd_sum, axpby and dropout are fixed sequences of IEEE single
operations and are restated exactly, once in numpy (*_np) and once as whole-tensor torch operations (*_t, what the GPU test
runs on the device at the wrap sizes; the CPU test holds the two to the same bits).  Heads and losses: tests/loss_range.py's
float64 references and bound.  Digamma: torch.digamma in float64.  Adam: adam_np, adam_many_kernel's statement order in float64
rounded to float32 where the kernel rounds.

Aliasing.  Every kernel here declares its pointers __restrict__.  The call sites of these entry points in csrc/plan.hip write
fresh buffers (plan.hip: rr_axpby_f32 into c.alloc, rr_relu_bwd_f32 with acc == nullptr, the heads into `out` / c.alloc).
reactranker_amd/functions.py has ONE form in which an output is also an input: ReactionModelFn.backward's
`axpby(1.0, a, 1.0, b, out=a)` (the two encoders' gradients summed in place).  It is the form "out_is_a" of rr_axpby_f32
below: every thread reads a[i] before it writes out[i] and no other thread touches index i, so the result is the plain one.
`acc` of rr_relu_bwd_f32 is read and written through one pointer, which __restrict__ allows."""
import functools
import math
import os
import re

import numpy as np
import torch

from oracle import dropout_ref as DR
from tests import loss_range as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "reactranker_amd", "csrc")
SEED = 20251
F32 = np.float32
SENTINEL_BITS = 0x7FC0BEEF                     # a quiet NaN with a payload: guards and unwritten outputs hold these bits
GUARD = 8                                      # guard floats in front of and behind every output and every acc


# ------------------------------------------------------------------------------------------------ the grid rule, from the sources
def _source(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def _find(pattern, text, what):
    m = re.search(pattern, text, re.S)
    if m is None:
        raise AssertionError(f"streaming_edges: cannot find {what} in the sources")
    return m


@functools.lru_cache(maxsize=None)
def constants():
    common = _source(CSRC, "rr_common.h")
    loss = _source(CSRC, "loss.hip")
    pack = _source(CSRC, "pack_weights.hip")
    elem = _source(CSRC, "elementwise.hip")
    header = _source(REPO, "include", "reactranker_hip.h")
    num_cu = int(_find(r"#define\s+RR_NUM_CU\s+(\d+)", common, "RR_NUM_CU").group(1))
    per_cu = int(_find(r"#define\s+RR_GRID_CAP\s+\(RR_NUM_CU\s*\*\s*(\d+)\)", common, "RR_GRID_CAP").group(1))
    body = _find(r"int pointwise_blocks\(int64_t n\)\s*\{(.*?)\n\}", loss, "pointwise_blocks").group(1)
    cap = _find(r"if \(b > (\d+)\) b = (\d+);", body, "the cap of pointwise_blocks")
    if cap.group(1) != cap.group(2):
        raise AssertionError("streaming_edges: pointwise_blocks compares with one number and assigns another")
    amax_cap = int(_find(r"rr_grid_for\(\(total \+ 3\) / 4, 256, (\d+)\)", pack, "the grid of rr_amax_f32").group(1))
    _find(r"for \(; e \+ 3 \* stride < total; e \+= 4 \* stride\)", pack, "the four-loads loop of amax_kernel")
    return dict(num_cu=num_cu, grid_cap=num_cu * per_cu, pointwise_cap=int(cap.group(1)), amax_cap=amax_cap,
                max_adds=int(_find(r"constexpr int RR_MAX_ADDS = (\d+);", elem, "RR_MAX_ADDS").group(1)),
                max_adam=int(_find(r"#define\s+RR_MAX_ADAM\s+(\d+)", header, "RR_MAX_ADAM").group(1)),
                amax_lanes=int(_find(r"#define\s+RR_AMAX_LANES\s+(\d+)", header, "RR_AMAX_LANES").group(1)),
                amax_stride=int(_find(r"#define\s+RR_AMAX_STRIDE\s+(\d+)", header, "RR_AMAX_STRIDE").group(1)),
                adam_block=int(_find(r"blocks \+= \(t\.n \+ (\d+)\) / (\d+);", elem, "Adam's block size").group(2)))


def grid_for(work, cap, block=256):
    """rr_grid_for / pointwise_blocks: workgroups of a launch over `work` items"""
    return int(min(max(1, -(-work // block)), cap))


def walk(work, cap):
    """(passes of the grid-stride loop, items of the last pass, threads of the launch) over `work` items"""
    threads = grid_for(work, cap) * 256
    passes = -(-work // threads)
    return passes, work - (passes - 1) * threads, threads


ONE_PASS = constants()["grid_cap"] * 256                    # 2,097,152 work items
WRAP_SCALAR = 2 * ONE_PASS + 77
WRAP_VEC = 4 * (ONE_PASS + 1000) + 3
POINT_PASS = constants()["pointwise_cap"] * 256             # 262,144 rows
POINTWISE = (256 * 256, POINT_PASS, POINT_PASS + 1, 600_003)
TINY = (1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025)
TODAY = 30_030
HEAD_GROUPS = {0: 1, 1: 1, 2: 1, 3: 2, 4: 2, 5: 2, 6: 4}
HEAD_ROWS = 262_200
ADAM_SIZES = (1, 1023, 1024, 1025, 4097)
ADAM_COUNTS = (1, 64, 65, 130)
ADAM_STEPS = (1, 100_000)
ADAM_DECAYS = (0.0, 0.01)
DROP_P = (0.0, 0.1, 0.5, 0.999)
DROP_SEEDS = (0x9E3779B97F4A7C15, (1 << 63) + (5 << 32) + 12345, 77)          # two with bits above 2^32
SCALE, ALPHA, BETA = -0.75, -1.5, 0.375                                        # exact in float32; negative: -0 products


def stream_class(n, vector):
    """what a launch of one of the four two-form kernels does at n elements: passes over the 16-byte groups (vector) or the
    elements (scalar), and the length of the scalar tail of the vector form"""
    if vector:
        passes, last, threads = walk((n + 3) // 4, constants()["grid_cap"])
        return dict(passes=passes, partial=last < threads, tail=n % 4)
    passes, last, threads = walk(n, constants()["grid_cap"])
    return dict(passes=passes, partial=last < threads, tail=0)


def point_class(n):
    passes, last, threads = walk(n, constants()["pointwise_cap"])
    return dict(passes=passes, partial=last < threads, partials=grid_for(n, constants()["pointwise_cap"]))


def head_shapes(head, size_class):
    """[(M, N)] of a head in a size class"""
    G = HEAD_GROUPS[head]
    if size_class == "zero":
        return [(0, G)]
    if size_class == "tiny":
        return [(m, G) for m in TINY]
    if size_class == "today":
        return [(1001, 30 // G * G)]
    shapes = [(-(-WRAP_SCALAR // (2 * G)), 2 * G)]                       # three passes, the last partial: every head
    if head == 6:
        shapes += [(HEAD_ROWS, 8), (1, 8)]
    if head == 3:
        shapes += [(HEAD_ROWS, 2), (1, 2)]
    return shapes


# ------------------------------------------------------------------------------------------------ rr_amax_f32's launch, restated
def amax_plan(rows, cols, ld, offset):
    """vector or scalar form, work items, stride and whether the four-loads loop wraps (pack_weights.hip: rr_amax_f32)"""
    vec = offset % 4 == 0 and ld % 4 == 0 and (cols + 3) // 4 * 4 <= ld
    per_row = (cols + 3) // 4 if vec else cols
    total = rows * per_row
    stride = grid_for((total + 3) // 4, constants()["amax_cap"]) * 256
    cls = "past_four_strides" if total > 4 * stride and (total % stride) != 0 else ("below_three_strides" if total <= 3 * stride else "between")
    return dict(vec=vec, per_row=per_row, total=total, stride=stride, cls=cls, tail=cols % 4 if vec else 0)


# (rows, cols, ld) per size class and alignment class; `offset` comes from the alignment class
AMAX_WRAP = {"aligned": (3500, 1203, 1204), "all_off_1": (875, 1203, 1204), "ld_odd": (875, 1203, 1205)}
AMAX_BELOW = (7, 99, 100)                      # at most three strides of its grid in both forms
AMAX_TODAY = (1001, 30, 32)


def amax_shape(size_class, n, align):
    if size_class == "zero":
        return (0, 5, 8)
    if size_class == "tiny":
        return (1, n, (n + 3) // 4 * 4 + 4 + (1 if align == "ld_odd" else 0))
    if size_class == "today":
        return AMAX_TODAY[:2] + (AMAX_TODAY[2] + (1 if align == "ld_odd" else 0),)
    return AMAX_WRAP[align]


# ------------------------------------------------------------------------------------------------ the table
# entry point -> (forms, operands of a form: the alignment classes misalign each in turn; None: one form of kernel only)
def _relu_ops(form):
    return ("dy", "y") + {"dz": ("dz",), "acc": ("acc",), "both": ("dz", "acc")}[form]


def _sum_ops(n_adds):
    return ("dy", "y", "out") + ((f"adds[{n_adds // 2}]",) if n_adds else ())


def _axpby_ops(form):
    return {"b_null": ("a", "out"), "b_given": ("a", "b", "out"), "out_is_a": ("a", "b")}[form]


LOSSES = ("mse", "gauss_nll", "lognorm", "exp_mse", "nig")
ENTRY_POINTS = {
    "rr_relu_bwd_f32": (("dz", "acc", "both"), _relu_ops),
    "rr_relu_bwd_sum_f32": ((0, 1, 2, 15), _sum_ops),
    "rr_axpby_f32": (("b_null", "b_given", "out_is_a"), _axpby_ops),
    "rr_dropout_f32": (DROP_P, None),
    "rr_head_fwd_f32": (tuple(HEAD_GROUPS), None),
    "rr_head_bwd_f32": (tuple(HEAD_GROUPS), None),
    "rr_amax_f32": (("slot",), lambda form: ("x",)),
    "rr_digamma_f32": (("values",), None),
    "rr_adam_step_f32": (("direct", "HipAdam"), None),
}
for _k in LOSSES:
    ENTRY_POINTS[f"rr_{_k}_fwd_f32"] = (("stride1", "stride2"), None)
    ENTRY_POINTS[f"rr_{_k}_bwd_f32"] = (("stride1", "stride2"), None)
SIZE_CLASSES = ("zero", "tiny", "today", "wrap")


def size_classes(entry):
    return ("adam",) if entry == "rr_adam_step_f32" else SIZE_CLASSES


def align_classes(entry, form, size_class):
    ops_of = ENTRY_POINTS[entry][1]
    if ops_of is None:
        return ("aligned",)
    if size_class == "zero":
        return ("aligned",)
    extra = ("ld_odd",) if entry == "rr_amax_f32" else ()
    if size_class == "wrap":
        return ("aligned", "all_off_1") + extra
    return ("aligned",) + tuple(f"off1:{op}" for op in ops_of(form)) + ("all_off_1", "all_off_2", "all_off_3") + extra


def offsets(entry, form, align):
    """operand -> element offset 0 .. 3 of an alignment class"""
    ops = ENTRY_POINTS[entry][1](form)
    if align in ("aligned", "ld_odd"):
        return {op: 0 for op in ops}
    if align.startswith("all_off_"):
        return {op: int(align[-1]) for op in ops}
    assert align.startswith("off1:") and align[5:] in ops, (entry, form, align)
    return {op: int(op == align[5:]) for op in ops}


def sizes(entry, form, size_class, align):
    """the sizes a cell runs: element counts, (M, N) for the heads, (rows, cols, ld) for amax, a label for Adam"""
    if entry == "rr_adam_step_f32":
        return [f"count {c}" for c in ADAM_COUNTS] if form == "HipAdam" else \
            [f"step {s} wd {w}" for s in ADAM_STEPS for w in ADAM_DECAYS] + ["count 65 is RR_ERR_ARG"]
    if entry.startswith("rr_head_"):
        return head_shapes(form, size_class)
    if entry == "rr_amax_f32":
        if size_class == "tiny":
            return [amax_shape("tiny", n, align) for n in TINY] + [AMAX_BELOW[:2] + (AMAX_BELOW[2] + (align == "ld_odd"),)]
        return [amax_shape(size_class, None, align)]
    if size_class == "zero":
        return [0]
    if size_class == "tiny":
        return list(TINY)
    if size_class == "today":
        return [TODAY]
    if entry == "rr_digamma_f32" or entry[3:-8] in LOSSES:
        return list(POINTWISE)
    if ENTRY_POINTS[entry][1] is not None and align == "aligned":
        return [WRAP_VEC]
    return [WRAP_SCALAR]


# cells left out, with the reason: (entry point, form, size class, alignment class) -> why
EXCLUDED = {}


def cells():
    """every (entry point, form, size class, alignment class) the GPU tests run"""
    out = []
    for entry, (forms, _) in ENTRY_POINTS.items():
        for form in forms:
            for sc in size_classes(entry):
                for al in align_classes(entry, form, sc):
                    if (entry, form, sc, al) not in EXCLUDED:
                        out.append((entry, form, sc, al))
    return out


def _operands(entry, form):
    """float arrays of one launch's size that a cell generates, places, runs and compares (inputs, outputs, references)"""
    if entry == "rr_relu_bwd_sum_f32":
        return 2 * (4 + form)
    if entry.startswith("rr_head_"):
        return 4
    if entry[3:-8] in LOSSES:
        return 3 * (1 + len(LOSS_COLUMNS[entry[3:-8]])) * int(form[-1])
    return {"rr_relu_bwd_f32": 8, "rr_axpby_f32": 6, "rr_dropout_f32": 3 * len(DROP_SEEDS), "rr_amax_f32": 1, "rr_digamma_f32": 2}[entry]


def dry_enumeration():
    """cell -> (launches, float words moved on the device, elements of host-side reference work), from the table alone.
    budget_seconds() turns it into the time a GPU test of that cell may take: 0.2 ms per launch with its readback, the device
    words at 100 GB/s (a tenth of what a streaming kernel reaches: generation, placement, the kernel, the restatement and the
    comparison each pass over them), host reference work (float64 heads and losses, the dropout hash, digamma) at 5 M
    elements per second."""
    out = {}
    for entry, form, sc, al in cells():
        if entry == "rr_adam_step_f32":
            n = sum(ADAM_SIZES) * max(ADAM_COUNTS) // len(ADAM_SIZES)
            out[(entry, form, sc, al)] = (4 * len(ADAM_COUNTS), 8 * n, 8 * n)
            continue
        launches = words = host = 0
        for s in sizes(entry, form, sc, al):
            n = s if isinstance(s, int) else (s[0] * s[1] if entry.startswith("rr_head_") else s[0] * s[2])
            per = 40 if entry == "rr_amax_f32" else (len(DROP_SEEDS) if entry == "rr_dropout_f32" else 1)
            per += len(slices(n)) if entry[3:-8] in LOSSES and n > POINT_PASS else 0
            launches += per
            words += n * _operands(entry, form) * (per if entry == "rr_amax_f32" else 1)
            on_device = ENTRY_POINTS[entry][1] is not None and sc == "wrap" and entry != "rr_amax_f32"
            host += 0 if on_device else n * (len(DROP_SEEDS) if entry == "rr_dropout_f32" else 1)
        out[(entry, form, sc, al)] = (launches, words, host)
    return out


def budget_seconds(launches, words, host):
    return 2e-4 * launches + 4 * words / 100e9 + host / 5e6


# ------------------------------------------------------------------------------------------------ inputs of the elementwise kernels
def _spread(rng, n):
    return (rng.standard_normal(n) * np.exp(3.0 * rng.standard_normal(n))).astype(F32)


def plant_positions(n):
    """where +0 and -0 go: the first and the last element (the vector body and its tail), and the middle"""
    plus = sorted({0, n - 1})
    minus = [n // 2] if n > 2 else []
    return plus, minus


@functools.lru_cache(maxsize=16)
def stream_inputs(n):
    """dy, y, acc, b and 15 addends of n elements (float32, read-only).  y is a ReLU output (about half zeros); the rest
    N(0, 1) x exp(3 N(0, 1)).  dy holds +0 (first and last element) and -0 (the middle) under an open gate, adds[0] a -0."""
    rng = np.random.default_rng(SEED + n)
    y = np.maximum(rng.standard_normal(n), 0.0).astype(F32)
    d = dict(dy=_spread(rng, n), acc=_spread(rng, n), b=_spread(rng, n), adds=[_spread(rng, n) for _ in range(constants()["max_adds"])])
    plus, minus = plant_positions(n)
    for i in plus:
        d["dy"][i], y[i] = F32(0.0), F32(1.0)
    for i in minus:
        d["dy"][i], y[i], d["adds"][0][i] = F32(-0.0), F32(2.0), F32(-0.0)
    d["y"] = y
    for a in [d["dy"], d["y"], d["acc"], d["b"]] + d["adds"]:
        a.setflags(write=False)
    return d


def stream_inputs_t(n, device, seed=SEED):
    """the same recipe as whole-tensor torch operations on `device` (the wrap sizes: nothing crosses to the host)"""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed + n)

    def normal():
        return torch.randn(n, generator=gen, device=device, dtype=torch.float32)

    def spread():
        return normal() * torch.exp(3.0 * normal())
    y = torch.clamp_min(normal(), 0.0)
    d = dict(dy=spread(), acc=spread(), b=spread(), adds=[spread() for _ in range(constants()["max_adds"])])
    plus, minus = plant_positions(n)
    for i in plus:
        d["dy"][i], y[i] = 0.0, 1.0
    for i in minus:
        d["dy"][i], y[i], d["adds"][0][i] = -0.0, 2.0, -0.0
    d["y"] = y
    return d


# ------------------------------------------------------------------------------------------------ exact restatements
def relu_bwd_np(dy, y, scale, acc=None):
    """(dz, acc after) of relu_bwd_kernel / relu_bwd_scalar_kernel"""
    r = np.where(y > 0, dy * F32(scale), F32(0.0)).astype(F32)
    return r, (None if acc is None else (acc + r).astype(F32))


def relu_bwd_sum_np(dy, y, scale, adds):
    """relu_bwd_sum_kernel: adds[0 .. n-1] summed in that order from 0.f, then the gated term"""
    s = np.zeros(dy.shape, F32)
    for a in adds:
        s = (s + a).astype(F32)
    return (s + relu_bwd_np(dy, y, scale)[0]).astype(F32)


def axpby_np(alpha, a, beta, b):
    r = (F32(alpha) * a).astype(F32)
    return r if b is None else (r + (F32(beta) * b).astype(F32)).astype(F32)


def keep_scale(p):
    return F32(1.0) / (F32(1.0) - F32(p))


def dropout_np(x, p, seed):
    keep = DR.keep_mask(seed, np.arange(x.size, dtype=np.uint64), p)
    return np.where(keep, x * keep_scale(p), F32(0.0)).astype(F32)


def _f32_scalar(t, value):
    return torch.tensor(float(F32(value)), dtype=torch.float32, device=t.device)


def relu_bwd_t(dy, y, scale, acc=None):
    r = torch.where(y > 0, dy * _f32_scalar(dy, scale), torch.zeros((), dtype=torch.float32, device=dy.device))
    return r, (None if acc is None else acc + r)


def relu_bwd_sum_t(dy, y, scale, adds):
    s = torch.zeros_like(dy)
    for a in adds:
        s = s + a
    return s + relu_bwd_t(dy, y, scale)[0]


def axpby_t(alpha, a, beta, b):
    r = a * _f32_scalar(a, alpha)
    return r if b is None else r + b * _f32_scalar(a, beta)


def relu_bwd_sum_f64(dy, y, scale, adds):
    """(the float64 value, the bound a chain of n_adds + 1 float32 additions and one product allows)"""
    gate = np.where(y > 0, dy.astype(np.float64) * float(F32(scale)), 0.0)
    total, mag = gate.copy(), np.abs(gate)
    for a in adds:
        total += a.astype(np.float64)
        mag += np.abs(a.astype(np.float64))
    return total, (len(adds) + 2) * 2.0 ** -24 * mag


def bits_np(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


# ------------------------------------------------------------------------------------------------ heads
HEAD_PLANTED = tuple(F32(v) for v in (0.0, -0.0, 20.0, np.nextafter(F32(20.0), F32(np.inf)), np.nextafter(F32(20.0), F32(-np.inf)),
                                      -20.0, 88.0, -87.0, -104.0))


@functools.lru_cache(maxsize=4)
def head_inputs(M, N):
    """(raw, dout): raw = N(0, 5) with every planted value in EVERY column (rows spread over the block, as many as fit)"""
    rng = np.random.default_rng(SEED + 31 * M + N)
    raw = (5.0 * rng.standard_normal((M, N))).astype(F32)
    k = min(len(HEAD_PLANTED), M)
    for j in range(k):
        raw[j * (M - 1) // max(1, k - 1)] = HEAD_PLANTED[j]
    dout = rng.standard_normal((M, N)).astype(F32)
    raw.setflags(write=False)
    dout.setflags(write=False)
    return raw, dout


def head_error(got, ref):
    """tests/test_gpu_loss_range.py's measure of the same two entry points: max |got - ref| / (1 + |ref|), against L.BOUND"""
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (1 + np.abs(ref)))) if ref.size else 0.0


def head_expected(raw, dout, head):
    """(out, draw) in float64"""
    out, slope, col_in, _ = L.head_reference(raw, head)
    draw = np.empty_like(out)
    draw[:, col_in] = dout.astype(np.float64) * slope
    return out, draw


# ------------------------------------------------------------------------------------------------ pointwise losses
LOSS_COLUMNS = {k: L.KINDS[k][0] for k in LOSSES}


@functools.lru_cache(maxsize=None)
def loss_inputs(n):
    """the columns of tests/loss_range.py's base inputs at n rows (targets N(0, 1)), float32 and read-only"""
    rng = np.random.default_rng(SEED + 7 * n)
    sp = lambda: np.log1p(np.exp(rng.standard_normal(n)))
    d = dict(score=2 * rng.standard_normal(n), targets=rng.standard_normal(n), var=sp() + 1e-6, pos=sp() + 0.1, nu=sp() + 1e-6,
             alpha=sp() + 1.0 + 1e-6, beta=sp() + 1e-6)
    return {k: L._f32(v) for k, v in d.items()}


def loss_evaluate(kind, n, dtype=torch.float64):
    d = loss_inputs(n)
    cols = [d[c] for c in LOSS_COLUMNS[kind]]
    if kind == "nig":
        return L.nig(cols, d["targets"], False, dtype)
    return L.pointwise(kind, cols, d["targets"], dtype)


@functools.lru_cache(maxsize=None)
def loss_reference(kind, n):
    """(loss, gradients) in float64, computed once"""
    return L._freeze(loss_evaluate(kind, n))


def slices(n):
    """[lo, hi) row ranges of at most POINT_PASS rows whose lengths are powers of two: with gloss = float32(1 / n) * length a
    backward launch over a slice divides by its length EXACTLY, so it scales by the float32(1 / n) of the whole launch"""
    out, lo = [], 0
    while lo < n:
        length = min(POINT_PASS, 1 << ((n - lo).bit_length() - 1))
        out.append((lo, lo + length))
        lo += length
    return out


# ------------------------------------------------------------------------------------------------ digamma
DIGAMMA_ROOT = 1.4616321449683623
DIGAMMA_SPECIAL = (F32(np.finfo(np.float32).tiny), F32(1e-40), F32(0.0), F32(-1.0))


@functools.lru_cache(maxsize=None)
def digamma_points():
    root = F32(DIGAMMA_ROOT)
    pts = list(DIGAMMA_SPECIAL) + [np.nextafter(root, F32(0)), root, np.nextafter(root, F32(2))]
    pts += [F32(k / 2) for k in range(1, 121)]
    pts += list(np.logspace(-6, 6, 4000).astype(F32))
    a = np.asarray(pts, F32)
    a.setflags(write=False)
    return a


def digamma_input(n):
    """n values: the points in order (the special ones first), truncated or repeated"""
    return np.resize(digamma_points(), n).astype(F32)


def digamma_reference(x):
    return torch.digamma(torch.from_numpy(np.asarray(x, F32)).double()).numpy()


def digamma_check(got, x):
    """-> (largest |got - ref| / (2^-24 |ref| + 1e-10) over the finite results, count of non-finite ones); asserts that a
    non-finite reference (as float32) is met exactly.  2^-24 |ref|: the one float32 rounding of a double result; 1e-10: the
    first omitted term of the series at its switch point x = 6, 691 / 32760 / 6^12 = 9.7e-12"""
    ref = digamma_reference(x)
    with np.errstate(over="ignore"):
        ref32 = ref.astype(F32)
    got = np.asarray(got, F32)
    odd = ~np.isfinite(ref32)
    assert np.array_equal(got[odd], ref32[odd], equal_nan=True), (x[odd], got[odd], ref32[odd])
    if odd.all():
        return 0.0, int(odd.sum())
    err = np.abs(got[~odd].astype(np.float64) - ref[~odd]) / (2.0 ** -24 * np.abs(ref[~odd]) + 1e-10)
    return float(err.max()), int(odd.sum())


# ------------------------------------------------------------------------------------------------ amax
AMAX_PAD = F32(1e30)


@functools.lru_cache(maxsize=4)
def amax_block(rows, cols, ld):
    """[rows, ld] float32: N(0, 1) in the valid columns, 1e30 in the pad columns"""
    rng = np.random.default_rng(SEED + rows * 131 + cols)
    x = np.full((rows, ld), AMAX_PAD, F32)
    x[:, :cols] = rng.standard_normal((rows, cols)).astype(F32)
    x.setflags(write=False)
    return x


def amax_positions(rows, cols):
    """(row, column) of the planted maxima: first element, last valid element, the last valid column of a middle row (next to
    the pad columns), and 30 seeded random positions"""
    rng = np.random.default_rng(SEED + rows + cols)
    fixed = [(0, 0), (rows - 1, cols - 1), (rows // 2, cols - 1)]
    return fixed + [(int(rng.integers(rows)), int(rng.integers(cols))) for _ in range(30)]


def amax_np(x, cols):
    """max |x| over the valid region, NaNs skipped, as float32"""
    v = np.abs(np.asarray(x, F32)[:, :cols])
    return F32(np.fmax.reduce(v, axis=None)) if v.size else F32(0.0)


# ------------------------------------------------------------------------------------------------ Adam
def adam_np(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay):
    """(p, m, v) after adam_many_kernel's update of one tensor: float64 arithmetic in the kernel's statement order, rounded to
    float32 where the kernel rounds (the decayed gradient, both moments, the parameter)"""
    p64, m64, v64 = (np.asarray(a, F32).astype(np.float64) for a in (p, m, v))
    step_size = lr / (1.0 - math.pow(beta1, float(step)))
    bc2_sqrt = math.sqrt(1.0 - math.pow(beta2, float(step)))
    g64 = np.asarray(g, F32).astype(np.float64)
    if weight_decay != 0.0:
        g64 = g64 + weight_decay * p64
    gf = g64.astype(F32).astype(np.float64)
    m_new = (m64 + (1.0 - beta1) * (gf - m64)).astype(F32)
    v_new = (beta2 * v64 + (1.0 - beta2) * gf * gf).astype(F32)
    denom = np.sqrt(v_new.astype(np.float64)) / bc2_sqrt + eps
    p_new = (p64 - step_size * m_new.astype(np.float64) / denom).astype(F32)
    return p_new, m_new, v_new


def ulps(a, b):
    """distance of two float32 arrays in units in the last place (both finite)"""
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def adam_tensors(sizes_, seed):
    """[(p, g, m, v)] float32 per size; m and v as after some steps (v >= 0)"""
    rng = np.random.default_rng(SEED + seed)
    out = []
    for n in sizes_:
        out.append((rng.standard_normal(n).astype(F32), _spread(rng, n) * F32(1e-2), (rng.standard_normal(n) * 1e-2).astype(F32),
                    (rng.standard_normal(n) ** 2 * 1e-4).astype(F32)))
    return out
