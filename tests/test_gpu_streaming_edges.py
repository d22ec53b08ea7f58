"""The streaming kernels past one grid pass and at 16-byte edges: every cell of tests/streaming_edges.py's table on the device.

relu_bwd, relu_bwd_sum, axpby and dropout against their exact restatements, bit for bit (the sign of zero included); the heads
and the pointwise losses against float64 under tests/loss_range.py's measure and bound, their gradients past one pass also
against the same rows in one-pass slices, bit for bit; rr_amax_f32 against numpy's max |x|, as bits; rr_digamma_f32 against
torch.digamma in float64; rr_adam_step_f32 and train_utils.HipAdam against adam_np within one unit in the last place.  Every
output and every acc lies between 8 guard floats holding a sentinel NaN, and a buffer the call must not write starts as the
same sentinel: the guards keep their bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import loss_range as L
from tests import streaming_edges as S

from reactranker_amd import _lib
from reactranker_amd._lib import lib, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
RR_OK, RR_ERR_ARG = 0, -1
NEG_ZERO = -2 ** 31


# ------------------------------------------------------------------------------------------------ guarded buffers
class Placed:
    """n floats at element offset `off` (0 .. 3) behind S.GUARD guard floats of a fresh buffer whose every other word holds the
    sentinel; values: what the n floats start as (None: the sentinel too - an output)"""

    def __init__(self, values, n, off=0):
        self.n, self.start = int(n), S.GUARD + int(off)
        self.buf = torch.full((self.n + 2 * S.GUARD + 4,), S.SENTINEL_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
        self.view = self.buf[self.start:self.start + self.n]
        if values is not None and self.n:
            self.view.copy_(values if isinstance(values, torch.Tensor) else torch.from_numpy(np.array(values, dtype=np.float32)))
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * self.start)

    def guards_hold(self):
        b = self.buf.view(torch.int32)
        return bool((b[:self.start] == S.SENTINEL_BITS).all()) and bool((b[self.start + self.n:] == S.SENTINEL_BITS).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == S.SENTINEL_BITS).all())

    def bits(self):
        return self.view.view(torch.int32) if self.n else self.view.new_empty(0, dtype=torch.int32)

    def host(self):
        return self.view.cpu().numpy()


def optr(p):
    return None if p is None else p.ptr


def same_bits(placed, want):
    """the placed floats against a numpy array or a device tensor, as bits -> count of differing elements"""
    if isinstance(want, torch.Tensor):
        return int((placed.bits() != want.view(torch.int32)).sum())
    return int((placed.host().view(np.int32) != S.bits_np(want)).sum())


@functools.lru_cache(maxsize=None)
def dev_inputs(n):
    d = S.stream_inputs(n)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    return {k: ([up(a) for a in v] if k == "adds" else up(v)) for k, v in d.items()}


@functools.lru_cache(maxsize=2)
def wrap_inputs(n):
    return S.stream_inputs_t(n, DEV)


def inputs_for(n, size_class):
    """(device tensors, host arrays or None): at the wrap sizes everything stays on the device"""
    if size_class == "wrap":
        return wrap_inputs(n), None
    return dev_inputs(n), S.stream_inputs(n)


def cells_of(entry):
    return [c[1:] for c in S.cells() if c[0] == entry]


def cell_id(c):
    return "-".join(str(x) for x in c).replace(":", ".").replace("[", "").replace("]", "")


def all_off(align):
    return int(align[-1]) if align.startswith("all_off_") else 0


def zero_signs(placed):
    """(+0 count, -0 count) among the placed floats"""
    b = placed.bits()
    return int((b == 0).sum()), int((b == NEG_ZERO).sum())


# ------------------------------------------------------------------------------------------------ relu_bwd
@pytest.mark.parametrize("cell", cells_of("rr_relu_bwd_f32"), ids=cell_id)
def test_relu_bwd(cell, parity_log):
    form, sc, align = cell
    off = S.offsets("rr_relu_bwd_f32", form, align)
    for n in S.sizes("rr_relu_bwd_f32", form, sc, align):
        t, h = inputs_for(n, sc) if n else (dev_inputs(1), None)
        dy, y = Placed(t["dy"][:n], n, off["dy"]), Placed(t["y"][:n], n, off["y"])
        dz = Placed(None, n, off["dz"]) if form in ("dz", "both") else None
        acc = Placed(t["acc"][:n], n, off["acc"]) if form in ("acc", "both") else None
        st = lib().rr_relu_bwd_f32(dy.ptr, y.ptr, S.SCALE, optr(dz), optr(acc), n, stream())
        assert st == RR_OK, (n, st)
        torch.cuda.synchronize()
        for p in (dy, y, dz, acc):
            assert p is None or p.guards_hold(), (n, cell)
        if n == 0:
            continue
        if h is None:
            want_dz, want_acc = S.relu_bwd_t(t["dy"], t["y"], S.SCALE, t["acc"] if acc else None)
        else:
            want_dz, want_acc = S.relu_bwd_np(h["dy"], h["y"], S.SCALE, h["acc"] if acc else None)
        bad = (same_bits(dz, want_dz) if dz else 0) + (same_bits(acc, want_acc) if acc else 0)
        Hh.record(f"relu_bwd {form} {align}: elements whose bits differ from the restatement", bad, 0)
        assert bad == 0, (n, cell, bad)
        assert same_bits(dy, t["dy"][:n]) == 0 and same_bits(y, t["y"][:n]) == 0          # the inputs are as they were
        if dz:
            assert zero_signs(dz)[1] >= 1                              # a -0 product came out as -0
    parity_log(f"relu_bwd {cell_id(cell)}: n = {S.sizes('rr_relu_bwd_f32', form, sc, align)}, bit for bit, guards intact")


# ------------------------------------------------------------------------------------------------ relu_bwd_sum
@pytest.mark.parametrize("cell", cells_of("rr_relu_bwd_sum_f32"), ids=cell_id)
def test_relu_bwd_sum(cell, parity_log):
    n_adds, sc, align = cell
    off = S.offsets("rr_relu_bwd_sum_f32", n_adds, align)
    for n in S.sizes("rr_relu_bwd_sum_f32", n_adds, sc, align):
        t, h = inputs_for(n, sc) if n else (dev_inputs(1), None)
        dy, y, out = Placed(t["dy"][:n], n, off["dy"]), Placed(t["y"][:n], n, off["y"]), Placed(None, n, off["out"])
        adds = [Placed(t["adds"][k][:n], n, off.get(f"adds[{k}]", all_off(align))) for k in range(n_adds)]
        arr = (C.c_void_p * max(1, n_adds))(*[a.ptr for a in adds])
        st = lib().rr_relu_bwd_sum_f32(dy.ptr, y.ptr, S.SCALE, arr, n_adds, out.ptr, n, stream())
        assert st == RR_OK, (n, st)
        torch.cuda.synchronize()
        assert out.guards_hold() and (n > 0 or out.untouched()), (n, cell)
        if n == 0:
            continue
        if h is None:
            want = S.relu_bwd_sum_t(t["dy"], t["y"], S.SCALE, t["adds"][:n_adds])
        else:
            want = S.relu_bwd_sum_np(h["dy"], h["y"], S.SCALE, h["adds"][:n_adds])
        bad = same_bits(out, want)
        Hh.record(f"relu_bwd_sum n_adds {n_adds} {align}: elements whose bits differ from the restatement", bad, 0)
        assert bad == 0, (n, cell, bad)
        assert all(same_bits(a, t["adds"][k][:n]) == 0 for k, a in enumerate(adds))
    parity_log(f"relu_bwd_sum {cell_id(cell)}: n = {S.sizes('rr_relu_bwd_sum_f32', n_adds, sc, align)}, bit for bit, guards intact")


# ------------------------------------------------------------------------------------------------ axpby
@pytest.mark.parametrize("cell", cells_of("rr_axpby_f32"), ids=cell_id)
def test_axpby(cell, parity_log):
    """b null (the sign of a -0 product is kept by the 16-byte body, its tail and the scalar form alike), b given, and the one
    aliased form the package has: out is a (functions.py: ReactionModelFn.backward, axpby(1.0, a, 1.0, b, out=a))"""
    form, sc, align = cell
    off = S.offsets("rr_axpby_f32", form, align)
    for n in S.sizes("rr_axpby_f32", form, sc, align):
        t, h = inputs_for(n, sc) if n else (dev_inputs(1), None)
        a = Placed(t["dy"][:n], n, off["a"])
        b = None if form == "b_null" else Placed(t["b"][:n], n, off["b"])
        out = a if form == "out_is_a" else Placed(None, n, off["out"])
        alpha, beta = (1.0, 1.0) if form == "out_is_a" else (S.ALPHA, S.BETA)
        st = lib().rr_axpby_f32(alpha, a.ptr, beta, optr(b), out.ptr, n, stream())
        assert st == RR_OK, (n, st)
        torch.cuda.synchronize()
        assert out.guards_hold() and (n > 0 or form == "out_is_a" or out.untouched()), (n, cell)
        if n == 0:
            continue
        if h is None:
            want = S.axpby_t(alpha, t["dy"], beta, None if b is None else t["b"])
        else:
            want = S.axpby_np(alpha, h["dy"], beta, None if b is None else h["b"])
        bad = same_bits(out, want)
        Hh.record(f"axpby {form} {align}: elements whose bits differ from the restatement (zero signs included)", bad, 0)
        assert bad == 0, (n, cell, bad)
        if form == "b_null":                                           # +0 at the first and the last element times alpha < 0
            got = out.bits()
            assert int(got[0]) == NEG_ZERO and int(got[n - 1]) == NEG_ZERO, (n, cell)
        assert b is None or same_bits(b, t["b"][:n]) == 0
    parity_log(f"axpby {cell_id(cell)}: n = {S.sizes('rr_axpby_f32', form, sc, align)}, bit for bit, guards intact")


# ------------------------------------------------------------------------------------------------ dropout
def dropout_input(n):
    if n <= S.TODAY:
        return np.array(S.stream_inputs(n)["dy"]) if n else np.zeros(0, np.float32)
    x = np.random.default_rng(S.SEED + n).standard_normal(n).astype(np.float32)
    x[[0, n // 2, n - 1]] = np.float32(-0.0)
    return x


@pytest.mark.parametrize("cell", cells_of("rr_dropout_f32"), ids=cell_id)
def test_dropout(cell, parity_log):
    p, sc, _ = cell
    for n in S.sizes("rr_dropout_f32", p, sc, "aligned"):
        x_np = dropout_input(n)
        x = Placed(x_np, n)
        for seed in (S.DROP_SEEDS[1:2] if sc == "wrap" else S.DROP_SEEDS):
            out = Placed(None, n)
            st = lib().rr_dropout_f32(x.ptr, n, p, seed, out.ptr, stream())
            assert st == RR_OK, (n, st)
            torch.cuda.synchronize()
            assert out.guards_hold() and (n > 0 or out.untouched())
            if n == 0:
                continue
            bad = same_bits(out, S.dropout_np(x_np, p, seed))
            Hh.record(f"dropout p {p}: elements whose bits differ from the restatement", bad, 0)
            assert bad == 0, (n, p, hex(seed), bad)
            if p == 0.0:
                assert same_bits(out, x_np) == 0                       # x bit for bit
    parity_log(f"dropout {cell_id(cell)}: n = {S.sizes('rr_dropout_f32', p, sc, 'aligned')}, mask and scale bit for bit")


# ------------------------------------------------------------------------------------------------ heads
def check(what, err, bound):
    Hh.record(what, err, bound)
    print(f"[streaming edges] {what}: {err:.3e} (bound {bound:g})")
    assert err <= bound, f"{what}: {err:.3e} > {bound:g}"


@pytest.mark.parametrize("sc", S.SIZE_CLASSES)
@pytest.mark.parametrize("head", tuple(S.HEAD_GROUPS))
def test_heads(head, sc, parity_log):
    assert ("rr_head_fwd_f32", head, sc, "aligned") in S.cells() and ("rr_head_bwd_f32", head, sc, "aligned") in S.cells()
    for M, N in S.head_shapes(head, sc):
        raw_np, dout_np = S.head_inputs(M, N)
        raw, dout = Placed(raw_np.reshape(-1), M * N), Placed(dout_np.reshape(-1), M * N)
        out, draw = Placed(None, M * N), Placed(None, M * N)
        assert lib().rr_head_fwd_f32(raw.ptr, M, N, head, out.ptr, stream()) == RR_OK
        assert lib().rr_head_bwd_f32(dout.ptr, raw.ptr, M, N, head, draw.ptr, stream()) == RR_OK
        torch.cuda.synchronize()
        assert out.guards_hold() and draw.guards_hold()
        if M == 0:
            assert out.untouched() and draw.untouched()
            continue
        want_out, want_draw = S.head_expected(raw_np, dout_np, head)
        check(f"head {head} {sc} forward", S.head_error(out.host().reshape(M, N), want_out), L.BOUND)
        check(f"head {head} {sc} backward", S.head_error(draw.host().reshape(M, N), want_draw), L.BOUND)
    parity_log(f"head {head} {sc}: [M, N] = {S.head_shapes(head, sc)}")


# ------------------------------------------------------------------------------------------------ amax
def slot_lanes(slot):
    c = S.constants()
    return slot.host()[::c["amax_stride"]][:c["amax_lanes"]]


def amax_run(x, rows, cols, ld, preset=0.0):
    """-> (status, the slot as the maximum over its lanes, the Placed slot)"""
    c = S.constants()
    slot = Placed(np.full(c["amax_lanes"] * c["amax_stride"], preset, np.float32), c["amax_lanes"] * c["amax_stride"])
    st = lib().rr_amax_f32(x.ptr, rows, cols, ld, slot.ptr, stream())
    torch.cuda.synchronize()
    assert slot.guards_hold()
    between = np.delete(slot.host(), np.arange(c["amax_lanes"]) * c["amax_stride"])
    assert (between.view(np.int32) == np.float32(preset).view(np.int32)).all()          # only the lanes are written
    return st, np.float32(slot_lanes(slot).max()), slot


def as_bits(v):
    return int(np.float32(v).view(np.int32))


@pytest.mark.parametrize("cell", cells_of("rr_amax_f32"), ids=cell_id)
def test_amax(cell, parity_log):
    _, sc, align = cell
    off = S.offsets("rr_amax_f32", "slot", align)["x"]
    launches = 0
    for rows, cols, ld in S.sizes("rr_amax_f32", "slot", sc, align):
        plan = S.amax_plan(rows, cols, ld, off)
        assert plan["vec"] == (align == "aligned"), (cell, rows, cols, ld)
        if sc == "wrap":
            assert plan["cls"] == "past_four_strides"
        block = S.amax_block(max(rows, 1), cols, ld)
        x = Placed(block.reshape(-1), max(rows, 1) * ld, off)
        if rows == 0:
            st, got, slot = amax_run(x, 0, cols, ld, preset=0.5)
            assert st == RR_OK and (slot.host().view(np.int32) == as_bits(0.5)).all()
            continue
        x2d = x.view.view(rows, ld)
        base = S.amax_np(block, cols)
        st, got, _ = amax_run(x, rows, cols, ld)
        assert st == RR_OK and as_bits(got) == as_bits(base), (cell, rows, cols, ld, got, base)
        # the unique largest magnitude, negative, at each planted position
        for k, (r, c) in enumerate(S.amax_positions(rows, cols)):
            big = np.float32(1000.0 + k)
            keep = float(x2d[r, c])
            x2d[r, c] = -float(big)
            st, got, _ = amax_run(x, rows, cols, ld)
            x2d[r, c] = keep
            assert st == RR_OK and as_bits(got) == as_bits(big), (cell, (rows, cols, ld), (r, c), got)
            launches += 1
        # a NaN elsewhere is skipped; an inf wins
        r, c = rows // 3, cols // 2
        keep = float(x2d[r, c])
        if rows * cols > 1:
            x2d[r, c] = float("nan")
            want = S.amax_np(x2d.cpu().numpy(), cols)
            st, got, _ = amax_run(x, rows, cols, ld)
            assert st == RR_OK and np.isfinite(want) and as_bits(got) == as_bits(want), (cell, got, want)
        x2d[rows - 1, 0] = float("-inf")
        st, got, _ = amax_run(x, rows, cols, ld)
        assert st == RR_OK and as_bits(got) == as_bits(np.inf), (cell, got)
        x2d[r, c], x2d[rows - 1, 0] = keep, float(block[rows - 1, 0])
        # a slot preset to a larger value keeps it, one preset to a smaller value is raised
        st, got, slot = amax_run(x, rows, cols, ld, preset=1e6)
        assert st == RR_OK and (slot.host().view(np.int32) == as_bits(1e6)).all()
        st, got, slot = amax_run(x, rows, cols, ld, preset=1e-3)
        assert st == RR_OK and as_bits(got) == as_bits(max(base, np.float32(1e-3))), (cell, got, base)
        # an all-zero block (the pad columns keep their 1e30) leaves the slot untouched
        x2d[:, :cols] = 0.0
        st, got, slot = amax_run(x, rows, cols, ld, preset=0.5)
        assert st == RR_OK and (slot.host().view(np.int32) == as_bits(0.5)).all(), cell
        x2d[:, :cols] = -0.0
        st, got, slot = amax_run(x, rows, cols, ld, preset=0.0)
        assert st == RR_OK and (slot.host().view(np.int32) == 0).all(), cell
        assert x.guards_hold()
    Hh.record(f"amax {sc} {align}: launches whose slot differs from numpy's max |x| as bits", 0, 0)
    parity_log(f"amax {cell_id(cell)}: [rows, cols, ld] = {S.sizes('rr_amax_f32', 'slot', sc, align)}, {launches} planted maxima, "
               "NaN skipped, inf wins, presets kept / raised, zero block untouched: all equal as bits")


# ------------------------------------------------------------------------------------------------ digamma
@pytest.mark.parametrize("sc", S.SIZE_CLASSES)
def test_digamma(sc, parity_log):
    assert ("rr_digamma_f32", "values", sc, "aligned") in S.cells()
    for n in S.sizes("rr_digamma_f32", "values", sc, "aligned"):
        x_np = S.digamma_input(n)
        x, y = Placed(x_np, n), Placed(None, n)
        assert lib().rr_digamma_f32(x.ptr, n, y.ptr, stream()) == RR_OK
        torch.cuda.synchronize()
        assert y.guards_hold() and (n > 0 or y.untouched())
        if n == 0:
            continue
        err, odd = S.digamma_check(y.host(), x_np)
        check(f"digamma n {n}: |got - ref| / (2^-24 |ref| + 1e-10)", err, 1.0)
        parity_log(f"digamma n {n}: {odd} non-finite results equal to the float32 cast of torch.digamma (float64)")


# ------------------------------------------------------------------------------------------------ pointwise losses
def strided(values, n, stride):
    """a column of n floats `stride` apart (the words between hold the sentinel) -> Placed"""
    p = Placed(None, n * stride)
    if n:
        p.view[::stride].copy_(torch.from_numpy(np.array(values, dtype=np.float32)))
    return p


def at(p, row, stride):
    return C.c_void_p(p.ptr.value + 4 * row * stride)


def loss_call(kind, direction, cols, stride, targets, lo, n, tail):
    """one launch over rows [lo, lo + n) of the columns; tail: (loss, partial) or (gloss, outputs, dstride)"""
    ins = [at(c, lo, stride) for c in cols]
    t = at(targets, lo, 1)
    if direction == "fwd":
        loss, partial = tail
        if kind == "nig":
            args = [x for c in ins for x in (c, stride)] + [t, n, 0, L.NIG_LAM, L.NIG_EPS, loss.ptr, partial.ptr]
        elif kind in ("mse", "exp_mse"):
            args = [ins[0], stride, t, n, loss.ptr, partial.ptr]
        else:
            args = [ins[0], ins[1], stride, t, n, loss.ptr, partial.ptr]
    else:
        gloss, outs, dstride = tail
        douts = [at(o, lo, dstride) for o in outs]
        if kind == "nig":
            args = [x for c in ins for x in (c, stride)] + [t, n, 0, L.NIG_LAM, gloss.ptr] + douts + [dstride]
        elif kind in ("mse", "exp_mse"):
            args = [ins[0], stride, t, n, gloss.ptr, douts[0], dstride]
        else:
            args = [ins[0], ins[1], stride, t, n, gloss.ptr] + douts + [dstride]
    return getattr(lib(), f"rr_{kind}_{direction}_f32")(*args, stream())


def strided_ok(p, stride):
    """the words between the rows of a strided output still hold the sentinel"""
    if stride == 1 or p.n == 0:
        return True
    keep = torch.ones(p.n, dtype=torch.bool, device=DEV)
    keep[::stride] = False
    return bool((p.bits()[keep] == S.SENTINEL_BITS).all())


@pytest.mark.parametrize("sc", S.SIZE_CLASSES)
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("kind", S.LOSSES)
def test_pointwise_loss(kind, stride, sc, parity_log):
    form = f"stride{stride}"
    assert (f"rr_{kind}_fwd_f32", form, sc, "aligned") in S.cells() and (f"rr_{kind}_bwd_f32", form, sc, "aligned") in S.cells()
    names = S.LOSS_COLUMNS[kind]
    for n in S.sizes(f"rr_{kind}_fwd_f32", form, sc, "aligned"):
        d = S.loss_inputs(max(n, 1))
        cols = [strided(d[c][:n], n, stride) for c in names]
        targets = Placed(d["targets"][:n], n)
        loss, partial = Placed(None, 1), Placed(None, int(lib().rr_pointwise_partial_count(n)))
        assert loss_call(kind, "fwd", cols, stride, targets, 0, n, (loss, partial)) == RR_OK
        gloss = Placed(np.ones(1, np.float32), 1)
        outs = [Placed(None, n * stride) for _ in names]
        assert loss_call(kind, "bwd", cols, stride, targets, 0, n, (gloss, outs, stride)) == RR_OK
        torch.cuda.synchronize()
        assert loss.guards_hold() and partial.guards_hold() and all(o.guards_hold() and strided_ok(o, stride) for o in outs)
        if n == 0:
            assert np.isnan(loss.host()[0]) and all(o.untouched() for o in outs)       # the mean of nothing; no gradient written
            continue
        ref = S.loss_reference(kind, n)
        check(f"{kind} {form} loss", L.value_error(kind, float(loss.host()[0]), ref[0]), L.BOUND)
        for name, o, r in zip(names, outs, ref[1]):
            check(f"{kind} {form} d {name}", L.grad_error(o.host()[::stride], r), L.BOUND)
        if n > S.POINT_PASS:                                           # the wrap on its own: the same rows in one-pass slices
            sliced = [Placed(None, n * stride) for _ in names]
            scale = np.float32(1.0) / np.float32(n)
            for lo, hi in S.slices(n):
                g = Placed(np.array([scale * np.float32(hi - lo)], np.float32), 1)
                assert float(g.host()[0]) / (hi - lo) == float(scale)
                assert loss_call(kind, "bwd", cols, stride, targets, lo, hi - lo, (g, sliced, stride)) == RR_OK
            torch.cuda.synchronize()
            bad = sum(int((a.bits() != b.bits()).sum()) for a, b in zip(outs, sliced))
            Hh.record(f"{kind} {form}: gradient entries past one pass that differ from the one-pass slices", bad, 0)
            assert bad == 0, (kind, n, stride, bad)
            parity_log(f"{kind} {form} n {n}: gradients == {len(S.slices(n))} one-pass slices bit for bit")


# ------------------------------------------------------------------------------------------------ Adam
def adam_descs(tensors):
    arr = (_lib.AdamTensor * max(1, len(tensors)))()
    for j, (p, g, m, v) in enumerate(tensors):
        arr[j].p, arr[j].g, arr[j].m, arr[j].v, arr[j].n = p.ptr.value, (g.ptr.value if g is not None else None), m.ptr.value, v.ptr.value, p.n
    return arr


def adam_compare(label, got, want):
    """parameters and both moments within one unit in the last place of the restatement -> count of differing elements"""
    differing = 0
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got, want):
        u = S.ulps(a, b)
        differing += int((u != 0).sum())
        assert int(u.max()) <= 1, (label, name, int(u.max()))
    Hh.record(f"{label}: elements one unit in the last place from the restatement", differing, None)
    return differing


@pytest.mark.parametrize("wd", S.ADAM_DECAYS)
@pytest.mark.parametrize("step", S.ADAM_STEPS)
def test_adam_step_direct(step, wd, parity_log):
    """the five block-edge sizes, a descriptor without a gradient in the middle of the list and a tensor whose gradient is zero"""
    assert ("rr_adam_step_f32", "direct", "adam", "aligned") in S.cells()
    host = S.adam_tensors(S.ADAM_SIZES + (1025, 300), seed=step)
    host[5] = (host[5][0], np.zeros_like(host[5][1]), host[5][2], host[5][3])          # an all-zero gradient
    order = [0, 1, 2, 6, 3, 4, 5]                                                      # tensor 6 sits in the middle, g == NULL
    placed = [tuple(Placed(a, a.size) if (k != 1 or i != 6) else None for k, a in enumerate(host[i])) for i in order]
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    st = lib().rr_adam_step_f32(C.cast(adam_descs(placed), C.c_void_p), len(placed), step, lr, b1, b2, eps, wd, stream())
    assert st == RR_OK
    torch.cuda.synchronize()
    differing = total = 0
    for i, (p, g, m, v) in zip(order, placed):
        assert p.guards_hold() and m.guards_hold() and v.guards_hold()
        if g is None:
            assert all(same_bits(x, host[i][k]) == 0 for k, x in ((0, p), (2, m), (3, v)))     # skipped: nothing written
            continue
        want = S.adam_np(*host[i], step, lr, b1, b2, eps, wd)
        differing += adam_compare(f"adam direct step {step} wd {wd}", (p.host(), m.host(), v.host()), want)
        total += 3 * p.n
        assert same_bits(g, host[i][1]) == 0
    parity_log(f"adam direct step {step} wd {wd}: {differing} of {total} values one ulp from the float64 restatement, the rest equal")


def test_adam_step_refuses_more_than_its_limit():
    assert "count 65 is RR_ERR_ARG" in S.sizes("rr_adam_step_f32", "direct", "adam", "aligned")
    cap = S.constants()["max_adam"]
    assert cap == _lib.RR_MAX_ADAM
    host = S.adam_tensors((3,) * (cap + 1), seed=5)
    placed = [tuple(Placed(a, a.size) for a in t) for t in host]
    args = (1, 1e-3, 0.9, 0.999, 1e-8, 0.0, stream())
    assert lib().rr_adam_step_f32(C.cast(adam_descs(placed), C.c_void_p), cap + 1, *args) == RR_ERR_ARG
    torch.cuda.synchronize()
    assert all(same_bits(x, a) == 0 for t, h in zip(placed, host) for x, a in zip(t, h))
    assert lib().rr_adam_step_f32(C.cast(adam_descs(placed), C.c_void_p), 0, *args) == RR_OK
    assert lib().rr_adam_step_f32(C.cast(adam_descs(placed[:cap]), C.c_void_p), cap, *args) == RR_OK
    torch.cuda.synchronize()
    for (p, g, m, v), h in zip(placed[:cap], host):
        adam_compare("adam direct 64 tensors", (p.host(), m.host(), v.host()), S.adam_np(*h, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0))
    assert all(same_bits(x, a) == 0 for x, a in zip(placed[cap], host[cap]))


@pytest.mark.parametrize("count", S.ADAM_COUNTS)
def test_hip_adam_in_chunks(count, parity_log):
    """HipAdam over `count` tensors, two steps; every third tensor has no gradient in the first step, so the second step has two
    step counts inside one group.  Each step against adam_np from the state the device held before it; above 64 tensors also
    against separate optimizers of at most 64, bit for bit."""
    from reactranker_amd.train_utils import HipAdam
    assert f"count {count}" in S.sizes("rr_adam_step_f32", "HipAdam", "adam", "aligned")
    sizes_ = [S.ADAM_SIZES[i % len(S.ADAM_SIZES)] for i in range(count)]
    host = S.adam_tensors(sizes_, seed=count)
    wd, lr = 0.01, 1e-3
    cap = _lib.RR_MAX_ADAM

    def params():
        return [torch.nn.Parameter(torch.from_numpy(h[0].copy()).to(DEV)) for h in host]
    P, Q = params(), params()
    whole = HipAdam([{"params": P, "lr": lr, "weight_decay": wd}])
    parts = [HipAdam([{"params": Q[i:i + cap], "lr": lr, "weight_decay": wd}]) for i in range(0, count, cap)]
    differing = total = 0
    for it in range(2):
        rng = np.random.default_rng(S.SEED + count + it)
        grads = [None if (it == 0 and i % 3 == 1 and count > 1) else (rng.standard_normal(n) * 10.0 ** (it - 2)).astype(np.float32)
                 for i, n in enumerate(sizes_)]
        before = []
        for p in P:
            s = whole.state.get(p) or {}
            zero = np.zeros(p.numel(), np.float32)
            before.append((p.detach().cpu().numpy().copy(), s["exp_avg"].cpu().numpy() if s else zero,
                           s["exp_avg_sq"].cpu().numpy() if s else zero, int(s["step"]) if s else 0))
        for group in (P, Q):
            for p, g in zip(group, grads):
                p.grad = None if g is None else torch.from_numpy(g).to(DEV)
        whole.step()
        for o in parts:
            o.step()
        torch.cuda.synchronize()
        steps = set()
        for i, (p, q, g) in enumerate(zip(P, Q, grads)):
            if g is None:
                assert np.array_equal(p.detach().cpu().numpy(), before[i][0]) and p not in whole.state
                continue
            s = whole.state[p]
            steps.add(int(s["step"]))
            assert int(s["step"]) == before[i][3] + 1
            got = (p.detach().cpu().numpy(), s["exp_avg"].cpu().numpy(), s["exp_avg_sq"].cpu().numpy())
            want = S.adam_np(before[i][0], g, before[i][1], before[i][2], int(s["step"]), lr, 0.9, 0.999, 1e-8, wd)
            differing += adam_compare(f"HipAdam {count} tensors", got, want)
            total += 3 * p.numel()
            own = [o for o in parts if q in o.state][0].state[q]
            for a, b in ((p.detach(), q.detach()), (s["exp_avg"], own["exp_avg"]), (s["exp_avg_sq"], own["exp_avg_sq"])):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (count, it, i)
        assert len(steps) == (2 if (it == 1 and count > 1) else 1), steps
    parity_log(f"HipAdam {count} tensors, 2 steps: {differing} of {total} values one ulp from the restatement, the rest equal; "
               f"{len(parts)} optimizers of at most {cap} give the same bits")
