"""The fused tail of linear_split_kernel (reactranker_amd/csrc/linear_split.hip, mfma_block / launch_split_tail): where the last
k-step of a 12-wave one-column-block launch has at most 16 live columns, its six products per tile are issued as three MFMAs
- [w2|w1].[x0|x1], [w0|w1].[x2|x0], [w0|w0].[x1|x0], each operand the lanes 0-31 of two terms side by side - against the
six-MFMA step that RR_NO_TAIL_FUSE=1 restores.

Shapes.  rr_linear_f32 sends N <= 304 to the 12-wave geometry only above 8192 rows, so the row counts are 43 full blocks of
192 rows followed by the three endings that matter: 16 rows (one wave), 197 (a full block and 5 rows) and 389 (two blocks and
5 rows).  A wave WITHOUT rows in the kernel's sense (uwave >= nw: the persistent form's and the balanced grid's short last
blocks) needs more row blocks than CUs: 192 * CUs + 197 rows, at the model's K only, the plain forms once more with
RR_NO_PERSIST=1.  N = 300, 304; K = 12 (one step that is itself the tail), 44 and 48 (tails of 12 and 16), 76 (three steps:
the odd-count twin behind its pair loop), 300, and 61 | 300;
K = 49 (17 live columns) is the control that must take the six-MFMA step and equal the knob's bits on random inputs - 52
for the sign-bit form, whose k1 must be a multiple of 4.

(a) exact inputs: +-(a + b 2^-9 + c 2^-18), a in 1..3, b, c in 0 / 1 (c only next to b: with b = 0 the SECOND term of the
split would be c 2^-18 and its kept product with a weight's second term 2^-27), so that the three bf16 terms are exactly
these pieces, at a density that keeps sum |x||w| of every output below 64 (128 for the sign-bit form, whose mask scale 2
doubles the operand): every kept product is then a multiple of 2^-18 (2^-17), every partial sum a 24-bit number, and the f64 sum of the six kept products round-trips through float32 - asserted on the
CPU for each case.  Fused, knob and that f64 evaluation must be the same numbers: a wrong lane, term or half is another one.
(b) random inputs: the criterion of tests/test_gpu_split.py (_compare: error against f64 relative to sum |x||w|, held
against the f32-MFMA chain's) for the fused launch.  How many outputs differ from the knob's is printed, not asserted:
two products are summed inside one instruction where the six-MFMA step rounds after each, so last bits may move; equality
with the unfused kernel's bits is not a contract.
Which kernel ran cannot be told from the numbers, so every launch is bracketed by rr_linear_split_tail_launches: the default
launch of an eligible shape counts one fused launch, the knob's and the controls' none.
Forms: "plain" is MODE 0 / EPI 0 (the persistent instantiation), "plain_res" MODE 0 with bias, residual, ReLU, dropout and
sign bits (EPI 1), "gathered" MODE 1 with a residual (EPI 1), "gathered_nores" MODE 1 without (EPI 0), "masked" MODE 3.
(c) side outputs: dz_out never passes through the MFMAs and must be the knob's bits on random inputs as well; the sign-bit
image, c_pre and the column-sum partials are functions of the accumulators, so they are held bit for bit on the exact
inputs (where the accumulators are) and, on random inputs, to the output they were taken from (bits == out > 0)."""
import os

import pytest
import torch

from reactranker_amd import functions as Fn
from reactranker_amd._lib import lib
from tests.test_gpu_gemm_dispatch import _decode_bits, _encode_bits, _n_cu, _pack_f32
from tests.test_gpu_split import _compare, _pack_split

pytestmark = pytest.mark.gpu
dev = "cuda"
KNOB = "RR_NO_TAIL_FUSE"
ASK = "RR_TAIL_FUSE"       # asks for the fused kernels whatever the library's default is
SENTINEL = 1e30          # operand padding: a kernel that multiplies one into a kept product fails at once
FILL = 7.5               # outputs start out as this
FULL = 43 * 192          # whole row blocks in front of the endings (the 12-wave geometry starts above 8192 rows)
ENDS = (16, 197, 389)
NS = (300, 304)
KS = [(12, 0), (44, 0), (48, 0), (76, 0), (300, 0)]
MODES = ("plain", "gathered", "masked")          # MODE 0, 1, 3 of the kernel
# (two segments, 61 | 300: the plain form - the sign-bit form has one segment, and so has the model's gathered form; the
# other epilogue instantiation of MODE 0 / 1 at an odd and an even number of k-steps)
FORMS = ([(mode, k1, k2) for mode in MODES for k1, k2 in KS] + [("plain", 61, 300)]
         + [(mode, k1, 0) for mode in ("plain_res", "gathered_nores") for k1 in (76, 300)])
CONTROL = {"plain": (49, 0), "plain_res": (49, 0), "gathered": (49, 0), "gathered_nores": (49, 0), "masked": (52, 0)}


def live(k1, k2):
    """live columns of the last k-step (split_tail_live in the source)"""
    k = k2 if k2 else k1
    return k - ((k + 31) // 32 - 1) * 32


def _exact(g, rows, cols, density):
    v = torch.randint(0, 24, (rows, cols), generator=g, dtype=torch.int32)      # a, b, c and the sign from one draw
    a, b, c, neg = v % 3 + 1, (v // 3) % 2, (v // 6) % 2, v // 12
    mag = a.float() + b.float() * 2.0 ** -9 + (b * c).float() * 2.0 ** -18      # (24 bits at the most: exact in f32)
    keep = torch.rand(rows, cols, generator=g) < density
    return torch.where(keep, torch.where(neg > 0, -mag, mag), torch.zeros(1))


def _small_ints(g, *shape):
    return torch.randint(-2, 3, shape, generator=g).float()


def _padded(values, pad=4):
    rows, cols = values.shape
    buf = torch.full((rows, (cols + 3) // 4 * 4 + pad), SENTINEL)
    buf[:, :cols] = values
    return buf


def make_case(mode, M, N, k1, k2, exact, seed):
    """CPU tensors of one launch: the arguments of Fn.linear (`kw`), the operand as the kernel forms it (`x`, [M, K] f32), the
    weight and what is added behind the GEMM"""
    g = torch.Generator().manual_seed(seed)
    K = k1 + k2
    dens = min(0.5, (0.3 / K) ** 0.5)
    if exact:
        draw = lambda r, c, d=dens: _exact(g, r, c, d)                       # noqa: E731
        W = draw(N, K)
    else:
        draw = lambda r, c, d=None: torch.randn(r, c, generator=g)           # noqa: E731
        W = draw(N, K) / K ** 0.5
    kw, add = dict(k1=k1), {}
    form, mode = mode, mode.split("_")[0]
    if mode == "plain":
        x1 = draw(M, k1)
        kw.update(a1=_padded(x1))
        x = x1
        if k2:
            x2 = draw(M, k2)
            kw.update(a2=_padded(x2), k2=k2)
            x = torch.cat([x1, x2], 1)
        if k2:                                              # the W_o form: bias, ReLU, dropout, sign bits
            add["bias"] = _small_ints(g, N) if exact else torch.randn(N, generator=g)
            kw.update(bias=add["bias"], act=Fn.ACT_RELU, drop_p=0.1, seed=seed * 7919 + 5)
        if form == "plain_res":                             # the model's forward layer on a materialised operand
            n3 = M // 2 + 5
            ridx = torch.randint(-1, n3, (M,), generator=g).to(torch.int32)
            add["bias"] = _small_ints(g, N) if exact else torch.randn(N, generator=g)
            res = _small_ints(g, n3, N) if exact else torch.randn(n3, N, generator=g)
            add["residual"] = torch.where(ridx[:, None] >= 0, res[ridx.clamp(min=0).long()], torch.zeros(1))
            kw.update(bias=add["bias"], residual=res, residual_idx=ridx, act=Fn.ACT_RELU, drop_p=0.1, seed=seed * 7919 + 5)
    elif mode == "gathered":                                # a1[idx] - sub[idx2], bias, residual[ridx], ReLU, dropout, sign bits
        n1, n2, n3 = M // 2 + 3, M // 3 + 2, M // 2 + 5
        a1, sub = draw(n1, k1), draw(n2, k1)
        if exact:                                           # disjoint columns: an element of the difference is one of the values, not
            a1[:, 1::2] = 0.0                               # a difference of two (3 + 2^-18 - 3 has ONE term, 2^-18, and its kept
            sub[:, 0::2] = 0.0                              # product with a weight's third term is 2^-36)
        idx = torch.randint(-1, n1, (M,), generator=g).to(torch.int32)
        idx2 = torch.randint(-1, n2, (M,), generator=g).to(torch.int32)
        ridx = torch.randint(-1, n3, (M,), generator=g).to(torch.int32)
        gat = lambda s, i: torch.where(i[:, None] >= 0, s[i.clamp(min=0).long()], torch.zeros(1))   # noqa: E731
        x = gat(a1, idx) - gat(sub, idx2)
        add["bias"] = _small_ints(g, N) if exact else torch.randn(N, generator=g)
        res = _small_ints(g, n3, N) if exact else torch.randn(n3, N, generator=g)
        kw.update(a1=_padded(a1), a1_idx=idx, a1_sub=_padded(sub), a1_sub_idx=idx2, bias=add["bias"], act=Fn.ACT_RELU, drop_p=0.1,
                  seed=seed * 7919 + 5)
        if form == "gathered":
            add["residual"] = gat(res, ridx)
            kw.update(residual=res, residual_idx=ridx)
    else:                                                   # dX: (dy * 2 where the sign bit is set) W, dZ and column sums
        dy = draw(M, k1)
        pos = torch.rand(M, k1, generator=g) < 0.6
        x = torch.where(pos, dy * 2.0, torch.zeros(1))
        kw.update(a1=_padded(dy), mask_scale=2.0)
        add["pos"] = pos
    cw = torch.rand(M, generator=g) if mode == "masked" or (form == "plain" and not k2) else None
    return dict(mode=mode, M=M, N=N, k1=k1, k2=k2, W=W, x=x, kw=kw, add=add, cw=cw)


def _terms(v):
    """the three bf16 terms of an f32 tensor, as split_pair and rr_pack_weights form them (round to nearest even)"""
    t0 = v.bfloat16().float()
    r = v - t0
    t1 = r.bfloat16().float()
    t2 = r - t1
    assert torch.equal(t2.bfloat16().float(), t2)
    return t0.double(), t1.double(), t2.double()


def six_products(x, W):
    """the six kept products per multiply, summed in f64 (any device), and sum |x||w|"""
    x0, x1, x2 = _terms(x)
    w0, w1, w2 = _terms(W)
    ref = x0 @ w0.t() + (x0 @ w1.t() + x1 @ w0.t()) + (x0 @ w2.t() + x1 @ w1.t() + x2 @ w0.t())
    return ref, x.double().abs() @ W.double().abs().t()


def assert_exact_range(ref, den, extra=0.0, lsb=2.0 ** -18):
    """(on the CPU) the f64 evaluation round-trips through float32, and so does every partial sum of it: multiples of `lsb`
    (2^-18; 2^-17 where the operand is doubled by the mask scale) below 2^24 lsb"""
    ref, den = ref.cpu(), den.cpu()
    assert torch.equal(ref.float().double(), ref)
    assert torch.equal(torch.round(ref / lsb) * lsb, ref)
    assert float(den.max()) + extra < 2.0 ** 24 * lsb, float(den.max())
    assert float(den.max()) > 0.0


def _to_dev(kw):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}


def _launch(case, w, kwd, cwd, bitsd):
    M, N, mode = case["M"], case["N"], case["mode"]
    bufs = {"out": torch.full((M, N), FILL, device=dev)}
    if mode == "masked":
        bufs["dz_out"] = torch.full((M, case["k1"] + 4), FILL, device=dev)
        kwd = dict(kwd, a_mask_bits=bitsd)
    elif "bias" in case["add"]:
        bufs["mask_bits_out"] = torch.full((M, int(lib().rr_mask_bits_row_bytes(N))), 0xA5, dtype=torch.uint8, device=dev)
        if "residual" in case["add"]:
            bufs["c_pre"] = torch.full((M, N), FILL, device=dev)
    res = Fn.linear(M, N, w, colsum_w=cwd, **kwd, **bufs)
    if cwd is not None:
        bufs["colsum_partial"] = res[1]
    torch.cuda.synchronize()
    return bufs


def run_both(case, w, extra_env=None):
    """the same launch with the default (fused where eligible) and with the knob"""
    assert os.environ.get(KNOB) is None and os.environ.get(ASK) is None
    kwd = _to_dev(case["kw"])
    cwd = case["cw"].to(dev) if case["cw"] is not None else None
    bitsd = _encode_bits(case["add"]["pos"].to(dev)) if case["mode"] == "masked" else None
    env = dict(extra_env or {}, **{ASK: 1})                 # (the knob wins over it)
    for k in env:
        os.environ[k] = "1"
    count = lib().rr_linear_split_tail_launches
    try:
        n0 = int(count())
        new = _launch(case, w, kwd, cwd, bitsd)
        n1 = int(count())
        os.environ[KNOB] = "1"
        old = _launch(case, w, kwd, cwd, bitsd)
        n2 = int(count())
    finally:
        for k in list(env) + [KNOB]:
            os.environ.pop(k, None)
    eligible = 1 <= live(case["k1"], case["k2"]) <= 16
    assert (n1 - n0, n2 - n1) == (1 if eligible else 0, 0), (case["mode"], case["k1"], case["k2"], n1 - n0, n2 - n1)
    return new, old


def _check_exact(case, extra_env=None):
    what = (case["mode"], case["M"], case["N"], case["k1"], case["k2"], extra_env)
    Wd, xd = case["W"].to(dev), case["x"].to(dev)
    ref, den = six_products(xd, Wd)
    add = case["add"]
    extra = 4.0 if "bias" in add else 0.0                   # |bias| + |residual| <= 4: the sums behind the GEMM stay exact too
    assert_exact_range(ref, den, extra, 2.0 ** -17 if case["mode"] == "masked" else 2.0 ** -18)
    w = _pack_split(Wd, 0, case["N"], 0, case["k1"], case["k2"])
    new, old = run_both(case, w, extra_env)
    for name in old:
        assert torch.equal(new[name], old[name]), (what, name)
    out = new["out"]
    if "bias" in add:                                       # what the epilogue adds is exact as well
        pre = ref + add["bias"].to(dev).double()
        if "residual" in add:
            pre = pre + add["residual"].to(dev).double()
            assert torch.equal(new["c_pre"].double(), pre), what
        keep_scale = 1.0 / (1.0 - torch.tensor(0.1, dtype=torch.float32))
        kept = torch.relu(pre.float()) * keep_scale.to(dev)
        assert bool(((out == 0) | (out == kept)).all()), what
        assert 0.85 < float((out[kept > 0] != 0).float().mean()) < 0.95, what
        assert torch.equal(_decode_bits(new["mask_bits_out"], case["N"]), out > 0), what
    else:
        assert torch.equal(out.double(), ref), what
    if case["mode"] == "masked":
        assert torch.equal(new["dz_out"][:, :case["k1"]], xd), what
        assert bool((new["dz_out"][:, case["k1"]:] == FILL).all()), what


@pytest.mark.parametrize("mode,k1,k2", FORMS)
def test_fused_tail_knob_and_f64_agree_on_exact_inputs(mode, k1, k2):
    assert 1 <= live(k1, k2) <= 16
    for i, N in enumerate(NS):
        for j, end in enumerate(ENDS):
            _check_exact(make_case(mode, FULL + end, N, k1, k2, True, 1000 * k1 + 10 * i + j))


@pytest.mark.parametrize("mode,k1,k2,no_persist", [("plain", 300, 0, False), ("plain", 300, 0, True), ("plain", 61, 300, False),
                                                    ("plain", 61, 300, True), ("gathered", 300, 0, False), ("masked", 300, 0, False),
                                                    ("plain_res", 300, 0, False), ("gathered_nores", 300, 0, False)])
def test_fused_tail_with_waves_without_rows_on_exact_inputs(mode, k1, k2, no_persist):
    """more row blocks than CUs: the persistent form (its wrap into the next block included) and the balanced last round,
    whose short blocks have waves without rows; the plain forms once more as one block per workgroup"""
    M = 192 * _n_cu() + 197
    _check_exact(make_case(mode, M, 300, k1, k2, True, 77 + k1), {"RR_NO_PERSIST": 1} if no_persist else None)


def _check_random(case, eligible):
    what = f"{case['mode']} M {case['M']} N {case['N']} K {case['k1']}|{case['k2']}"
    Wd, xd = case["W"].to(dev), case["x"].to(dev)
    ref, den = xd.double() @ Wd.double().t(), xd.double().abs() @ Wd.double().abs().t() + 1e-300
    add = case["add"]
    if "bias" in add:
        ref, den = ref + add["bias"].to(dev).double(), den + add["bias"].to(dev).double().abs()
    if "residual" in add:
        ref, den = ref + add["residual"].to(dev).double(), den + add["residual"].to(dev).double().abs()
    new, old = run_both(case, _pack_split(Wd, 0, case["N"], 0, case["k1"], case["k2"]))
    differ = int((new["out"] != old["out"]).sum())
    print(f"[tail fuse] {what}: {differ} of {new['out'].numel()} outputs differ from the knob's")
    if not eligible:                                        # the control: the six-MFMA step, the knob's launch
        for name in old:
            assert torch.equal(new[name], old[name]), (what, name)
        return
    if "dz_out" in new:                                     # never passes through the MFMAs
        assert torch.equal(new["dz_out"], old["dz_out"]), what
        assert torch.equal(new["dz_out"][:, :case["k1"]], xd), what
    if "mask_bits_out" in new:
        assert torch.equal(_decode_bits(new["mask_bits_out"], case["N"]), new["out"] > 0), what
    # the criterion of tests/test_gpu_split.py: the pre-activation GEMM (no ReLU / dropout in front of the comparison) against
    # the f32-MFMA chain on the same operands
    plain_kw = {k: v for k, v in case["kw"].items() if k not in ("act", "drop_p", "seed")}
    kwd = _to_dev(plain_kw)
    if case["mode"] == "masked":
        kwd["a_mask_bits"] = _encode_bits(add["pos"].to(dev))
    osp = Fn.linear(case["M"], case["N"], _pack_split(Wd, 0, case["N"], 0, case["k1"], case["k2"]), **kwd)
    if case["mode"] == "masked":                            # the f32 kernels read the mask as floats
        del kwd["a_mask_bits"]
        kwd["a_mask"] = torch.where(add["pos"], 1.0, -1.0).to(dev)
    o32 = Fn.linear(case["M"], case["N"], _pack_f32(Wd, case["N"], case["k1"], case["k2"]), w_packed=True, **kwd)
    _compare(o32, osp, ref, den, "fused tail, " + what)


@pytest.mark.parametrize("mode,k1,k2", FORMS)
def test_fused_tail_error_is_not_above_the_f32_mfma_chain(mode, k1, k2):
    for i, N in enumerate(NS):
        for j, end in enumerate(ENDS):
            _check_random(make_case(mode, FULL + end, N, k1, k2, False, 500 * k1 + 10 * i + j), True)


@pytest.mark.parametrize("mode", sorted(CONTROL))
def test_a_tail_of_more_than_16_columns_takes_the_six_mfma_step(mode):
    k1, k2 = CONTROL[mode]
    assert live(k1, k2) > 16
    for i, N in enumerate(NS):
        _check_random(make_case(mode, FULL + ENDS[1], N, k1, k2, False, 31 + i), False)


def test_live_columns_of_the_shapes():
    assert [live(*k) for k in KS + [(61, 300)]] == [12, 12, 16, 12, 12, 12]
    assert live(49, 0) == 17 and live(52, 0) == 20 and live(83, 0) == 19 and live(600, 0) == 24 and live(300, 22) == 22
