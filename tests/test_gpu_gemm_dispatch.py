"""Every launch path of the split GEMMs against f64: each linear_split_kernel instantiation rr_linear_f32 can reach with
w_packed = 2 (tests/gemm_dispatch_table.py: LINEAR_LEAVES, the persistent form included), the K > 992 and masked legs of
w_packed = 3, every wgrad_split_kernel<MASK, SUB, WTK, false> and the scalar fallback of rr_linear_wgrad_f32, the row-dot
kernel's edges, and the argument-level refusals of the split path.

The three-bf16-term form is held to the yardstick of tests/test_gpu_split.py: on the same inputs, its error relative to
sum |a||w| is at most 2x the f32-MFMA chain's maximum and 1.25x its mean, and at most 2e-6 (the f32 chain meets that bound up
to K = 683: where a segment is wider than 992 columns the bound is scaled by K / 683, nowhere else).  This module is in none
of tests/conftest.py's arithmetic sets: every test builds its weight images itself and restores any functions.* flag it sets."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dropout_ref
from reactranker_amd import _lib
from reactranker_amd import functions as Fn
from reactranker_amd._lib import PackDesc, check, lib, ptr, stream
from tests import gemm_dispatch_table as T
from tests import helpers as Hh
from tests.test_gpu_f16x2 import _pack as _pack_terms
from tests.test_gpu_split import _compare, _err, _pack_split

pytestmark = pytest.mark.gpu
dev = "cuda"

N_EDGES = {(4, 4, 8): [4, 16, 60, 64], (10, 10, 8): [68, 128, 160], (19, 5, 8): [164, 300, 304], (19, 19, 12): [164, 300, 304],
           (38, 19, 12): [308, 600, 608]}
K_LEAN = [1, 31, 32, 33, 133, 300, 992]
K_WIDE = [993, 1024, 1025]
M_EDGES = [1, 15, 16, 17, 191, 192, 193, 8192, 8193]
SENTINEL = 1e30          # padding columns of operands: a kernel that multiplies one into a kept product fails at once
OUT_PAD = 7.5            # padding columns of outputs: must come back untouched


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bound(k1, k2):
    """2e-6 of sum |a||w|; scaled by K / 683 for the generic-loader shapes (a segment wider than 992 columns)"""
    return 2e-6 * max(1.0, (k1 + k2) / 683) if not T.lean(k1, k2) else 2e-6


def _padded(rows, cols, pad, fill=SENTINEL, scale=1.0):
    buf = torch.full((rows, cols + pad), fill, device=dev)
    buf[:, :cols] = torch.randn(rows, cols, device=dev) * scale
    return buf


def _out(rows, cols, pad):
    return torch.full((rows, cols + pad), OUT_PAD, device=dev)


def _pack_f32(w, rows, k1, k2):
    """the zero-padded f32 layout of rr_pack_weight_f32 (w_packed = 1: the f32-MFMA yardstick)"""
    dst = torch.empty(rows, int(lib().rr_packed_weight_ld(k1, k2)), dtype=torch.float32, device=dev)
    d = (PackDesc * 1)()
    d[0].src, d[0].ld_src, d[0].transpose, d[0].rows, d[0].c0, d[0].k1, d[0].k2 = ptr(w), w.stride(0), 0, rows, 0, k1, k2
    d[0].dst, d[0].split = ptr(dst), 0
    check(lib().rr_pack_weights_f32(d, 1, stream()), "rr_pack_weights_f32")
    return dst


def _bit_slots(n):
    """byte and bit of every column in a sign-bit row (include/reactranker_hip.h, rr_linear_args.mask_bits_out)"""
    c = torch.arange(n, device=dev)
    return (c // 304) * 40 + ((c % 304) % 16) // 8 * 20 + (c % 304) // 16, c % 8


def _decode_bits(bits, n):
    byte, bit = _bit_slots(n)
    return ((bits[:, byte].int() >> bit) & 1).bool()


def _encode_bits(pos):
    M, n = pos.shape
    byte, bit = _bit_slots(n)
    out = torch.zeros(M, int(lib().rr_mask_bits_row_bytes(n)), dtype=torch.int64, device=dev)
    out.index_add_(1, byte, pos.long() << bit)
    return out.to(torch.uint8)


def _gather(src, idx, cols):
    return torch.where(idx[:, None] >= 0, src[idx.clamp(min=0).long(), :cols], torch.zeros(1, device=dev))


def _indices(M, n_src, rng):
    idx = torch.as_tensor(rng.integers(-1, n_src, M), dtype=torch.int32, device=dev)
    idx[0] = -1
    return idx


# ---------------------------------------------------------------------------------------------- the w_packed = 2 sweep
def _draw(leaf, rng, n_cu, alt_wide):
    """a random case of rr_linear_f32 that leaf_of sends to `leaf` (rejection sampling over the edge values)"""
    ntp, nt, mode, waves, epi, persistent = leaf
    for _ in range(10000):
        N = int(rng.choice(N_EDGES[(ntp, nt, waves)]))
        if persistent:
            M = int(rng.integers(192 * n_cu + 1, 192 * n_cu + 10000))
        elif waves == 12:
            M = int(rng.choice([8193, int(rng.integers(8194, 30000))]))
        elif (ntp, nt) == (19, 5):
            M = int(rng.choice(M_EDGES[:-1] + [int(rng.integers(194, 8192))]))
        else:
            M = int(rng.choice(M_EDGES + [int(rng.integers(8194, 20000))]))
        wide = epi >= 2 if waves == 12 and mode in (0, 1) else alt_wide

        def k(w):
            return int(rng.choice(K_WIDE + [int(rng.integers(993, 1500))])) if w else int(rng.choice(K_LEAN))
        if mode in (2, 3):
            k1, k2 = k(wide), 0
            if mode == 3 or rng.integers(2):          # (the sign-bit mask and the dZ side output need k1 % 4 == 0)
                k1 = (k1 + 3) // 4 * 4
        elif wide and rng.integers(2):
            k1, k2 = k(False), k(True)
        else:
            k1, k2 = k(wide), int(rng.choice([0, k(False)]))
        residual = bool(rng.integers(2)) if not (waves == 12 and mode in (0, 1)) else epi % 2 == 1
        if T.leaf_of(M, N, k1, k2, mode, residual, n_cu) == leaf:
            return dict(M=M, N=N, k1=k1, k2=k2, mode=mode, residual=residual)
    raise AssertionError(f"no case drawn for {leaf}")


def _cases(n_cu):
    rng = np.random.default_rng(20261016)
    cases = []
    for leaf in T.LINEAR_LEAVES:
        for i in range(2):                             # (where the leaf leaves K free: one case K <= 992, one K > 992)
            cases.append(_draw(leaf, rng, n_cu, alt_wide=i == 1))
    # the one-block form of the persistent shape: more row blocks than CUs, an odd number of k-steps
    cases.append(dict(M=192 * n_cu + 4321, N=300, k1=257, k2=0, mode=0, residual=False))
    assert T.leaf_of(192 * n_cu + 4321, 300, 257, 0, 0, False, n_cu) == (19, 19, 0, 12, 0, False)
    for c in cases:
        c["opts"] = dict(gather=c["mode"] in (0, 1) and bool(rng.integers(2)), sub_idx=bool(rng.integers(2)),
                         bias=bool(rng.integers(2)), ridx=c["residual"] and bool(rng.integers(2)), relu=bool(rng.integers(2)),
                         drop=rng.random() < 0.3 and c["M"] * c["N"] <= 4e6, cpre=rng.random() < 0.3, colsum=rng.random() < 0.4,
                         bits=rng.random() < 0.4,
                         pads=[int(p) for p in rng.choice([0, 4, 12], 6)],
                         seed=int(rng.integers(1, 2 ** 62)))
    return cases


def _run_case(c, reached):
    """one case: the split GEMM, the f32-MFMA yardstick on the same inputs, f64; returns (label, split err, f32 err)"""
    M, N, k1, k2, mode, o = c["M"], c["N"], c["k1"], c["k2"], c["mode"], c["opts"]
    K = k1 + k2
    pa, ps, p2, pr, pc, pm = o["pads"]
    rng = np.random.default_rng(o["seed"])
    torch.manual_seed(o["seed"] & 0xFFFFFFFF)
    W = torch.randn(N, K, device=dev) / K ** 0.5
    z = torch.zeros(1, device=dev)
    kw = dict(k1=k1, mask_scale=1.25)
    n_src = M // 2 + 3 if o["gather"] else M
    a1 = _padded(n_src, k1, (-k1) % 4 + pa)              # (leading dimensions: multiples of 4, as the split path needs)
    kw["a1"] = a1
    A1 = a1[:, :k1]
    if o["gather"]:
        kw["a1_idx"] = _indices(M, n_src, rng)
        A1 = _gather(a1, kw["a1_idx"], k1)
    if mode == 1:
        n_sub = M // 3 + 2 if o["sub_idx"] else M
        sub = _padded(n_sub, k1, (-k1) % 4 + ps)
        kw["a1_sub"] = sub
        if o["sub_idx"]:
            kw["a1_sub_idx"] = _indices(M, n_sub, rng)
            A1 = A1 - _gather(sub, kw["a1_sub_idx"], k1)
        else:
            A1 = A1 - sub[:, :k1]
    y = bits = None
    if mode in (2, 3):
        y = _padded(M, k1, (-k1) % 4 + pm)
        A1 = torch.where(y[:, :k1] > 0, a1[:, :k1] * torch.tensor(1.25, device=dev), z)   # (f32 product, as the kernel forms it)
        if mode == 3:
            bits = _encode_bits(y[:, :k1] > 0)
    X = A1
    if k2:
        a2 = _padded(M, k2, (-k2) % 4 + p2)
        kw.update(a2=a2, k2=k2)
        X = torch.cat([A1, a2[:, :k2]], 1)
    ref = X.double() @ W.double().t()
    den = X.double().abs() @ W.double().abs().t()
    if o["bias"]:
        b = torch.randn(N, device=dev)
        kw["bias"] = b
        ref, den = ref + b.double(), den + b.double().abs()
    if c["residual"]:
        n_res = M // 2 + 3 if o["ridx"] else M
        R = _padded(n_res, N, pr)
        kw["residual"] = R
        Rr = R[:, :N]
        if o["ridx"]:
            kw["residual_idx"] = _indices(M, n_res, rng)
            Rr = _gather(R, kw["residual_idx"], N)
        ref, den = ref + Rr.double(), den + Rr.double().abs()
    pre, den_pre = ref, den
    if o["relu"]:
        kw["act"] = Fn.ACT_RELU
        ref = torch.relu(ref)
    keep = None
    if o["drop"]:
        p, seed = 0.2, o["seed"]
        kw.update(drop_p=p, seed=seed)
        keep = torch.from_numpy(dropout_ref.keep_mask(seed & 0xFFFFFFFFFFFFFFFF, np.arange(M * N, dtype=np.uint64), p).reshape(M, N)).to(dev)
        ks = float(np.float32(1) / (np.float32(1) - np.float32(p)))
        ref = torch.where(keep, ref * ks, torch.zeros_like(ref))
        den = den * ks
    den = den + 1e-300

    # f32-MFMA yardstick (w_packed = 1; a sign-bit mask is read as the f32 activation it encodes)
    kw32 = dict(kw)
    if mode in (2, 3):
        kw32["a_mask"] = y
    o32 = Fn.linear(M, N, _pack_f32(W, N, k1, k2), w_packed=True, **kw32)

    # the split GEMM with every side output the ABI allows here
    ksp = dict(kw)
    wsp = _pack_split(W, 0, N, 0, k1, k2)
    out = _out(M, N, pc)
    ksp["out"] = out[:, :N]
    cpre = dz = bits_out = None
    if o["cpre"]:
        cpre = _out(M, N, pc)
        ksp["c_pre"] = cpre[:, :N]
    if mode in (2, 3) and k1 % 4 == 0:
        dz = _out(M, k1, pm)
        ksp["dz_out"] = dz[:, :k1]
    if o["bits"]:
        bits_out = torch.full((M, int(lib().rr_mask_bits_row_bytes(N))), 0xA5, dtype=torch.uint8, device=dev)
        ksp["mask_bits_out"] = bits_out
    cw = torch.rand(M, device=dev) if o["colsum"] else None
    if mode == 2:
        ksp["a_mask"] = y
    if mode == 3:
        ksp["a_mask_bits"] = bits
    res = Fn.linear(M, N, wsp, colsum_w=cw, **ksp)
    osp, part = res if cw is not None else (res, None)
    leaf = T.leaf_of(M, N, k1, k2, mode, c["residual"], _n_cu())
    reached.add(leaf)
    label = (f"{T.leaf_name(leaf)} M {M} N {N} K {k1}+{k2} " +
             " ".join(k for k in ("gather", "sub_idx", "bias", "ridx", "relu", "drop", "cpre", "colsum", "bits") if o[k] and
                      (k != "sub_idx" or mode == 1) and (k != "ridx" or c["residual"])))
    bound = _bound(k1, k2)
    esp, e32 = _compare(o32, osp, ref, den, label, north_star=True, bound=bound)

    assert torch.all(out[:, N:] == OUT_PAD), label + ": wrote past N"
    if cpre is not None:                               # the pre-activation output, and the stored output is its epilogue
        assert torch.all(cpre[:, N:] == OUT_PAD)
        e_pre, _ = _err(cpre[:, :N], pre, den_pre + 1e-300)
        Hh.record(label + " | c_pre", e_pre, bound)
        assert e_pre <= bound, (label, e_pre)
        fin = torch.relu(cpre[:, :N]) if o["relu"] else cpre[:, :N]
        if keep is not None:
            fin = torch.where(keep, fin * torch.tensor(ks, device=dev), torch.zeros_like(fin))
        assert torch.equal(fin, osp), label + ": c_pre and c disagree"
    if dz is not None:                                 # the masked operand, exactly
        assert torch.equal(dz[:, :k1], A1) and torch.all(dz[:, k1:] == OUT_PAD), label + ": dz_out"
    if bits_out is not None:                           # the sign of what was stored, in the documented layout
        assert torch.equal(_decode_bits(bits_out, N), osp > 0), label + ": mask_bits_out"
    if part is not None:                               # 64-row partials: a sum of depth < 16 each, against f64
        cs = (osp.double() * cw.double()[:, None]).sum(0)
        csd = (osp.double().abs() * cw.double()[:, None]).sum(0) + 1e-300
        e_cs = float(((part[:, :N].double().sum(0) - cs).abs() / csd).max())
        Hh.record(label + " | column sums", e_cs, 2.0 ** -20)
        assert part.shape[0] == int(lib().rr_linear_colsum_rows(M)) and e_cs <= 2.0 ** -20, (label, e_cs)
    if mode == 3:                                      # the sign bits are the f32 mask: MODE 2 must give the same bits
        k2sp = dict(ksp)
        del k2sp["a_mask_bits"]
        k2sp["a_mask"] = y
        out2 = _out(M, N, pc)
        k2sp["out"] = out2[:, :N]
        if dz is not None:
            dz2 = _out(M, k1, pm)
            k2sp["dz_out"] = dz2[:, :k1]
        if cpre is not None:
            k2sp["c_pre"] = _out(M, N, pc)[:, :N]
        if bits_out is not None:
            k2sp["mask_bits_out"] = torch.empty_like(bits_out)
        res2 = Fn.linear(M, N, wsp, colsum_w=cw, **k2sp)
        reached.add(T.leaf_of(M, N, k1, k2, 2, c["residual"], _n_cu()))
        o2, part2 = res2 if cw is not None else (res2, None)
        assert torch.equal(o2, osp), label + ": MODE 3 differs from MODE 2"
        if dz is not None:
            assert torch.equal(dz2, dz)
        if part is not None:
            assert torch.equal(part2, part)
    return leaf, esp, e32, bound


def test_split_gemm_every_leaf_against_f64(parity_log):
    """every (NTP, NT, MODE, WAVES, EPI, persistent) of the w_packed = 2 dispatcher, two or more random shapes each (N, K, M at
    the bucket / k-step / row-block edges, padded leading dimensions everywhere, gathered rows with -1 entries, subtrahends,
    residual rows by index, bias / ReLU / dropout, c_pre, column sums, sign bits, dZ side output, MODE 3 = MODE 2)"""
    n_cu = _n_cu()
    reached, worst = set(), {}
    for c in _cases(n_cu):
        leaf, esp, e32, bound = _run_case(c, reached)
        w = worst.get(leaf, (0.0, 0.0, 0, bound))
        worst[leaf] = (max(w[0], esp), max(w[1], e32), w[2] + 1, max(w[3], bound))
    for leaf in sorted(worst):
        e, e32, n, bound = worst[leaf]
        parity_log(f"linear_split_kernel{T.leaf_name(leaf)}: {n} shapes, worst max err / sum|a||w| {e:.2e} (f32-MFMA chain {e32:.2e}, "
                   f"bound {bound:.2e})")
    assert reached == set(T.LINEAR_LEAVES), sorted(set(T.LINEAR_LEAVES) ^ reached)


def test_mode3_reads_the_bits_a_forward_gemm_wrote():
    """MODE 3 fed the sign bits that the producing forward GEMM stored (mask_bits_out), MODE 2 fed its f32 output: same bits
    of output, dZ and column sums - in every geometry"""
    torch.manual_seed(11)
    reached = set()
    for N, M, k1 in ((64, 777, 300), (160, 193, 132), (300, 4001, 600), (300, 9001, 64), (600, 8193, 300)):
        xf = torch.randn(M, 40, device=dev)
        Wf = torch.randn(k1, 40, device=dev) / 7
        bits = torch.zeros(M, int(lib().rr_mask_bits_row_bytes(k1)), dtype=torch.uint8, device=dev)
        y = Fn.linear(M, k1, _pack_split(Wf, 0, k1, 0, 40, 0), a1=xf, k1=40, act=Fn.ACT_RELU, drop_p=0.1, seed=5, mask_bits_out=bits)
        assert torch.equal(bits, _encode_bits(y > 0))
        W = torch.randn(N, k1, device=dev) / k1 ** 0.5
        dy = torch.randn(M, k1, device=dev)
        cw = torch.rand(M, device=dev)
        wsp = _pack_split(W, 0, N, 0, k1, 0)
        dz2, dz3 = torch.empty(M, k1, device=dev), torch.empty(M, k1, device=dev)
        o2, p2 = Fn.linear(M, N, wsp, a1=dy, k1=k1, a_mask=y, mask_scale=1 / 0.9, dz_out=dz2, colsum_w=cw)
        o3, p3 = Fn.linear(M, N, wsp, a1=dy, k1=k1, a_mask_bits=bits, mask_scale=1 / 0.9, dz_out=dz3, colsum_w=cw)
        assert torch.equal(o2, o3) and torch.equal(dz2, dz3) and torch.equal(p2, p3), (N, M, k1)
        reached |= {T.leaf_of(M, N, k1, 0, m, False, _n_cu()) for m in (2, 3)}
    assert {(l[0], l[1], l[3]) for l in reached} == set(T.GEOMETRIES)


# ---------------------------------------------------------------------------------------------- row independence
@pytest.mark.parametrize("N", [300, 600])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("residual", [False, True])
def test_a_row_does_not_depend_on_its_batch(N, mode, residual, monkeypatch):
    """rows [0, M0) computed alone (N = 300: <19,5,8>), inside M0 + 9000 rows (<19,19,12>) and, for plain operands without a
    residual, inside more than 192 x CUs rows (the persistent form; also against its one-block form) are the same bits
    (rr_linear_f32: "same weight image, same k order"; functions.SplitGemm: a query's scores do not depend on its batch)"""
    torch.manual_seed(N + 10 * mode + residual)
    rng = np.random.default_rng(N + mode)
    n_cu = _n_cu()
    M0, K = 3001, 300
    persistent = N == 300 and mode == 0 and not residual
    sizes = [M0, M0 + 9000] + ([192 * n_cu + 777] if persistent else [])
    Mb = max(sizes)
    W = torch.randn(N, K, device=dev) / K ** 0.5
    wsp = _pack_split(W, 0, N, 0, K, 0)
    b = torch.randn(N, device=dev)
    a1 = torch.randn(Mb // 2 + 3 if mode == 1 else Mb, K, device=dev)
    sub = torch.randn(Mb, K, device=dev)
    idx, sidx = _indices(Mb, a1.shape[0], rng), _indices(Mb, Mb, rng)
    y = torch.randn(Mb, K, device=dev)
    bits = _encode_bits(y > 0)
    R = torch.randn(Mb, N, device=dev)

    def run(M):
        kw = dict(k1=K, bias=b, mask_scale=1.25)
        if residual:
            kw["residual"] = R[:M]
        if mode == 0:
            kw.update(a1=a1[:M], act=Fn.ACT_RELU)
        elif mode == 1:
            kw.update(a1=a1, a1_idx=idx[:M], a1_sub=sub, a1_sub_idx=sidx[:M], act=Fn.ACT_RELU)
        else:
            dz = torch.empty(M, K, device=dev)
            kw.update(a1=a1[:M], dz_out=dz)
            if mode == 2:
                kw["a_mask"] = y[:M]
            else:
                kw["a_mask_bits"] = bits[:M]
        out = Fn.linear(M, N, wsp, **kw)
        return out[:M0], (kw["dz_out"][:M0] if mode >= 2 else None)

    ref, ref_dz = run(M0)
    leaves = {T.leaf_of(M0, N, K, 0, mode, residual, n_cu)}
    for M in sizes[1:]:
        got, got_dz = run(M)
        leaves.add(T.leaf_of(M, N, K, 0, mode, residual, n_cu))
        assert torch.equal(got, ref), (M, T.leaf_of(M, N, K, 0, mode, residual, n_cu))
        if ref_dz is not None:
            assert torch.equal(got_dz, ref_dz)
    if persistent:
        assert T.leaf_of(Mb, N, K, 0, 0, False, n_cu)[5]
        got = run(Mb)[0]
        monkeypatch.setenv("RR_NO_PERSIST", "1")           # (an A/B knob of the library: the one-block launch of the same shape)
        assert torch.equal(run(Mb)[0], got)
    assert len(leaves) == (1 if N == 600 else len(sizes))


# ---------------------------------------------------------------------------------------------- w_packed = 3 legs
def test_f16x2_wide_and_masked_legs_against_f64(parity_log):
    """what tests/test_gpu_f16x2.py's sweep does not reach: segments wider than 992 columns (EPI 2 / 3 of the 12-wave
    geometries, the select-per-element loader of the 8-wave ones) and the masked MODE 2 / 3 forms, in every geometry"""
    rng = np.random.default_rng(4242)
    n_cu = _n_cu()
    reached, worst = set(), 0.0
    for (ntp, nt, waves), Ns in N_EDGES.items():
        M = 9001 if waves == 12 else int(rng.choice([17, 193, 4001]))
        for mode, residual, wide in ((0, False, True), (0, True, True), (1, False, True), (1, True, True),
                                     (2, False, False), (2, True, True), (3, False, True), (3, True, False)):
            N = int(rng.choice(Ns))
            if mode in (2, 3):
                k1 = int(rng.choice([996, 1024, 1028, 1300])) if wide else int(rng.choice([4, 32, 300, 992]))
                k2 = 0
            else:
                k1 = int(rng.choice([993, 1025, int(rng.integers(993, 1500))]))
                k2 = int(rng.choice([0, 83]))
                if rng.integers(2):
                    k1, k2 = k2 or 300, k1
            K = k1 + k2
            torch.manual_seed(int(rng.integers(1 << 30)))
            W = torch.randn(N, K, device=dev) / K ** 0.5
            x1 = torch.randn(M, (k1 + 3) // 4 * 4, device=dev) * torch.exp(torch.randn(M, 1, device=dev))
            kw = dict(a1=x1, k1=k1, bias=torch.randn(N, device=dev))
            A1 = x1[:, :k1]
            if mode == 1:
                sub = torch.randn(M, (k1 + 3) // 4 * 4, device=dev)
                sidx = _indices(M, M, rng)
                kw.update(a1_sub=sub, a1_sub_idx=sidx)
                A1 = A1 - _gather(sub, sidx, k1)
            y = None
            if mode in (2, 3):
                y = torch.randn(M, k1, device=dev)
                A1 = torch.where(y > 0, A1 * torch.tensor(1.25, device=dev), torch.zeros(1, device=dev))
                kw["mask_scale"] = 1.25
                if mode == 2:
                    kw["a_mask"] = y
                else:
                    kw["a_mask_bits"] = _encode_bits(y > 0)
            X = A1
            if k2:
                x2 = torch.randn(M, (k2 + 3) // 4 * 4, device=dev) * 0.5
                kw.update(a2=x2, k2=k2)
                X = torch.cat([A1, x2[:, :k2]], 1)
            ref = X.double() @ W.double().t() + kw["bias"].double()
            den = X.double().abs() @ W.double().abs().t() + kw["bias"].double().abs()
            if residual:
                R = torch.randn(M, N, device=dev)
                kw["residual"] = R
                ref, den = ref + R.double(), den + R.double().abs()
            wh = _pack_terms(W, 0, N, 0, k1, k2, 2)
            dz = torch.empty(M, k1, device=dev) if mode in (2, 3) else None
            out = Fn.linear(M, N, wh, dz_out=dz, **kw)
            # (test_gpu_f16x2.py's contract term: 2^-40 of the operand tensor's largest magnitude per product)
            den = den + 2.0 ** -36 * float(X.abs().max()) * W.double().abs().sum(1)[None, :] * 1e6
            e = float(((out.double() - ref).abs() / (den + 1e-300)).max())
            leaf = T.leaf_of(M, N, k1, k2, mode, residual, n_cu)
            reached.add(leaf + (T.lean(k1, k2),))
            Hh.record(f"f16x2 {T.leaf_name(leaf)} M {M} N {N} K {k1}+{k2}", e, 2e-6)
            worst = max(worst, e)
            assert e <= 2e-6, (leaf, M, N, k1, k2, e)
            if mode in (2, 3):
                assert torch.equal(dz, A1)
            if mode == 3:                              # same bound, same values: the bits equal the f32 mask
                kw2 = dict(kw)
                del kw2["a_mask_bits"]
                dz2 = torch.empty(M, k1, device=dev)
                assert torch.equal(Fn.linear(M, N, wh, a_mask=y, dz_out=dz2, **kw2), out) and torch.equal(dz2, dz)
    want = {l + (False,) for l in T.LINEAR_LEAVES if l[4] >= 2}                   # EPI 2 / 3
    want |= {(g[0], g[1], m, 8, 0, False, False) for g in T.GEOMETRIES if g[2] == 8 for m in (0, 1)}   # 8-wave, K > 992
    want |= {(g[0], g[1], m, g[2], 0, False, w) for g in T.GEOMETRIES for m in (2, 3) for w in (False, True)}
    assert want <= reached, sorted(want - reached)
    parity_log(f"w_packed = 3, {len(reached)} (leaf, loader) pairs (K > 992 and masked forms): worst max err {worst:.2e} (bound 2e-06)")


# ---------------------------------------------------------------------------------------------- weight gradient, split = 1
def _wgrad_raw(M, N, dy, dw, x1, k1, split, dbias=None):
    nbytes = int(lib().rr_linear_wgrad_workspace_bytes(M, N, k1))
    ws = torch.empty(max(1, nbytes // 4), device=dev)
    A = _lib.WgradArgs()
    A.M, A.N = M, N
    A.dy, A.ld_dy = ptr(dy), dy.stride(0)
    A.x1, A.ldx1, A.k1 = ptr(x1), x1.stride(0), k1
    A.dw, A.ld_dw, A.dbias = ptr(dw), dw.stride(0), ptr(dbias)
    A.workspace, A.workspace_bytes = ptr(ws), nbytes
    A.split = split
    check(lib().rr_linear_wgrad_f32(C.byref(A), stream()), "rr_linear_wgrad_f32")


def test_wgrad_split_every_instantiation_against_f64(parity_log):
    """all 12 wgrad_split_kernel<MASK, SUB, WTK, false>, two or more random shapes each (N 4 .. 608, M around multiples of 32
    and the chunk planner's switch points, gathered / subtracted X with -1 indices, ld_dw > K, dbias given or not): error
    against f64 as test_gpu_split.py bounds it, accumulate == dw + dw exactly; then the same K split [k1 | k2] in random
    places with exactly rr_linear_wgrad_workspace_bytes(M, N, K) bytes; then the scalar kernel a split request falls back to"""
    rng = np.random.default_rng(5150)
    old = (Fn.SPLIT_MIN_ROWS, Fn.SplitGemm.enabled, Fn.SplitGemm.f16)
    Fn.SPLIT_MIN_ROWS, Fn.SplitGemm.f16 = 1, False
    count = {k: 0 for k in T.WGRAD_SPLIT}
    worst = {}
    try:
        cases = []
        for _ in range(20000):
            if min(count.values()) >= 2:
                break
            k1 = int(rng.choice([1, 31, 32, 33, 61, 91, 95, 127, 133, 159, 191, 255, 300, 319, 600, int(rng.integers(1, 700))]))
            k2 = int(rng.choice([0, 0, 1, 83, 133, 300]))
            key = (bool(rng.integers(2)), bool(rng.integers(2)), T.wgrad_wtk(k1, k2))
            if count[key] >= 2:
                continue
            count[key] += 1
            N = int(rng.choice([4, 16, 60, 64, 68, 128, 160, 164, 300, 304, 308, 600, 608]))
            M = int(rng.choice([31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, int(rng.integers(9000, 40000))]))
            cases.append((key, M, N, k1, k2, bool(rng.integers(2)), bool(rng.integers(2)), int(rng.integers(1 << 30))))
        assert min(count.values()) >= 2
        for (mask, sub, wtk), M, N, k1, k2, gather, with_db, seed in cases:
            torch.manual_seed(seed)
            K = k1 + k2
            pad = lambda: int(rng.choice([0, 4, 8]))  # noqa: E731
            dz = _padded(M, N, pad(), fill=100.0)
            n_src = M // 2 + 3 if gather else M
            x1 = _padded(n_src, k1, (-k1) % 4 + pad(), fill=100.0)
            kw = dict(x1=x1, k1=k1)
            X1 = x1[:, :k1]
            if gather:
                kw["x1_idx"] = _indices(M, n_src, rng)
                X1 = _gather(x1, kw["x1_idx"], k1)
            if sub:
                n_sub = M // 3 + 2
                xs = _padded(n_sub, k1, (-k1) % 4 + pad(), fill=100.0)
                kw.update(x1_sub=xs, x1_sub_idx=_indices(M, n_sub, rng))
                X1 = X1 - _gather(xs, kw["x1_sub_idx"], k1)
            X = X1
            if k2:
                x2 = _padded(M, k2, (-k2) % 4 + pad(), fill=100.0)
                kw.update(x2=x2, k2=k2)
                X = torch.cat([X1, x2[:, :k2]], 1)
            dzr = dz[:, :N]
            if mask:
                y = _padded(M, N, pad(), fill=-1.0)
                kw.update(mask=y, mask_scale=1.25)
                dzr = torch.where(y[:, :N] > 0, dzr * torch.tensor(1.25, device=dev), torch.zeros(1, device=dev))
            got = {}
            for split in (False, True):
                Fn.SplitGemm.enabled = split
                dwb = _out(N, K, 4)
                db = torch.full((N,), OUT_PAD, device=dev) if with_db else None
                Fn.wgrad(M, N, dz, dwb[:, :K], dbias=db, **kw)
                dwb2, db2 = dwb.clone(), (db.clone() if with_db else None)
                Fn.wgrad(M, N, dz, dwb2[:, :K], dbias=db2, accumulate=True, **kw)
                assert torch.equal(dwb2[:, :K], dwb[:, :K] + dwb[:, :K]) and torch.all(dwb2[:, K:] == OUT_PAD)
                if with_db:
                    assert torch.equal(db2, db + db)
                got[split] = (dwb[:, :K], db)
            label = f"wgrad_split_kernel<{str(mask).lower()},{str(sub).lower()},{wtk},false> M {M} N {N} K {k1}+{k2}"
            ref, den = dzr.double().t() @ X.double(), dzr.double().abs().t() @ X.double().abs() + 1e-300
            e, _ = _compare(got[False][0], got[True][0], ref, den, label + " dW", False)
            if with_db:
                _compare(got[False][1], got[True][1], dzr.double().sum(0), dzr.double().abs().sum(0) + 1e-300, label + " dbias", False)
            worst[(mask, sub, wtk)] = max(worst.get((mask, sub, wtk), 0.0), e)

        # the workspace bound holds for every [k1 | k2] split of K
        Fn.SplitGemm.enabled = True
        for M, N, K in ((8193, 300, 383), (40000, 64, 161), (4097, 608, 97)):
            Xf = torch.randn(M, K, device=dev)
            dz = torch.randn(M, N, device=dev)
            ref, den = dz.double().t() @ Xf.double(), dz.double().abs().t() @ Xf.double().abs() + 1e-300
            for k1 in sorted({0, K, *(int(v) for v in rng.integers(1, K, 4))}):
                k2 = K - k1
                kw = dict(k1=k1, k2=k2)
                if k1:
                    x1 = torch.zeros(M, (k1 + 3) // 4 * 4, device=dev)
                    x1[:, :k1] = Xf[:, :k1]
                    kw["x1"] = x1
                if k2:
                    x2 = torch.zeros(M, (k2 + 3) // 4 * 4, device=dev)
                    x2[:, :k2] = Xf[:, k1:]
                    kw["x2"] = x2
                dw = torch.empty(N, K, device=dev)
                Fn.wgrad(M, N, dz, dw, **kw)                # (functions._wgrad_launch hands exactly that many bytes)
                e, _ = _err(dw, ref, den)
                Hh.record(f"wgrad M {M} N {N} K {k1}|{k2}", e, 2e-6)
                assert e <= 2e-6, (M, N, k1, k2, e)

        # a split request on an operand whose leading dimension is not a multiple of 4: the scalar wgrad_kernel, silently
        # (its M-chunks are planned for the split kernel's 32-row tiles: against the f32 request, not bit for bit)
        for M, N, k1 in ((4097, 300, 33), (65, 64, 301)):
            dz = torch.randn(M, N, device=dev)
            x1 = torch.randn(M, k1, device=dev)
            outs = []
            for split in (0, 1):
                dw, db = torch.empty(N, k1, device=dev), torch.empty(N, device=dev)
                _wgrad_raw(M, N, dz, dw, x1, k1, split, db)
                outs.append((dw, db))
            label = f"wgrad_kernel (split request, ldx1 {k1}) M {M} N {N}"
            _compare(outs[0][0], outs[1][0], dz.double().t() @ x1.double(), dz.double().abs().t() @ x1.double().abs() + 1e-300,
                     label + " dW", False)
            _compare(outs[0][1], outs[1][1], dz.double().sum(0), dz.double().abs().sum(0) + 1e-300, label + " dbias", False)
    finally:
        Fn.SPLIT_MIN_ROWS, Fn.SplitGemm.enabled, Fn.SplitGemm.f16 = old
    for key in sorted(worst):
        parity_log(f"wgrad_split_kernel<{str(key[0]).lower()},{str(key[1]).lower()},{key[2]},false>: {count[key]} shapes, "
                   f"worst max err / sum|dz||x| {worst[key]:.2e} (bound 2e-06)")
    assert set(worst) == set(T.WGRAD_SPLIT)


# ---------------------------------------------------------------------------------------------- refusals
def test_split_path_refusals_are_statuses_and_leave_the_outputs_alone():
    """shapes the split path does not take come back as a status (RuntimeError from _lib.check) before any launch"""
    M, K = 100, 64
    x = torch.randn(M, K, device=dev)
    w608 = _pack_split(torch.randn(608, K, device=dev), 0, 608, 0, K, 0)
    c = _out(M, 609, 3)
    with pytest.raises(RuntimeError, match=r"\(status -2\)"):                  # RR_ERR_ALIGN: N > 608
        Fn.linear(M, 609, w608, a1=x, k1=K, out=c[:, :609])
    assert torch.all(c == OUT_PAD)
    w = _pack_split(torch.randn(300, K, device=dev), 0, 300, 0, K, 0)
    c = _out(M, 304, 4)
    with pytest.raises(RuntimeError, match=r"\(status -2\)"):                  # RR_ERR_ALIGN: C not 16-byte aligned
        Fn.linear(M, 300, w, a1=x, k1=K, out=c[:, 1:301])
    assert torch.all(c == OUT_PAD)
    wt = _pack_split(torch.randn(300, K, device=dev), 0, 300, 0, K, 0)
    y = torch.randn(M, K, device=dev)
    dz = _out(M, K, 0)
    c = _out(M, 300, 0)
    with pytest.raises(RuntimeError, match=r"\(status -4\)"):                  # RR_ERR_UNSUPPORTED: dz_accumulate
        Fn.linear(M, 300, wt, a1=x, k1=K, a_mask=y, dz_out=dz, dz_accumulate=True, out=c)
    assert torch.all(dz == OUT_PAD) and torch.all(c == OUT_PAD)
    k1 = 62
    w62 = _pack_split(torch.randn(300, k1, device=dev), 0, 300, 0, k1, 0)
    bits = _encode_bits(torch.randn(M, k1, device=dev) > 0)
    with pytest.raises(RuntimeError, match=r"\(status -1\)"):                  # RR_ERR_ARG: sign bits need k1 % 4 == 0
        Fn.linear(M, 300, w62, a1=torch.randn(M, 64, device=dev), k1=k1, a_mask_bits=bits, out=c)
    assert torch.all(c == OUT_PAD)


# ---------------------------------------------------------------------------------------------- row-dot kernel
@pytest.mark.parametrize("N", [1, 2, 8])
def test_rowdot_edges_against_f64(N, monkeypatch):
    """linear_rowdot_kernel (N <= 8, k1 <= 1024, plain packed f32 operand) against f64 at its k edges; at k1 = 1028 the call
    is the MFMA kernel's, bit for bit"""
    for k1 in (4, 1020, 1024, 1028):
        for M in (1, 15, 16, 17, 5000):
            torch.manual_seed(N * 100000 + k1 * 10 + M)
            a = torch.randn(M, k1, device=dev)
            W = torch.randn(N, k1, device=dev) / k1 ** 0.5
            b = torch.randn(N, device=dev)
            wp = _pack_f32(W, N, k1, 0)
            got = Fn.linear(M, N, wp, w_packed=True, a1=a, k1=k1, bias=b)
            monkeypatch.setenv("RR_NO_ROWDOT", "1")
            mfma = Fn.linear(M, N, wp, w_packed=True, a1=a, k1=k1, bias=b)
            monkeypatch.delenv("RR_NO_ROWDOT")
            ref = a.double() @ W.double().t() + b.double()
            den = a.double().abs() @ W.double().abs().t() + b.double().abs() + 1e-300
            e, _ = _err(got, ref, den)
            bound = 2e-6 * max(1.0, k1 / 683)
            Hh.record(f"row-dot N {N} k1 {k1} M {M}", e, bound)
            assert e <= bound, (N, k1, M, e)
            if k1 > 1024:
                assert torch.equal(got, mfma), (N, k1, M)
            elif M == 5000 and k1 >= 1020:                  # (another summation order: the row-dot kernel served the call)
                assert not torch.equal(got, mfma), (N, k1, M)
