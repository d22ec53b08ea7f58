"""No result of the library may depend on what its scratch or output memory held before the call.

Every wrapper of reactranker_amd hands the library uninitialised memory (torch.empty outputs and scratch, the packed-weight
buffers, the step plans' workspace - which from the second training step on is the previous step's activations).  The contract
("What a caller buffer may hold"): every word read from a caller buffer is written earlier in the same
call; the only caller-zeroed words are the ticket counters.  A test process mostly gets zeroed memory, on which a split-K slab
that is summed but not written, a pad column a 16-byte gather reads, a per-block partial past the last block or the gradient
entry of an empty list are all "right".

Each case here runs four times - plain, then with every such buffer filled with 0x00, 0x7F (finite-huge floats: a stale word
that is added shows) and 0xFF (NaN: a stale word multiplied by zero shows), tests/poison.py - and everything it returns or
leaves in .grad must be the same BITS in all four.  No tolerance: the library's claim is fixed-order, bit-reproducible results.
Group B also holds the 0xFF result to a float64 product, so a kernel that is equally wrong under every fill cannot pass here.

Before any integer could be poisoned: the plans' arena (plan.hip Arena / Ctx::alloc / pack / mask_bits) hands out float tensors,
packed weights, sign-bit images and magnitude slots only - every index a plan kernel follows comes from the caller's graph;
eval.ranking_stats' `order`, uncertainty.top1_sets' `rank` / `in_set` and the window losses' `count` are store-only outputs of
their kernels.  The helper fills integer allocations with 0 / 1 regardless."""
import contextlib
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from reactranker_amd import _lib, featurization, synth
from reactranker_amd import eval as E
from reactranker_amd import functions as Fn
from reactranker_amd import loss as RL
from reactranker_amd import uncertainty as U
from reactranker_amd._lib import check, lib, ptr, stream
from reactranker_amd.utils import save_checkpoint
from tests import gemm_dispatch_table as G
from tests import hidden_sizes as HS
from tests import poison
from tests.test_gpu_model import make_model
from tests.test_gpu_ops import close
from tests.test_gpu_plan import CASES as PLAN_CASES
from tests.test_gpu_plan import _run
from tests.test_gpu_uncertainty import _batch as uq_batch
from tests.test_gpu_uncertainty import _model as uq_model
from tests.test_gpu_uncertainty import _quantised

pytestmark = pytest.mark.gpu

# Returned storage that include/reactranker_hip.h documents as unspecified may be left out of a comparison - only through this
# list: (case id prefix, what is left out, the header line that says so).
EXCLUDED = [
    ("pack_weights f16x2", "the bytes of a two-f16-term packed weight buffer behind its scale S",
     "rr_pack_desc.split: \"The bytes of dst behind that float (the buffer is sized for three terms) are unspecified: scratch of "
     "the packing launch, never read by rr_linear_f32\""),
    ("linear", "the bytes of a sign-bit image that stand for no column",
     "rr_linear_args.mask_bits_out: \"Bytes 19 and 39 of a 40-byte block and the bytes of the 16-column tiles past N stand for no "
     "column: they are unspecified (not necessarily written) and never read.\""),
    ("segment_mean", "the pad columns H+F .. r4(H+F)-1 of the readout's pitched output (its reader runs in the same case)",
     "rr_segment_mean_fwd_f32: \"Columns H+F .. ld_out-1 of a row of out (the pad of a pitched output) are unspecified: not "
     "written here, and no result of a kernel that reads the rows with k = H+F depends on them.\""),
]
# byte ranges of the plans' workspace that poisoned() leaves alone (an integer region that could not be shown to be written
# before it is read would go here).  Empty: the arena holds no integers (module docstring).
SPARE_POOL = []

DEV = "cuda"


def _check(case, fn, parity_log, pool=False):
    """fn() plain and under the three fills: same bits, and something was in fact poisoned -> the result under 0xFF"""
    report, counters, last = poison.fill_dependence(fn, spare_pool=SPARE_POOL, sync=torch.cuda.synchronize)
    for byte in poison.FILLS:
        c = counters[byte]
        assert c.buffers > 0 and c.bytes > 0, (case, byte, c)
        assert not pool or c.takes > 0, (case, "no workspace was taken from the pool")
    c = counters[0xFF]
    parity_log(f"{case}: {c.buffers} buffers, {c.bytes} bytes poisoned per fill ({c.takes} pool takes); "
               + ("identical" if not report else "DIFFERENT"))
    assert not report, case + " depends on uninitialised memory:\n  " + "\n  ".join(report[:20])
    return last


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, device=DEV, generator=g) * scale


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(int(seed))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi, shape, device=DEV, generator=g, dtype=torch.int64).to(torch.int32)


def _pitched(t, ld):
    """t's values in a buffer of row pitch ld >= t.shape[1] (zero pad columns: the caller's own memory)"""
    buf = torch.zeros(t.shape[0], ld, device=t.device, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


@contextlib.contextmanager
def _knobs(**kw):
    """class attributes of functions.* for the duration: split=, f16=, chain=, side=, aux=, order="""
    where = dict(split=(Fn.SplitGemm, "enabled"), f16=(Fn.SplitGemm, "f16"), chain=(Fn.FfnChain, "enabled"),
                 side=(Fn.SideStream, "enabled"), aux=(Fn.AuxStream, "enabled"), order=(Fn.WgradOrder, "mode"))
    old = {k: getattr(*where[k]) for k in kw}
    try:
        for k, v in kw.items():
            setattr(*where[k], v)
        yield
    finally:
        for k, v in old.items():
            setattr(*where[k], v)


ARITH = {"f32": dict(split=False, f16=False), "bf16x3": dict(split=True, f16=False), "f16x2": dict(split=True, f16=True)}


def test_the_net_catches_a_kernel_that_reads_what_it_was_handed(parity_log):
    """the positive control, on the GPU: rr_weighted_colsum_f32 told to ACCUMULATE into an uninitialised output reads it - the
    comparison must say so (0 + sum, 3.4e38 + sum and NaN are three different results, whatever the plain run's memory held)"""
    g = _gen(3)
    x, w = _randn(g, 1000, 300), _randint(g, 0, 5, (1000,)).float()
    report, counters, _ = poison.fill_dependence(
        lambda: Fn.weighted_colsum(x, w, 300, torch.empty(300, device=DEV), accumulate=True), sync=torch.cuda.synchronize)
    parity_log(f"control (accumulate into torch.empty): {len(report)} of 3 fills differ from the plain run")
    assert len(report) >= 2 and all(counters[b].buffers == 2 for b in poison.FILLS), report


# =========================================================================================== A. the step plans
# (a plan packs its weights into the workspace on every call - plan.hip pack() allocates from the arena - so the packed weights
# of a plan step are poisoned with the workspace; LinW's cached packs belong to the per-op path and are packed inside fn in B)
def _plan_step(H, d, dd, fd, bias, tn, last, tt, F, p, train, dedup, qb=None):
    cfg = dict(hidden_size=H, mpnn_depth=d, mpnn_diff_depth=dd, ffn_depth=fd, use_bias=bias, task_num=tn, ffn_last_layer=last,
               task_type=tt, add_features_dim=F)
    w = synth.seeded_weights(O.model_shapes(H, d, dd, fd, tn, F, bias), 5)
    model = make_model(cfg, w, dropout=p)
    model = model.train() if train else model.eval()
    model.dedup_reactants = dedup
    if qb is None:
        qb = synth.make_queries(17, 4, [7, 3, 9, 5], atoms_lo=5, atoms_hi=14)          # test_gpu_plan's 4-query batch
    rb, pb = featurization.BatchMolGraph(qb.r_specs, K=4), featurization.BatchMolGraph(qb.p_specs, K=4)
    loss = "mle" if tn == 1 else "lin"
    return (lambda: _run(model, rb, pb, qb, 4242, plan=True, loss=loss)), rb, pb


RUNG = lambda H: (H, 2, 2, 3, True, 1, "with_softplus", None, 1, 0.1, True)            # noqa: E731  (test_gpu_plan's ladder row)
H32, H300 = PLAN_CASES[0], PLAN_CASES[6]
assert H32[0] == 32 and H300[0] == 300 and len(PLAN_CASES) >= 10


@pytest.mark.parametrize("dedup", ["auto", False])
@pytest.mark.parametrize("case", PLAN_CASES[:10], ids=lambda c: f"H{c[0]}-d{c[1]}-dd{c[2]}-f{c[3]}-t{c[5]}-p{c[9]}")
def test_plan_step_of_every_hand_written_case(case, dedup, parity_log):
    with _knobs(**ARITH["bf16x3"]):
        fn, _, _ = _plan_step(*case, dedup)
        _check(f"plan {case} dedup={dedup}", fn, parity_log, pool=True)


@pytest.mark.parametrize("H", [4, 68, 164, 308, 480, 612, 644])
def test_plan_step_at_the_pad_heavy_and_branching_hidden_sizes(H, parity_log):
    """pitches r4(H + F), each split geometry, the f32 layout (612) and the per-layer FFN (644): tests/hidden_sizes.py"""
    assert H in HS.LADDER and HS.plan_taken(H)
    with _knobs(**ARITH["bf16x3"]):
        fn, _, _ = _plan_step(*RUNG(H), "auto")
        _check(f"plan rung H={H}", fn, parity_log, pool=True)


@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("case", [H32, H300], ids=["H32", "H300"])
def test_plan_step_in_the_three_arithmetics(case, arith, parity_log):
    with _knobs(**ARITH[arith]):
        fn, _, _ = _plan_step(*case, "auto")
        _check(f"plan H={case[0]} {arith}", fn, parity_log, pool=True)


@pytest.mark.parametrize("knob", [dict(chain=False), dict(side=False, aux=False), dict(order="early"), dict(order="late")],
                         ids=["no-ffn-chain", "no-side-aux-streams", "wgrad-early", "wgrad-late"])
def test_plan_step_with_each_launch_order_knob(knob, parity_log):
    with _knobs(**ARITH["bf16x3"], **knob):
        fn, _, _ = _plan_step(*H32, "auto")
        _check(f"plan H=32 {knob}", fn, parity_log, pool=True)


def test_plan_step_above_8192_bond_rows(parity_log):
    """the 12-wave geometry of every bond GEMM: test_gpu_headline_kernels' batch (synth.make_queries(seed + 1, Q, 64 ...,
    atoms 16..24)) shrunk to the smallest candidate count in steps of 4 whose bond rows pass 8192 (4 x 60: 8641)"""
    qb = synth.make_queries(502, 4, 60, atoms_lo=16, atoms_hi=24)
    with _knobs(**ARITH["bf16x3"]):
        fn, rb, pb = _plan_step(*H300, "auto", qb=qb)
        assert rb.n_bonds > 8192 and pb.n_bonds > 8192, (rb.n_bonds, pb.n_bonds)
        _check("plan H=300 above 8192 bond rows", fn, parity_log, pool=True)


# =========================================================================================== B. the per-op wrappers
def _scaled_close(got, ref, what):
    """test_wgrad's / test_linear_plain's bound: 2e-5 of the largest entry"""
    s = max(1.0, float(ref.abs().max())) if ref.numel() else 1.0
    close(got / s, ref / s, tol=2e-5, what=what)


def _defined_bits(bits, N):
    """the bytes of a sign-bit image that hold columns (EXCLUDED names the rest): byte 40*b + 20*h + t for the tiles t of block b"""
    if bits is None:
        return None
    assert any(c == "linear" for c, _, _ in EXCLUDED) and bits.shape[1] == 40 * ((N + 303) // 304)
    at = [40 * b + 20 * h + t for b in range((N + 303) // 304) for h in (0, 1) for t in range(min(19, (N - 304 * b + 15) // 16))]
    return bits[:, at]


LINEAR_SHAPES = [(1, 300, 300, 300), (65, 300, 83, 84), (3, 32, 32, 32), (130, 600, 300, 300), (8193, 300, 300, 300)]
# mode 3 (the operand mask as a sign-bit image) exists only where a split GEMM can have written the image: a split layout and
# K % 4 == 0 - not on the f32 layout, not at K = 83.  Those combinations are not cases.
LINEAR_CASES = [(layout, mode, *shape) for layout in sorted(ARITH) for mode in (0, 1, 2, 3) for shape in LINEAR_SHAPES
                if mode != 3 or (layout != "f32" and shape[2] % 4 == 0)]


@pytest.mark.parametrize("layout,mode,M,N,K,ld", LINEAR_CASES)
def test_linear_every_operand_mode_and_weight_layout(layout, mode, M, N, K, ld, parity_log):
    """rr_linear_f32 on packed weights.  Modes 0 / 1 in the forward's form (bias, residual, ReLU, the sign-bit image of the
    output where the split GEMM writes one); modes 2 / 3 in the backward's (masked operand, dZ side output, the weighted column
    sums).  Mode 3 reads the mask as the sign-bit image a split GEMM wrote for it (LINEAR_CASES)."""
    g = _gen(1000 * M + N + K + mode)
    W, b = _randn(g, N, K, scale=K ** -0.5), _randn(g, N)
    if mode == 0:
        a = _pitched(_randn(g, M, K), ld)
        ref = torch.relu(a.double() @ W.double().t() + b.double())
    elif mode == 1:
        nS = M + 7
        src_a, src_s = _pitched(_randn(g, nS, K), ld), _pitched(_randn(g, nS, K), ld)
        ia, isub = _randint(g, 0, nS, (M,)), _randint(g, 0, nS, (M,))
        inp = _randn(g, M, N)
        ref = torch.relu(inp.double() + (src_a[ia.long()] - src_s[isub.long()]).double() @ W.double().t() + b.double())
    else:
        dy = _pitched(_randn(g, M, K), ld)
        rw = _randint(g, 0, 5, (M,)).float()
        with _knobs(**ARITH[layout]):                     # the mask: a split GEMM's ReLU + dropout output with its sign bits
            y = Fn.linear(M, K, Fn.LinW(_randn(g, K, K, scale=K ** -0.5), None).pk(K), w_packed=True, a1=_randn(g, M, K), k1=K,
                          act=Fn.ACT_RELU, drop_p=0.2, seed=9, want_bits=(mode == 3))
        if mode == 2 or ld != K:
            y = _pitched(y, ld)                           # same values, no sign-bit image attached (rows 16-byte addressable)
        ref = (dy * (y > 0) * 1.25).double() @ W.double().t()

    def fn():
        with _knobs(**ARITH[layout]):
            L = Fn.LinW(W, b)
            wp = L.pk(K)                                   # packed under the fill as well
            if mode == 0:
                out = Fn.linear(M, N, wp, w_packed=True, a1=a, k1=K, bias=L.b, act=Fn.ACT_RELU, want_bits=True)
                return out, _defined_bits(getattr(out, "_rr_bits", None), N)
            if mode == 1:
                out = Fn.linear(M, N, wp, w_packed=True, a1=src_a, k1=K, a1_idx=ia, a1_sub=src_s, a1_sub_idx=isub, bias=L.b,
                                residual=inp, act=Fn.ACT_RELU, want_bits=True)
                return out, _defined_bits(getattr(out, "_rr_bits", None), N)
            dz = torch.empty(M, K, device=DEV) if K % 4 == 0 else None      # (the side output needs 16-byte rows)
            out, part = Fn.linear(M, N, wp, w_packed=True, a1=dy, k1=K, a_mask=y, mask_scale=1.25, dz_out=dz, colsum_w=rw)
            return out, part, dz
    last = _check(f"linear {layout} mode {mode} M={M} N={N} K={K} ld={ld}", fn, parity_log)
    if layout != "f32":
        assert G.geometry(M, N)[2] == (12 if (M > 8192 or N > 304) else 8)
        if mode < 2:
            assert last[1] is not None and last[1].dtype == torch.uint8           # the mask-bits output was written and compared
    if mode == 3:
        assert getattr(y, "_rr_bits", None) is not None                           # mode 3 was in fact reached
    _scaled_close(last[0], ref, "linear under 0xFF vs f64")
    if mode >= 2:
        want = (rw.double()[:, None] * ref).sum(0)
        scale = float((rw.double()[:, None] * ref.abs()).sum(0).max()) + 1e-30
        assert float((last[1][:, :N].double().sum(0) - want).abs().max()) <= 2e-5 * scale   # colsum side output vs f64
        if last[2] is not None:
            assert torch.equal(last[2], dy * (y > 0) * 1.25)


WGRAD_K = [(83, 0), (61, 300), (300, 0)]
assert sorted(G.wgrad_wtk(*k) for k in WGRAD_K) == [3, 4, 5]                    # each WTK class once


def _wgrad_case(name, M, N, k1, k2, parity_log, mask=True, gather=False, sub=False):
    g = _gen(M + N + k1 + k2 + 7 * gather + 11 * sub)
    nS = 150 if gather else M
    x1 = _pitched(_randn(g, nS, k1), (k1 + 3) // 4 * 4)
    xi = _randint(g, -1, nS, (M,)) if gather else None
    xs = _pitched(_randn(g, M + 7, k1), (k1 + 3) // 4 * 4) if sub else None
    xsi = _randint(g, -1, M + 7, (M,)) if sub else None
    x2 = _randn(g, M, k2) if k2 else None
    dy = _randn(g, M, N)
    y = torch.relu(_randn(g, M, N)) if mask else None

    def rows(src, idx):
        return src if idx is None else torch.where((idx >= 0)[:, None], src[idx.clamp(min=0).long()], torch.zeros((), device=DEV))
    X = rows(x1, xi).double() - (rows(xs, xsi).double() if sub else 0.0)
    if x2 is not None:
        X = torch.cat([X, x2.double()], 1)
    dz = (dy * (y > 0) * 0.5).double() if mask else dy.double()
    ref_w, ref_b = dz.t() @ X, dz.sum(0)

    def fn():
        dw, db = torch.empty(N, k1 + k2, device=DEV), torch.empty(N, device=DEV)
        Fn.wgrad(M, N, dy, dw, dbias=db, mask=y, mask_scale=0.5, x1=x1, k1=k1, x1_idx=xi, x1_sub=xs, x1_sub_idx=(xsi if sub else None),
                 x2=x2, k2=k2)
        acc, accb = torch.ones(N, k1 + k2, device=DEV), torch.ones(N, device=DEV)
        Fn.wgrad(M, N, dy, acc, dbias=accb, mask=y, mask_scale=0.5, x1=x1, k1=k1, x1_idx=xi, x1_sub=xs,
                 x1_sub_idx=(xsi if sub else None), x2=x2, k2=k2, accumulate=True)
        return dw, db, acc, accb
    with _knobs(**ARITH["bf16x3"]):
        last = _check(name, fn, parity_log)
    s = max(1.0, float(ref_w.abs().max()))
    close(last[0] / s, ref_w / s, tol=2e-5, what="dw under 0xFF vs f64")
    close(last[1] / s, ref_b / s, tol=2e-5, what="db under 0xFF vs f64")


@pytest.mark.parametrize("M", [1, 16, 100, 5000, 70000])
@pytest.mark.parametrize("k1,k2", WGRAD_K)
def test_wgrad_slabs_and_reduction(M, k1, k2, parity_log):
    """rr_linear_wgrad_f32's split-M slabs (the `ws` of functions._wgrad_launch) and their fixed-order reduction, fresh and
    accumulating: the fast kernel below 8192 rows, the split kernel at 70000"""
    _wgrad_case(f"wgrad M={M} N=300 k=({k1},{k2}) wtk={G.wgrad_wtk(k1, k2)}", M, 300, k1, k2, parity_log)


@pytest.mark.parametrize("what,M,kw", [("gather", 9000, dict(gather=True, mask=False)), ("gather-sub", 9000, dict(gather=True, sub=True, mask=False)),
                                       ("sub+mask", 100, dict(sub=True)), ("no mask", 100, dict(mask=False))])
def test_wgrad_operand_forms(what, M, kw, parity_log):
    _wgrad_case(f"wgrad {what} M={M}", M, 300, 300, 0, parity_log, **kw)


def test_wgrad_scalar_fallback(parity_log):
    _wgrad_case("wgrad scalar fallback N=2 k1=33", 100, 2, 33, 0, parity_log)


@pytest.mark.parametrize("n", [1, 255, 256, 70001])
def test_weighted_colsum(n, parity_log):
    g = _gen(n)
    x, w = _randn(g, n, 300), _randint(g, 0, 5, (n,)).float()

    def fn():
        fresh = Fn.weighted_colsum(x, w, 300, torch.empty(300, device=DEV), accumulate=False)
        plain = Fn.weighted_colsum(x, None, 300, torch.empty(300, device=DEV), accumulate=False)
        acc = Fn.weighted_colsum(x, w, 300, torch.full((300,), 2.0, device=DEV), accumulate=True)
        return fresh, plain, acc
    last = _check(f"weighted_colsum n={n}", fn, parity_log)
    l1 = (w[:, None] * x.abs()).double().sum(0)
    assert bool(((last[0].double() - (w[:, None].double() * x.double()).sum(0)).abs() <= 1e-6 * l1 + 1e-5).all())


GATHERS = ["sum", "sum_1d", "masked", "dropmask", "multi", "epilogue", "csr", "padrow", "diff", "dropout"]
NEEDS_16_BYTE_ROWS = {"dropmask", "epilogue"}             # rr_gather_sum_dropmask_f32 / _epi_f32 return RR_ERR_ALIGN otherwise


@pytest.mark.parametrize("H,ld", [(30, 30), (300, 300), (300, 304)])
@pytest.mark.parametrize("kind", GATHERS)
def test_gather_variants(kind, H, ld, parity_log):
    g = _gen(H + ld + len(kind))
    n_src, n_out, K = 517, 301, 4
    src = _pitched(_randn(g, n_src, H), ld)
    idx = _randint(g, -1, n_src, (n_out, K))
    idx[0] = -1
    mask = _pitched(torch.relu(_randn(g, n_src, H)), ld)
    ymask = torch.relu(_randn(g, n_out, H))
    adds = [_randn(g, n_out, H) for _ in range(3)]
    part = _randn(g, 29, (H + 3) // 4 * 4)
    ia, im = _randint(g, -1, n_src, (n_out,)), _randint(g, -1, n_src, (n_out,))
    offsets, dest = Fn._transpose_index(idx.clamp(min=0), n_src)
    rows = torch.div(dest, K, rounding_mode="floor").to(torch.int32)
    go = _randn(g, n_out, H)
    fns = {
        "sum": lambda: Fn.gather_sum(src, idx, H),
        "sum_1d": lambda: Fn.gather_sum(src, ia, H),
        "masked": lambda: Fn.gather_sum_masked(src, mask, 1.0 / 0.9, idx, H),
        "dropmask": lambda: Fn.gather_sum_dropmask(src, ymask, 1.0 / 0.9, idx, H, 0.1, 0x1234ABCD5678),
        "multi": lambda: Fn.gather_sum_multi([src, mask, src], idx, H),
        "epilogue": lambda: Fn.gather_sum(src, idx, H, row0_partial=part, mask=ymask, mask_scale=1.25, adds=adds),
        "csr": lambda: Fn.gather_sum_csr(go, offsets, rows, n_src, H),
        "padrow": lambda: Fn.gather_sum(src, idx, H, row0_partial=part),
        "diff": lambda: Fn.gather_diff(src, ia, src, im, H),
        "dropout": lambda: Fn.gather_dropout(src, ia.clamp(min=0), H, 0.2, 77),
    }
    case = f"gather {kind} H={H} ld={ld}"
    if kind in NEEDS_16_BYTE_ROWS and H % 4 != 0:
        with poison.poisoned(0xFF) as c, pytest.raises(RuntimeError):            # refused, not mangled - under the fill too
            fns[kind]()
        parity_log(f"{case}: refused (rows are not 16-byte chunks); {c.buffers} buffers poisoned")
        return
    last = _check(case, fns[kind], parity_log)
    if kind == "sum":
        want = torch.where((idx >= 0)[..., None], src[idx.clamp(min=0).long()], torch.zeros((), device=DEV)).double().sum(1)
        close(last, want, what="gather_sum under 0xFF vs f64")


def _mol_graph(g_seed, n_mols):
    rng = np.random.default_rng(g_seed)
    sizes = rng.integers(1, 9, size=n_mols)
    M, nA = len(sizes), int(sizes.sum()) + 1
    starts = np.concatenate([[1], 1 + np.cumsum(sizes)[:-1]])
    a_scope = np.stack([starts, sizes], 1).astype(np.int32)
    atom2mol = np.full(nA, -1, np.int32)
    for m, (s0, n) in enumerate(a_scope):
        atom2mol[s0:s0 + n] = m
    return SimpleNamespace(a_scope=torch.as_tensor(a_scope).cuda(), atom2mol=torch.as_tensor(atom2mol).cuda(), M=M, nA=nA)


@pytest.mark.parametrize("H,F,p", [(300, 1, 0.1), (32, 0, 0.0), (30, 1, 0.2)])
def test_segment_mean_forward_and_backward(H, F, p, parity_log):
    """the readout: its output is pitched (r4(H + F) floats a row, H + F in view) - the view is what is compared"""
    mg = _mol_graph(H + F, 37)
    g = _gen(H)
    x, dout = _randn(g, mg.nA, H), _randn(g, mg.M, H + F)
    feat = _randn(g, mg.M, F) if F else None
    hid = torch.relu(_randn(g, mg.nA, H))
    wb = _ffn_layers([H + F, 64, 1], H)

    def fn():
        fwd = Fn.segment_mean_fwd(x, mg, H, feat, F, p, 77)        # (compared over the H + F columns in view: EXCLUDED)
        # ... and its reader: the FFN's first GEMM walks the pitched rows in 16-byte lanes (k1 = H + F, pitch r4(H + F))
        ffn = Fn.ffn_forward(fwd, [Fn.LinW(w, b, big=False) for w, b in wb], 0.0, 5, 0)[0]
        bwd = Fn.segment_mean_bwd(dout, mg, H, F, p, 77)
        masked = Fn.segment_mean_bwd(dout, mg, H, F, p, 77, mask=hid, mask_scale=1.25) if H % 4 == 0 else None
        return fwd, bwd, masked, ffn
    assert any(c == "segment_mean" for c, _, _ in EXCLUDED)
    _check(f"segment_mean H={H} F={F} p={p}", fn, parity_log)


def test_elementwise_wrappers(parity_log):
    g = _gen(5)
    n = 1001 * 30
    dy, y = _randn(g, n), torch.relu(_randn(g, n))
    adds = [_randn(g, n) for _ in range(15)]
    acc0 = _randn(g, n)

    def fn():
        acc = acc0.clone()
        out = dict(relu_bwd=Fn.relu_bwd(dy, y, -1.5), relu_bwd_acc=Fn.relu_bwd(dy, y, -1.5, acc=acc), acc=acc,
                   relu_bwd_misaligned=Fn.relu_bwd(dy[1:], y[1:], 2.0),           # relu_bwd_scalar_kernel
                   sum0=Fn.relu_bwd_sum(dy, y, 1.25, []), sum15=Fn.relu_bwd_sum(dy, y, 1.25, adds),
                   axpy=Fn.axpby(2.0, dy), axpby=Fn.axpby(2.0, dy, -1.0, y), dropout=Fn.dropout(dy, 0.2, 0x1234567890ABCDEF))
        return out
    last = _check("relu_bwd / relu_bwd_sum / axpby / dropout", fn, parity_log)
    assert torch.equal(last["relu_bwd_misaligned"], dy[1:] * (y[1:] > 0) * 2.0)
    assert torch.equal(last["axpby"], 2.0 * dy - y)


@pytest.mark.parametrize("head,N", [(0, 1), (1, 1), (2, 1), (3, 2), (4, 2), (5, 2), (6, 4), (3, 4), (6, 8)])
def test_head_forward_and_backward(head, N, parity_log):
    g = _gen(head * 10 + N)
    raw, go = _randn(g, 50, N, scale=5.0), _randn(g, 50, N)
    raw[0, 0] = 25.0                                       # softplus threshold branch
    _check(f"head {head} N={N}", lambda: (Fn.head_fwd(raw, head), Fn.head_bwd(go, raw, head)), parity_log)


def _ffn_layers(widths, seed):
    g = _gen(seed)
    return [(_randn(g, n, k, scale=k ** -0.5), _randn(g, n, scale=0.3)) for k, n in zip(widths[:-1], widths[1:])]


@pytest.mark.parametrize("H,inst", [(128, (8, 1)), (132, (8, 3)), (388, (8, 5))])
def test_ffn_chain_forward_and_backward(H, inst, parity_log):
    """rr_ffn_chain_f32 (csrc/ffn.hip) as the plans call it, every stage's output and the packed weights allocated uninitialised:
    forward [H + 1, H, H, 1] and the input-gradient chain back to the H readout columns"""
    widths = HS.forward_widths(H)
    assert HS.chain_of(widths)[1] == inst and HS.chain_of(HS.backward_widths(H), rowdot=False)[1] == inst
    M, p, seed = 37, 0.1, 91
    K0, nl = widths[0], len(widths) - 1
    wb = _ffn_layers(widths, 3)
    g = _gen(H)
    x = torch.zeros(M, (K0 + 3) // 4 * 4, device=DEV)
    x[:, :K0] = _randn(g, M, K0)
    d = _randn(g, M, widths[-1])
    ks = 1.0 / (1.0 - p)

    def fn():
        layers = [Fn.LinW(w, b, big=False) for w, b in wb]
        a = _lib.FfnChainArgs()
        a.M, a.n_stages, a.x, a.ldx, a.drop_p, a.mask_scale = M, nl, ptr(x), x.stride(0), p, 1.0
        hs, keep, k = [], [], K0
        for li, L in enumerate(layers):
            s, n = a.stage[li], L.w.shape[0]
            wp = L.pk(k)
            keep.append(wp)
            s.w, s.ldw, s.bias, s.n_out, s.n_in = ptr(wp), wp.stride(0), ptr(L.b), n, k
            if li < nl - 1:
                o = torch.empty(M, (n + 3) // 4 * 4, device=DEV)
                s.relu, s.dropout, s.drop_seed = 1, 1, Fn._site_seed(seed, 4000 + li)
            else:
                o = torch.empty(M, n, device=DEV)
                s.rowdot = 1
            s.out, s.ld_out = ptr(o), o.stride(0)
            hs.append(o)
            k = n
        check(lib().rr_ffn_chain_f32(C.byref(a), stream()), "rr_ffn_chain_f32")
        bk = _lib.FfnChainArgs()
        bk.M, bk.n_stages, bk.x, bk.ldx, bk.drop_p, bk.mask_scale = M, nl, ptr(d), d.stride(0), 0.0, ks
        outs = []
        for j in range(nl):
            li = nl - 1 - j
            L = layers[li]
            nin = L.w.shape[1] if li > 0 else H            # the readout columns only
            wt = L.pk_t(0, nin)
            keep.append(wt)
            s = bk.stage[j]
            s.w, s.ldw, s.n_out, s.n_in = ptr(wt), wt.stride(0), nin, L.w.shape[0]
            o = torch.empty(M, (nin + 3) // 4 * 4, device=DEV)
            s.out, s.ld_out = ptr(o), o.stride(0)
            if li > 0:
                s.post_mask, s.ld_mask = ptr(hs[li - 1]), hs[li - 1].stride(0)
            outs.append(o)
        check(lib().rr_ffn_chain_f32(C.byref(bk), stream()), "rr_ffn_chain_f32")
        return hs, outs, keep                               # (every width is a multiple of 4: no pad column anywhere)
    last = _check(f"ffn chain <{inst[0]},{inst[1]}> H={H}", fn, parity_log)
    ref = x[:, :K0].double()
    assert p > 0                                            # (dropout on: the f64 check is of the raw first layer only)
    first = torch.relu(ref @ wb[0][0].double().t() + wb[0][1].double())
    kept = last[0][0] != 0
    _scaled_close(torch.where(kept, last[0][0].double() / ks, first), first, "ffn chain first layer under 0xFF vs f64")


@pytest.mark.parametrize("layout", sorted(ARITH))
@pytest.mark.parametrize("rows,k1,k2", [(300, 83, 0), (300, 61, 300), (32, 32, 0), (600, 300, 0), (612, 612, 83)])
def test_packed_weights_are_the_same_bytes_pad_columns_included(layout, rows, k1, k2, parity_log):
    """rr_pack_weights_f32 into the uninitialised buffers of LinW._pack: the GEMMs read the zero pad of every k-segment, so the
    whole buffer is compared, for W = [W1 | W2] and for a transposed column slice"""
    g = _gen(rows + k1 + k2)
    w = _randn(g, rows, k1 + k2)

    def content(buf):
        """what rr_pack_desc.split says the buffer receives: all of it, except in the two-f16-term form, whose images take two
        thirds of the rr_split_weight_bytes() bytes and are followed by the scale S (EXCLUDED names the rest)"""
        if not getattr(buf, "_rr_f16", False):
            return buf
        assert any(c == "pack_weights f16x2" for c, _, _ in EXCLUDED)
        nblk = buf.numel() // 3072                         # [k-step][tile] blocks of 2 terms x 64 lanes x 8 f16
        return buf[:nblk * 2048 + 4]

    def fn():
        with _knobs(**ARITH[layout]):
            L = Fn.LinW(w, None)
            return content(L.pk(k1, k2)), content(L.pk_t(0, (k1 + 3) // 4 * 4 if (k1 + 3) // 4 * 4 <= k1 + k2 else k1))
    last = _check(f"pack_weights {layout} rows={rows} k=({k1},{k2})", fn, parity_log)
    if last[0].dtype == torch.float32:                     # the f32 layout: [rows, r16(k1) + r16(k2)], zero pad
        r16 = lambda k: (k + 15) & ~15                     # noqa: E731
        assert last[0].shape[1] == int(lib().rr_packed_weight_ld(k1, k2))
        want = torch.zeros_like(last[0])
        want[:, :k1] = w[:, :k1]
        want[:, r16(k1):r16(k1) + k2] = w[:, k1:]
        assert torch.equal(last[0], want)


# =========================================================================================== C. losses, evaluation, uncertainty
SCOPE = [0, 1, 2, 63, 64, 65, 300]                        # the empty list and both sides of the one-wave limit
MC = sum(SCOPE)


def _scores(seed, *shape, positive=False):
    q = _quantised(np.random.default_rng(seed), shape)
    return torch.from_numpy(np.abs(q) + 0.25 if positive else q).cuda()


def _grad_of(make_loss, inputs, fused):
    """forward + backward of a loss on fresh leaves -> (loss, every leaf's grad); fused: start the backward with the library's
    constant one (loss.backward(loss): the gradient the step launch already wrote)"""
    xs = [x.clone().requires_grad_(True) for x in inputs]
    out = make_loss(*xs)
    extra = None
    if isinstance(out, tuple):
        out, extra = out
    if out.numel() != 1:                                   # a vector result (soft_rank, LogCumsumExp): a weighted sum of it
        (out * torch.linspace(0.5, 1.5, out.numel(), device=out.device)).sum().backward()
    elif fused:
        RL.backward(out)
    else:
        (out.sum() * 1.0).backward()                       # any other upstream gradient: the backward kernel
    return out.detach(), extra, [x.grad for x in xs]


LIST_LOSS_NAMES = ["MLEloss", "ListnetLoss", "evidential_ranking", "ranknet_loss", "lambdarank_loss", "lambdarank_loss pairs=", "soft_rank",
                   "approx_ndcg_loss", "approx_ndcg_loss queries=", "MLEDisLoss", "Listnet_For_Gauss", "Listnetlognorm",
                   "Listnet_For_evidential", "Listnet_with_uq", "Dirichlet_uq", "betanet_loss", "beta_evidential_loss"]
LIST_LOSS_NAMES += [f"task_step_loss {tt}" for tt in sorted(RL.TASK_STEPS)]
_CACHE = {}


def _targets_list():
    if "t" not in _CACHE:
        _CACHE["t"] = _scores(900, MC)
    return _CACHE["t"]


def _list_losses():
    """name -> (inputs, loss(*leaves)); built on first use (the module imports without a GPU)"""
    if "losses" in _CACHE:
        return _CACHE["losses"]
    T_LIST = _targets_list()
    LIST_LOSSES = {
        # name: (inputs, loss(*leaves))
        "MLEloss": ([_scores(1, MC)], lambda s: RL.MLEloss()(s, SCOPE, T_LIST, 0)),
        "ListnetLoss": ([_scores(2, MC)], lambda s: RL.ListnetLoss()(s, SCOPE, T_LIST, 0)),
        "evidential_ranking": ([_scores(3, MC, 2, positive=True)], lambda s: RL.evidential_ranking()(s, SCOPE, T_LIST, None, None, None, 0)),
        "ranknet_loss": ([_scores(4, MC)], lambda s: RL.ranknet_loss(s, SCOPE, T_LIST, 1.0, 0)),
        "lambdarank_loss": ([_scores(5, MC)], lambda s: RL.lambdarank_loss(s, SCOPE, T_LIST, 1.0, 10, 0)),
        "lambdarank_loss pairs=": ([_scores(5, MC)], lambda s: RL.lambdarank_loss(s, SCOPE, T_LIST, 1.0, 0, 0, pairs=1234)),
        "soft_rank": ([_scores(6, MC)], lambda s: RL.soft_rank(s, SCOPE, 0.5, 0)),
        "approx_ndcg_loss": ([_scores(7, MC)], lambda s: RL.approx_ndcg_loss(s, SCOPE, T_LIST, 0.5, 10, 0)),
        "approx_ndcg_loss queries=": ([_scores(7, MC)], lambda s: RL.approx_ndcg_loss(s, SCOPE, T_LIST, 0.5, 0, 0, queries=7)),
        "MLEDisLoss": ([_scores(8, MC, 1), _scores(9, MC, 1, positive=True)], lambda m, v: RL.MLEDisLoss()(m, v, SCOPE, T_LIST, 0)),
        "Listnet_For_Gauss": ([_scores(10, MC, 1), _scores(11, MC, 1, positive=True)], lambda m, v: RL.Listnet_For_Gauss()(m, v, SCOPE, T_LIST, 0)),
        "Listnetlognorm": ([_scores(12, MC, 1, positive=True), _scores(13, MC, 1, positive=True)],
                           lambda m, v: RL.Listnetlognorm()(m, v, SCOPE, T_LIST, 0)),
        "Listnet_For_evidential": ([_scores(14, MC, 1), _scores(15, MC, 1, positive=True), _scores(16, MC, 1, positive=True) + 1.0],
                                   lambda m, v, a: RL.Listnet_For_evidential()(m, v, a, SCOPE, T_LIST, 0)),
        "Listnet_with_uq": ([_scores(17, MC, positive=True)], lambda s: RL.Listnet_with_uq()(s, SCOPE, T_LIST, 0.5, 3, 10, 0)),
        "Dirichlet_uq": ([_scores(18, MC, positive=True)], lambda s: RL.Dirichlet_uq()(s, SCOPE, T_LIST, 0.5, 3, 10, 0)),
        "betanet_loss": ([_scores(19, MC)], lambda s: RL.betanet_loss(s, SCOPE, T_LIST, 100.0, 0)),
        "beta_evidential_loss": ([_scores(20, MC, positive=True)], lambda s: RL.beta_evidential_loss(s, SCOPE, T_LIST, 0.3, 0)),
    }
    LIST_LOSSES.update({
        f"task_step_loss {tt}": ([_scores(30 + i, MC, positive=True) if RL.TASK_STEPS[tt][2] == 1 else _scores(30 + i, MC, 2, positive=True)],
                                (lambda tt: lambda o: RL.task_step_loss(tt, o, SCOPE, T_LIST, 0, coef=0.25))(tt))
        for i, tt in enumerate(sorted(RL.TASK_STEPS))})
    assert sorted(LIST_LOSSES) == sorted(LIST_LOSS_NAMES)
    _CACHE["losses"] = LIST_LOSSES
    return LIST_LOSSES


@pytest.mark.parametrize("name", LIST_LOSS_NAMES)
def test_per_list_losses_forward_backward_and_fused_step(name, parity_log):
    """ragged scope with the empty list: the gradient is compared whole (entries of lists that contribute nothing included),
    through the backward kernel and, where the forward launch writes it (FusedStep), as that launch left it"""
    inputs, make = _list_losses()[name]

    def fn():
        plain = _grad_of(make, inputs, fused=False)
        fused = _grad_of(make, inputs, fused=True)
        with torch.no_grad():
            fwd = make(*inputs)                             # no gradient wanted: the forward-only entry
        return plain, fused, fwd
    last = _check(f"loss {name}", fn, parity_log)
    assert all(gr is not None and gr.shape == x.shape for gr, x in zip(last[0][2], inputs))


def test_statistics_with_no_candidate_at_all(parity_log):
    """scope [0, 0]: outputs of max(total, 1) / max(Q, 1) elements behind an empty view"""
    empty = torch.zeros(0, device=DEV)

    def fn():
        return dict(sample_stats=U.sample_stats(torch.zeros(3, 0, device=DEV), [0, 0], empty, 0),
                    top1_sets=U.top1_sets(empty, [0, 0], empty, 0.5, 0),
                    analytic=U.analytic_stats(torch.zeros(0, 2, device=DEV), [0, 0], empty, "gaussian", 8, 0))
    _check("statistics on scope [0, 0]", fn, parity_log)


@pytest.mark.parametrize("n", [1, 1000])
def test_pointwise_losses(n, parity_log):
    t = _scores(40 + n, n)
    m, v = _scores(41 + n, n), _scores(42 + n, n, positive=True)
    pos = [_scores(43 + n + i, n, positive=True) + (1.0 if i == 1 else 0.0) for i in range(3)]     # v, alpha > 1, beta
    pairs_y, pairs_t = _scores(47 + n, n, 2, positive=True), _scores(48 + n, n, 2)

    def fn():
        out = dict(
            gauss=_grad_of(lambda a, b: RL.GaussDisLoss()(a, b, t, 0), [m, v], False),
            mse=_grad_of(lambda a: RL.MSELoss()(a, t), [m], False),
            lognorm=_grad_of(lambda a, b: RL.Lognorm()(a, b, t, 0), [v, v * 0.5], False),
            exp_mse=_grad_of(lambda a: RL.ExpMSELoss()(a, t), [m * 0.25], False),
            nig=_grad_of(lambda mu, vv, al, be: RL.evidential_loss_new(mu, vv, al, be, t, 0), [m] + pos, False),
            nig_cross=_grad_of(lambda mu, vv, al, be: RL.evidential_loss_new(mu, vv, al, be, t, 0),
                               [x.reshape(-1, 1) for x in [m] + pos], False),
            pair_mse=_grad_of(lambda y: RL.pair_softmax_mse(y, pairs_t), [pairs_y], False),
            logcumsumexp=_grad_of(lambda a: RL.LogCumsumExp.apply(a), [m], False),
            digamma=RL.digamma(v), ranknet_lambda=RL.ranknet_lambda(m, [n], t, 1.0, 0),
            pair_acc=E.pair_acc_from_outputs(pairs_y, pairs_t))
        return out
    _check(f"pointwise losses n={n}", fn, parity_log)


def test_evaluation_functions(parity_log):
    s, s2 = _scores(60, MC), _scores(61, MC, 2)
    T_LIST = _targets_list()

    def fn():
        return dict(ranking_stats=E.ranking_stats(s, SCOPE, T_LIST, 0), ranking_stats_2d=E.ranking_stats(s2, SCOPE, T_LIST, 0, 0.5, 0.25),
                    metrics=E.ranking_metrics_from_scores(s, SCOPE, T_LIST, 0), top=E.top_scores_from_scores(s, SCOPE, T_LIST, 0),
                    rank_corr=E.rank_correlation_stats(s, SCOPE, T_LIST, 0), rank_corr_dict=E.rank_correlation_from_scores(s, SCOPE, T_LIST, 0),
                    ndcg=E.ndcg_at_k(s, SCOPE, T_LIST.abs().round(), 0), pairwise=E.pairwise_stats_from_scores(s, SCOPE, T_LIST, 1.0, 0))
    last = _check("eval.py on the ragged scope", fn, parity_log)
    order = last["ranking_stats"][1]
    assert order.dtype == torch.int32 and order.shape[0] == MC             # the predicted orders: written, in range
    off = 0
    for c in SCOPE:
        assert sorted(order[off:off + c].tolist()) == list(range(c))
        off += c


def test_uncertainty_functions(parity_log, tmp_path):
    samples = _scores(70, 7, MC)
    out4 = torch.cat([_scores(71, MC, 1), _scores(72, MC, 3, positive=True)], 1)
    out4[:, 2] += 1.0                                      # alpha > 1
    pred, std = _scores(73, 1000), _scores(74, 1000, positive=True)
    tgt = _scores(75, 1000)
    T_LIST = _targets_list()
    p1 = U.sample_stats(samples, SCOPE, T_LIST, 0)["p_top1"].clone()
    model, ens_model, b = uq_model(0.1, 12), uq_model(0.1, 1), uq_batch(22, nq=5)     # (the ensemble replaces its model's weights)
    paths = []
    for i, ws in enumerate((31, 32)):
        paths.append(str(tmp_path / f"{i}.pt"))
        save_checkpoint(paths[-1], uq_model(0.1, ws))

    def fn():
        return dict(sample_stats=U.sample_stats(samples, SCOPE, T_LIST, 0),
                    gaussian=U.analytic_stats(out4, SCOPE, T_LIST, "gaussian", 32, 0),
                    log_variance=U.analytic_stats(out4 * 0.5, SCOPE, T_LIST, "log_variance", 8, 0),
                    nig=U.analytic_stats(out4, SCOPE, T_LIST, "nig", 32, 0),
                    calibration=U.uncertainty_calibration(pred, tgt, std), calibration1=U.uncertainty_calibration(pred[:1], tgt[:1], std[:1]),
                    gauss=U.probabilistic_calibration(pred, tgt, std, 20, 1.3), gauss1=U.probabilistic_calibration(pred[:1], tgt[:1], std[:1]),
                    sigma=U.fit_sigma_scale(pred, tgt, std), top1=U.top1_sets(p1, SCOPE, T_LIST, 0.6, 0),
                    mc=U.mc_dropout_predict(model, [b], 3, seed=1, gpu=0), ens=U.ensemble_predict(ens_model, paths, [b], gpu=0))
    last = _check("uncertainty.py on the ragged scope", fn, parity_log)
    rank = last["top1"]["rank"]
    assert rank.dtype == torch.int32 and int(rank.min()) >= 1 and int(rank.max()) <= max(SCOPE)


# =========================================================================================== D. the pool as it really runs
def test_real_pool_large_small_large_reuses_one_buffer(parity_log, monkeypatch):
    """No poison: a large step (H = 300), a small one (H = 32), the large one again through the real _WorkspacePool - the small
    step runs in the large step's leftovers, the second large step in both's.  Each is the same bits as the step of group A run
    on NaN-filled memory, and the pool allocated once."""
    with _knobs(**ARITH["bf16x3"]):
        large, _, _ = _plan_step(*H300, "auto")
        small, _, _ = _plan_step(*H32, "auto")
        refs = {}
        for name, fn in (("large", large), ("small", small)):
            with poison.poisoned(0xFF, SPARE_POOL) as c:
                refs[name] = poison.snapshot(fn())
            assert c.takes > 0
        torch.cuda.synchronize()
        monkeypatch.setattr(Fn._WorkspacePool, "free", [])
        before = Fn._WorkspacePool.allocs
        for name, fn in (("large", large), ("small", small), ("large", large)):
            got = poison.snapshot(fn())
            assert poison.differences(refs[name], got) == [], name
        assert Fn._WorkspacePool.allocs == before + 1
        assert len(Fn._WorkspacePool.free) == 1
    parity_log("real pool, H=300 then H=32 then H=300: 1 allocation, each step identical to its NaN-filled run")
