"""The balanced last round of linear_split_kernel's one-block-per-workgroup launches (reactranker_amd/csrc/linear_split.hip,
launch_split_epi): the grid in which the row blocks behind the last whole round of full blocks share their 64-row units
equally over the CUs - tail blocks of 4 or 8 active waves - against the grid of full blocks that RR_NO_BALANCED_TAIL=1
restores.  Which workgroup computes which rows is all that changes, and the rows do not interact: every output tensor (the
result, c_pre, the sign bits, dz_out, the column-sum partials) must be the same bits, the dropout stream - indexed by
element - included.

Every non-persistent 12-wave leaf of tests/gemm_dispatch_table.py is run (MODE 0 - 3 with their EPI variants, both
geometries; the two-column-block geometry <38,19,*,12> and the one-block form of the persistent instantiation keep the grid
of full blocks, so both of their runs take the same launch: they are here so that a later change of that is held too), at
row counts on both sides of every edge of the host's rule, restated in _tail_units.  The generic-loader twins EPI 2 / 3 and
the two-f16-term form (w_packed = 3) are not mapped either (split_balanced in the source): their kernels are the parent's."""
import os

import pytest
import torch

from reactranker_amd import functions as Fn
from reactranker_amd._lib import lib
from tests import gemm_dispatch_table as T
from tests.test_gpu_gemm_dispatch import _decode_bits, _encode_bits, _n_cu
from tests.test_gpu_split import _pack_split

pytestmark = pytest.mark.gpu
dev = "cuda"
KNOB = "RR_NO_BALANCED_TAIL"
FILL = 7.5               # outputs start out as this: a row no workgroup wrote keeps it

LEAVES = [leaf for leaf in T.LINEAR_LEAVES if leaf[3] == 12 and not leaf[5]]


def _tail_units(M, n_cu):
    """(full blocks F, tail units T) of launch_split_epi's rule; the map is used where 0 < T <= 2 * n_cu"""
    units = (M + 63) // 64
    full = units // (3 * n_cu) * n_cu
    return full, units - 3 * full


def _row_counts(n_cu):
    """the two sizes of the headline step, one and a few rows past a whole round, both sides of T = 2 * cus (the map's upper
    edge: above it the grid of full blocks stays), T = cus and cus + 1 (every tail block one unit / the first one two), and
    a second round that is all tail; 71,425, 138,881 and 192 * cus + 777 are not multiples of 16"""
    ms = [71425, 138881, 192 * n_cu + 1, 192 * n_cu + 777, 64 * (5 * n_cu + 1), 64 * 5 * n_cu, 64 * 4 * n_cu - 3, 64 * (4 * n_cu + 1) - 21,
          64 * (3 * n_cu + 2) - 63]
    assert any(m % 16 for m in ms)
    return ms


def _case(leaf, M, seed):
    """arguments of Fn.linear that tests/gemm_dispatch_table.leaf_of sends to `leaf`, with every side output the form allows"""
    ntp, nt, mode, waves, epi, _ = leaf
    n_cu = _n_cu()
    g = torch.Generator(device=dev).manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, device=dev, generator=g)
    N = 300 if ntp == 19 else 600
    wide = mode in (0, 1) and epi >= 2
    residual = mode in (0, 1) and epi % 2 == 1
    k1, k2 = (1000, 0) if wide else (300, 0)
    if mode == 0 and epi == 0:
        k1, k2 = 257, 0                                # an odd number of k-steps: the one-block form of the persistent shape
    if mode == 0 and epi == 1:
        k1, k2 = 61, 300                               # two segments
    assert T.leaf_of(M, N, k1, k2, mode, residual, n_cu) == leaf, (leaf, M)
    K = k1 + k2
    W = rn(N, K) / K ** 0.5
    ld1 = (k1 + 3) // 4 * 4
    kw = dict(k1=k1)
    out = {}
    if mode in (0, 1):
        n_src = M // 2 + 3
        a1 = torch.zeros(n_src, ld1, device=dev)
        a1[:, :k1] = rn(n_src, k1)
        idx = torch.randint(-1, n_src, (M,), device=dev, generator=g).to(torch.int32)
        kw.update(a1=a1, a1_idx=idx, bias=rn(N), act=Fn.ACT_RELU, drop_p=0.1, seed=seed * 7919 + 5)
        if mode == 1:
            sub = torch.zeros(M // 3 + 2, ld1, device=dev)
            sub[:, :k1] = rn(M // 3 + 2, k1)
            kw.update(a1_sub=sub, a1_sub_idx=torch.randint(-1, M // 3 + 2, (M,), device=dev, generator=g).to(torch.int32))
        if k2:
            kw.update(a2=rn(M, k2), k2=k2)
        if residual:
            kw.update(residual=rn(M // 2 + 3, N), residual_idx=torch.randint(-1, M // 2 + 3, (M,), device=dev, generator=g).to(torch.int32))
        out = dict(c_pre=(M, N), mask_bits_out=None)
        colsum = False
    else:
        y = rn(M, k1)
        kw.update(a1=rn(M, k1), mask_scale=1.0 / 0.9)
        if mode == 2:
            kw["a_mask"] = y
        else:
            kw["a_mask_bits"] = _encode_bits(y > 0)
        out = dict(dz_out=(M, k1))
        colsum = True
    return M, N, _pack_split(W, 0, N, 0, k1, k2), kw, out, colsum, g


def _run(M, N, w, kw, outs, cw):
    bufs = {"out": torch.full((M, N), FILL, device=dev)}
    for name, shape in outs.items():
        if name == "mask_bits_out":
            bufs[name] = torch.full((M, int(lib().rr_mask_bits_row_bytes(N))), 0xA5, dtype=torch.uint8, device=dev)
        else:
            bufs[name] = torch.full(shape, FILL, device=dev)
    res = Fn.linear(M, N, w, colsum_w=cw, **kw, **bufs)
    if cw is not None:
        bufs["colsum_partial"] = res[1]
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("leaf", LEAVES, ids=[T.leaf_name(leaf).strip("<>") for leaf in LEAVES])
def test_balanced_grid_gives_the_bits_of_the_grid_of_full_blocks(leaf):
    n_cu = _n_cu()
    assert os.environ.get(KNOB) is None
    mapped = 0
    for i, M in enumerate(_row_counts(n_cu)):
        full, tail = _tail_units(M, n_cu)
        mapped += 0 < tail <= 2 * n_cu
        _, N, w, kw, outs, colsum, g = _case(leaf, M, 100 * i + 3)
        cw = torch.rand(M, device=dev, generator=g) if colsum else None
        new = _run(M, N, w, kw, outs, cw)
        os.environ[KNOB] = "1"
        try:
            old = _run(M, N, w, kw, outs, cw)
        finally:
            del os.environ[KNOB]
        for name in old:
            assert torch.equal(new[name], old[name]), (T.leaf_name(leaf), M, name, full, tail)
        # every row was written (a row of FILL after bias / ReLU / dropout or a random GEMM does not happen by itself), and the
        # sign bits of the columns below N (the layout's padding bits are not specified) are those of what was stored
        assert bool((new["out"] != FILL).any(1).all()), (T.leaf_name(leaf), M)
        if "dz_out" in new:
            assert bool((new["dz_out"] != FILL).any(1).all())
        if cw is not None:                             # the partials are fresh memory in each run: held to the stored output too
            part = new["colsum_partial"]                 # (one row per 64-row unit, a sum of depth < 16 per 16 rows: the bound of
            units = (M + 63) // 64                       # tests/test_gpu_gemm_dispatch.py, per unit)
            assert part.shape[0] == units == int(lib().rr_linear_colsum_rows(M))
            wo = torch.zeros(units * 64, N, dtype=torch.float64, device=dev)
            wo[:M] = new["out"].double() * cw.double()[:, None]
            want, den = wo.view(units, 64, N).sum(1), wo.view(units, 64, N).abs().sum(1) + 1e-300
            e_cs = float(((part[:, :N].double() - want).abs() / den).max())
            print(f"[balanced tail] {T.leaf_name(leaf)} M {M}: column-sum partials, max err / sum|.| per unit {e_cs:.2e}")
            assert e_cs <= 2.0 ** -20, (T.leaf_name(leaf), M, e_cs)
            del wo, want, den
        if "mask_bits_out" in new:
            assert torch.equal(_decode_bits(new["mask_bits_out"], N), new["out"] > 0), (T.leaf_name(leaf), M)
        del new, old, w, kw, cw
    assert mapped >= 5                                 # (the row counts do reach the map's side of the rule, whatever the CU count)


def test_row_counts_cover_the_rule_s_edges():
    n_cu = _n_cu()
    tails = {M: _tail_units(M, n_cu) for M in _row_counts(n_cu)}
    assert tails[64 * (5 * n_cu + 1)] == (n_cu, 2 * n_cu + 1) and tails[64 * 5 * n_cu] == (n_cu, 2 * n_cu)
    assert tails[192 * n_cu + 1] == (n_cu, 1) and tails[64 * 4 * n_cu - 3][1] == n_cu and tails[64 * (4 * n_cu + 1) - 21][1] == n_cu + 1
    if n_cu == 256:
        assert tails[71425] == (256, 349) and tails[138881] == (512, 635)
