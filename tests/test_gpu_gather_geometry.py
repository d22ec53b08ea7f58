"""Every launch form of csrc/gather.hip against an exact reference (tests/gather_ref.py: a numpy float32 restatement that adds
in table order, so the comparison is on int32 views - bit for bit, signs of zero included).

The cases are named by the launch geometry they select and ASSERT it from the host's own arithmetic
(grid = min(ceil(n_out * HV / 256), RR_GRID_CAP), per-block ranges rounded to whole 256-thread passes):
  one_wg      below one workgroup
  xcd         one pass per thread, grid % 8 == 0 (gather_block_range permutes the blocks over the 8 XCDs)
  plain       one pass per thread, grid % 8 != 0 (identity map); H = 30 takes the scalar kernels
  capped      more chunks than RR_GRID_CAP workgroups cover in one pass: gather_walk's (row, column) carry and index prefetch
  hv257       H = 1028: more 16-byte chunks per row than a pass has threads (gather_walk's quo = 0, rem = 256)
Only output row 0 of the padding-row forms is a tree sum: it is held to 2e-6 x the summed magnitudes and to run-to-run
bit-stability, the rule of test_gpu_ops.py::test_linear_weighted_colsum_side_output_and_padrow_gather."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from reactranker_amd import functions as Fn
from reactranker_amd._lib import check, lib, ptr, stream
from tests import gather_ref as R
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

N_SRC = 4099
GEOMS = {
    # name: (H, n_out, class)
    "one_wg_h32_n1": (32, 1, "one_wg"), "one_wg_h32_n2": (32, 2, "one_wg"), "one_wg_h32_n3": (32, 3, "one_wg"),
    "one_wg_h300_n1": (300, 1, "one_wg"), "one_wg_h300_n2": (300, 2, "one_wg"), "one_wg_h300_n3": (300, 3, "one_wg"),
    "xcd_h300": (300, 7179, "xcd"),
    "plain_h300_2100_blocks": (300, 7168, "plain"), "plain_h300": (300, 977, "plain"), "plain_h600": (600, 977, "plain"),
    "plain_h30_scalar": (30, 977, "plain"),
    "capped_h300": (300, 30011, "capped"), "capped_h32": (32, 270001, "capped"), "capped_hv257": (1028, 8200, "capped"),
    "hv257": (1028, 977, "plain"),
}
ONE_PER_CLASS = ["one_wg_h300_n2", "xcd_h300", "plain_h300", "capped_h300", "hv257"]


def _geometry(name, vec=None):
    """Asserts that the case still selects the launch it is named after, from the host's arithmetic."""
    H, n_out, cls = GEOMS[name]
    vec = (H % 4 == 0) if vec is None else vec
    g = R.geometry(n_out, H, vec)
    if cls == "one_wg":
        assert g["one_workgroup"] and g["blocks"] == 1 and g["passes"] == 1, g
    elif cls == "xcd":
        assert not g["capped"] and g["xcd"] and g["passes"] == 1 and g["blocks"] > 8, g
    elif cls == "plain":
        assert not g["capped"] and not g["xcd"] and g["passes"] == 1 and g["blocks"] > 1, g
    else:
        assert g["capped"] and g["blocks"] == R.grid_cap() and g["passes"] >= 2, ("RR_GRID_CAP moved: re-derive the capped cases", g)
        assert n_out * H * 4 < 40e6                       # (every capped case stays under 40 MB of output)
    if name.endswith("hv257"):
        assert g["HV"] > 256
    if name == "plain_h300_2100_blocks":
        assert g["blocks"] == 2100
    return H, n_out, g


def dev(a):
    return torch.as_tensor(a).cuda()


@functools.lru_cache(maxsize=6)
def _src(H, ld=None, seed=0):
    """[N_SRC, ld] sources: normal values, 1 % negative zeros, rows 7 and 11 all -0.0; pad columns (ld > H) are NaN, so a
    kernel that reads or copies one shows."""
    ld = H if ld is None else ld
    rng = np.random.default_rng(1000 * seed + H)
    a = np.full((N_SRC, ld), np.nan, np.float32)
    v = rng.standard_normal((N_SRC, H)).astype(np.float32)
    v[rng.random((N_SRC, H)) < 0.01] = -0.0
    v[7] = v[11] = -0.0
    a[:, :H] = v
    return a


def _idx(n_out, K, seed, lo=-1):
    """[n_out, K] in [lo, N_SRC): row 0 all pad (the padding row), row 5 all pad, row 9 sums rows of -0.0 only (the result
    must be +0.0), row 10 is pads followed by one row of -0.0."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(lo, N_SRC, size=(n_out, K)).astype(np.int32)
    idx[0] = -1
    if n_out > 5:
        idx[5] = -1
    if n_out > 10:
        idx[9] = 7
        idx[10] = -1
        idx[10, -1] = 11
    return idx


def _pitched(a, ld, fill=np.nan):
    """[n, H] values in a [n, ld] buffer whose pad columns hold `fill`; returns (device buffer, device view of the payload)."""
    n, H = a.shape
    buf = np.full((n, ld), fill, np.float32)
    buf[:, :H] = a
    t = dev(buf)
    return t, t[:, :H]


def _dist64(what, got, ref64):
    """The float64 distance beside the bit comparison (parity log only)."""
    Hh.record(what + ": |got - f64| / (1 + |f64|)", float(np.max(np.abs(got.astype(np.float64) - ref64) / (1 + np.abs(ref64)))) if got.size else 0.0)


def _sum64(src, idx, H, rows):
    idx = idx.reshape(idx.shape[0], -1)[rows]
    return np.where(idx[..., None] >= 0, src[np.maximum(idx, 0), :H].astype(np.float64), 0.0).sum(1)


def _sample(n_out):
    return slice(None) if n_out <= 8192 else slice(0, None, 37)


def _bits(got, ref, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    if not R.same_bits(got, ref):
        bad = np.argwhere(np.ascontiguousarray(got, np.float32).view(np.int32) != np.ascontiguousarray(ref, np.float32).view(np.int32))
        r, c = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ref.size} elements differ in bits; first at row {r} column {c}: "
                             f"got {got[r, c]!r}, reference {ref[r, c]!r}; rows affected {np.unique(bad[:, 0])[:8]}")


def _sum_call(src, n_src, ld_src, idx, n_out, K, H, out, ld_out, part=None, slot=None):
    check(lib().rr_gather_sum_amax_f32(ptr(src), n_src, ld_src, ptr(idx), n_out, K, H, ptr(part), 0 if part is None else part.shape[0],
                                       0 if part is None else part.stride(0), ptr(out), ld_out, ptr(slot), stream()), "rr_gather_sum_amax_f32")


def _row0_rule(row0, part, H, what):
    """Row 0 of a padding-row form: the fixed-order tree sum of the partial rows, within 2e-6 x the summed magnitudes."""
    p64 = part[:, :H].double()
    want = p64.sum(0)
    scale = float(p64.abs().sum(0).max()) + 1e-30
    err = float((row0.double() - want).abs().max())
    Hh.record(what + ": padding row, |err| / summed magnitudes", err / scale, 2e-6)
    assert err <= 2e-6 * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------ rr_gather_sum_f32 / _amax_ / _padrow_
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 9])
@pytest.mark.parametrize("name", list(GEOMS))
def test_gather_sum_plain_amax_and_padrow_over_every_geometry(name, K):
    """K = 1..4 take gather_walk<K>, K >= 5 the generic loop (with its K % 4 remainder); each as the plain launch, with the
    magnitude slot, and with the padding-row reduction blocks appended to the grid (gblocks = gridDim - HV)."""
    H, n_out, g = _geometry(name)
    src_h, idx_h = _src(H), _idx(n_out, K, 100 * K + n_out % 97)
    ref = R.gather_sum(src_h, idx_h, H)
    src, idx = dev(src_h), dev(idx_h)
    got = Fn.gather_sum(src, idx, H)
    _bits(got, ref, f"rr_gather_sum_f32 {name} K={K}")
    rows = _sample(n_out)
    _dist64(f"gather_sum {name}", got.cpu().numpy()[rows], _sum64(src_h, idx_h, H, rows))
    if n_out > 10:
        assert not np.signbit(ref[9]).any() and not np.signbit(ref[10]).any()       # 0 + (-0.0) = +0.0
    # the magnitude slot: same output, slot = largest stored magnitude (read as tests/test_gpu_f16x2.py reads it)
    out = torch.full((n_out, H), float("nan"), device="cuda")
    slot = torch.zeros(_lib.RR_AMAX_FLOATS, device="cuda")
    _sum_call(src, N_SRC, H, idx, n_out, K, H, out, H, slot=slot)
    assert torch.equal(out, got) and float(slot.max()) == float(out.abs().max())
    # padding row: rows 1.. are the same gather, row 0 the tree sum of the partial rows
    part = dev(np.random.default_rng(K).standard_normal((29, (H + 3) // 4 * 4)).astype(np.float32))
    out2 = torch.full((n_out, H), float("nan"), device="cuda")
    slot2 = torch.zeros(_lib.RR_AMAX_FLOATS, device="cuda")
    _sum_call(src, N_SRC, H, idx, n_out, K, H, out2, H, part=part, slot=slot2)
    assert torch.equal(out2[1:], got[1:])
    _row0_rule(out2[0], part, H, f"padrow {name}")
    assert float(slot2.max()) == float(out2.abs().max())
    assert torch.equal(Fn.gather_sum(src, idx, H, row0_partial=part), out2)                 # rr_gather_sum_padrow_f32, run to run


@pytest.mark.parametrize("n_partial", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("name,K", [("one_wg_h300_n1", 3), ("one_wg_h32_n1", 6), ("plain_h300", 3), ("plain_h300", 6), ("xcd_h300", 2),
                                    ("xcd_h300", 5), ("plain_h30_scalar", 3), ("hv257", 6), ("capped_h300", 9)])
def test_padding_row_reduction_blocks(name, K, n_partial):
    """The reduction blocks' row loop (two rows in flight per thread, 512-row stride, an odd tail) at the partial counts where it
    changes form; n_out == 1 is the launch whose gather blocks have nothing to write (row 0 is the only row)."""
    H, n_out, g = _geometry(name)
    src_h, idx_h = _src(H), _idx(n_out, K, 7 * K + n_partial)
    src, idx = dev(src_h), dev(idx_h)
    part = dev(np.random.default_rng(n_partial).standard_normal((n_partial, (H + 3) // 4 * 4)).astype(np.float32))
    got = Fn.gather_sum(src, idx, H, row0_partial=part)
    _bits(got[1:], R.gather_sum(src_h, idx_h, H)[1:], f"padrow {name} K={K}")
    _row0_rule(got[0], part, H, f"padrow {name} n_partial={n_partial}")
    assert torch.equal(Fn.gather_sum(src, idx, H, row0_partial=part), got)


# ------------------------------------------------------------------------------------------------ rr_gather_sum_epi_f32
def _mask_for(H, n_out, kind):
    """(mask tensor as the wrapper takes it, its values on the host): the sign-bit image is what a split GEMM wrote for its
    ReLU + dropout output (only widths it can run at), the f32 form is that output without the image."""
    if kind == "none":
        return None, None
    if H in (32, 300, 304, 600):
        g = torch.Generator(device="cuda").manual_seed(H + n_out)
        W = torch.randn(H, H, device="cuda", generator=g) / 17
        x = torch.randn(n_out, H, device="cuda", generator=g)
        y = Fn.linear(n_out, H, Fn.LinW(W, None).pk(H), w_packed=True, a1=x, k1=H, act=Fn.ACT_RELU, drop_p=0.2, seed=9, want_bits=True)
        assert getattr(y, "_rr_bits", None) is not None
    else:
        assert kind == "f32"
        y = dev(np.maximum(np.random.default_rng(H).standard_normal((n_out, H)), 0).astype(np.float32))
    return (y if kind == "bits" else y.clone()), y.cpu().numpy()


def _epi_case(geom, K, n_adds, padrow, kind):
    H, n_out, g = geom
    what = f"epi H={H} n_out={n_out} K={K} adds={n_adds} padrow={padrow} mask={kind}"
    src_h, idx_h = _src(H), _idx(n_out, K, 31 * K + n_adds)
    src, idx = dev(src_h), dev(idx_h)
    rng = np.random.default_rng(n_adds + 17 * K)
    adds_h = [rng.standard_normal((n_out, H)).astype(np.float32) for _ in range(n_adds)]
    adds = [dev(a) for a in adds_h]
    part = dev(rng.standard_normal((29, H)).astype(np.float32)) if padrow else None
    mask, mask_h = _mask_for(H, n_out, kind)
    plain = None if mask is None else mask.clone()
    got = Fn.gather_sum(src, idx, H, row0_partial=part, mask=mask, mask_scale=1.25, adds=adds)
    # the separate-kernel sequence
    gsum = Fn.gather_sum(src, idx, H, row0_partial=part)
    if mask is None:
        want = Fn.relu_bwd_sum(gsum, torch.ones_like(gsum), 1.0, adds) if adds else gsum
    else:
        want = Fn.relu_bwd_sum(gsum, plain, 1.25, adds) if adds else Fn.relu_bwd(gsum, plain, 1.25)
    assert torch.equal(got, want), what
    # the numpy restatement (row 0 of a padding-row form: the epilogue on the tree sum the kernels agree on, held by the padrow tests)
    ref_g = R.gather_sum(src_h, idx_h, H)
    if padrow:
        ref_g[0] = gsum[0].cpu().numpy()
    _bits(got, R.epilogue(ref_g, H, mask_h, 1.25, adds_h), what)
    return got


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 8, 9])
@pytest.mark.parametrize("H", [32, 300, 304, 600, 1028])
def test_gather_sum_epilogue_every_pad_width_addend_count_and_mask_form(H, K):
    """gather_sum_epi_kernel: K <= 4 with n_adds <= 5 runs gather_walk with the prefetched epilogue (epi_load / epi_finish), everything
    else the generic loop + epi_apply<NADD> (unrolled addends up to 5, a run-time loop above) - each with and without the
    padding-row blocks, without a mask, with the f32 mask and with its sign-bit image: bit-identical to
    rr_gather_sum(_padrow)_f32 + rr_relu_bwd_sum_f32 and to the numpy restatement."""
    n_out = 977
    geom = (H, n_out, R.geometry(n_out, H))
    assert not geom[2]["capped"] and geom[2]["passes"] == 1
    for n_adds in (0, 3, 5, 7, 15):
        for padrow in (False, True):
            for kind in (("none", "f32") if H == 1028 else ("none", "f32", "bits")):
                _epi_case(geom, K, n_adds, padrow, kind)


@pytest.mark.parametrize("K", [3, 6])
def test_gather_sum_epilogue_capped_grid(K):
    """The fused epilogue where every thread walks two chunks: the last gather of a depth-4 backward (three addends, sign-bit
    mask, padding row), K = 3 on gather_walk and K = 6 on the generic loop."""
    _epi_case(_geometry("capped_h300"), K, 3, True, "bits")


# ------------------------------------------------------------------------------------------------ rr_gather_dropout_f32 / _amax_
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", list(GEOMS))
def test_gather_dropout_over_every_geometry(name, p):
    """gather_walk<1, false>: a copy with the destination row's keep bits - the sign of -0.0 survives (no 0 + v), pads read +0.0."""
    H, n_out, g = _geometry(name)
    src_h = _src(H)
    idx_h = _idx(n_out, 1, n_out % 89).reshape(-1)
    seed = 0x1234ABCD5678
    ref = R.gather_dropout(src_h, idx_h, H, p, seed)
    src, idx = dev(src_h), dev(idx_h)
    got = Fn.gather_dropout(src, idx, H, p, seed)
    _bits(got, ref, f"rr_gather_dropout_f32 {name} p={p}")
    if n_out > 10:
        assert np.signbit(ref[9]).all() if p == 0 else np.signbit(ref[9]).any()              # rows of -0.0 stay -0.0 where kept
        assert not np.signbit(ref[5]).any()
    out = torch.full((n_out, H), float("nan"), device="cuda")
    slot = torch.zeros(_lib.RR_AMAX_FLOATS, device="cuda")
    check(lib().rr_gather_dropout_amax_f32(ptr(src), N_SRC, H, ptr(idx), n_out, H, p, seed, ptr(out), H, ptr(slot), stream()), "gather_dropout_amax")
    assert torch.equal(out, got) and float(slot.max()) == float(out.abs().max())


# ------------------------------------------------------------------------------------------------ the grid-stride kernels with the XCD map
@pytest.mark.parametrize("name", ONE_PER_CLASS + ["plain_h30_scalar"])
def test_gather_sum_masked_and_diff_over_the_geometry_classes(name):
    H, n_out, g = _geometry(name)
    K = 5
    src_h, mask_h, idx_h = _src(H), np.maximum(_src(H, seed=1), 0), _idx(n_out, K, n_out % 83)
    src, mask, idx = dev(src_h), dev(mask_h), dev(idx_h)
    _bits(Fn.gather_sum_masked(src, mask, 1.0 / 0.9, idx, H), R.gather_sum_masked(src_h, mask_h, 1.0 / 0.9, idx_h, H),
          f"rr_gather_sum_masked_f32 {name}")
    ia, im = _idx(n_out, 1, 3).reshape(-1), _idx(n_out, 1, 4).reshape(-1)
    im[0] = 3
    other = _src(H, seed=1)
    _bits(Fn.gather_diff(src, dev(ia), dev(other), dev(im), H), R.gather_diff(src_h, ia, other, im, H), f"rr_gather_diff_f32 {name}")


@pytest.mark.parametrize("name", ONE_PER_CLASS)
def test_gather_sum_dropmask_and_multi_over_the_geometry_classes(name):
    H, n_out, g = _geometry(name)
    capped = g["capped"]
    K = 2 if capped else 5                                 # (the reference hashes n_out * H * K stream elements on the host)
    seed, p = 0x5EED5EED77, 0.1
    src_h, idx_h = _src(H), _idx(n_out, K, n_out % 79)
    y_h = np.maximum(np.random.default_rng(n_out).standard_normal((n_out, H)), 0).astype(np.float32)
    src, idx = dev(src_h), dev(idx_h)
    for pp in (p, 0.0):
        _bits(Fn.gather_sum_dropmask(src, dev(y_h), 1.0 / 0.9, idx, H, pp, seed), R.gather_sum_dropmask(src_h, y_h, 1.0 / 0.9, idx_h, H, pp, seed),
              f"rr_gather_sum_dropmask_f32 {name} p={pp}")
    for n_srcs, Km in ((3, 5), (4, 2), (2, 1)):
        if capped and n_srcs != 3:
            continue
        srcs_h = [_src(H, seed=s) for s in range(n_srcs)]
        idx_m = _idx(n_out, Km, 11 * Km)
        _bits(Fn.gather_sum_multi([dev(s) for s in srcs_h], dev(idx_m), H), R.gather_sum_multi(srcs_h, idx_m, H),
              f"rr_gather_sum_multi_f32 {name} n_srcs={n_srcs} K={Km}")


_EVERY_K = [1, 2, 3, 4, 5, 6, 7, 8, 9]                   # every K % 4, with and without a full group of four


@pytest.mark.parametrize("name,K", [(n, K) for n in ("plain_h300", "one_wg_h300_n3") for K in _EVERY_K] +
                         [("plain_h30_scalar", K) for K in (3, 4, 7)])
def test_gather_sum_masked_at_every_pad_width_remainder(name, K):
    """gather_row_sum's groups of four and its one-by-one remainder as gather_sum_masked_kernel<4> runs them (a source chunk and
    a mask chunk per entry), and the scalar kernel at a remainder, a whole group and both."""
    H, n_out, g = _geometry(name)
    src_h, mask_h, idx_h = _src(H), np.maximum(_src(H, seed=1), 0), _idx(n_out, K, 13 * K + n_out % 83)
    _bits(Fn.gather_sum_masked(dev(src_h), dev(mask_h), 1.0 / 0.9, dev(idx_h), H), R.gather_sum_masked(src_h, mask_h, 1.0 / 0.9, idx_h, H),
          f"rr_gather_sum_masked_f32 {name} K={K}")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("K", _EVERY_K)
@pytest.mark.parametrize("name", ["plain_h300", "one_wg_h300_n3"])
def test_gather_sum_dropmask_at_every_pad_width_remainder(name, K, p):
    """The same loop with gather_sum_dropmask_kernel's derived mask: its term also sees the entry's index (pads are off, the keep
    bits are those of source row j), with the dropout stream and without (threshold 0)."""
    H, n_out, g = _geometry(name)
    seed = 0x5EED5EED77
    src_h, idx_h = _src(H), _idx(n_out, K, 17 * K + n_out % 79)
    y_h = np.maximum(np.random.default_rng(n_out + K).standard_normal((n_out, H)), 0).astype(np.float32)
    _bits(Fn.gather_sum_dropmask(dev(src_h), dev(y_h), 1.0 / 0.9, dev(idx_h), H, p, seed),
          R.gather_sum_dropmask(src_h, y_h, 1.0 / 0.9, idx_h, H, p, seed), f"rr_gather_sum_dropmask_f32 {name} K={K} p={p}")


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n_srcs", [2, 3, 4])
def test_gather_sum_multi_at_every_source_count_and_pair_remainder(n_srcs, K):
    """gather_sum_multi_kernel<NS>: two rows x NS loads in flight, (acc + t0) + t1 per pair and an odd last entry - every source
    count with no pair, whole pairs only, and pairs with a remainder."""
    H, n_out, g = _geometry("plain_h300")
    srcs_h = [_src(H, seed=s) for s in range(n_srcs)]
    idx_h = _idx(n_out, K, 19 * K + n_srcs)
    _bits(Fn.gather_sum_multi([dev(s) for s in srcs_h], dev(idx_h), H), R.gather_sum_multi(srcs_h, idx_h, H),
          f"rr_gather_sum_multi_f32 n_srcs={n_srcs} K={K}")


# ------------------------------------------------------------------------------------------------ rr_gather_sum_csr_f32
def _csr_table(n_out, rng, big=1000):
    """Row source counts cycling through 0, 1, 2, 3, 4 with one row of `big` sources; the first and the last row are empty."""
    counts = np.arange(n_out) % 5
    counts[0] = counts[-1] = 0
    if n_out > 3:
        counts[n_out // 2] = big
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return offsets, rng.integers(0, N_SRC, size=int(offsets[-1])).astype(np.int32)


def _csr_call(src, ld_src, offsets, idx, n_out, H, out, ld_out):
    check(lib().rr_gather_sum_csr_f32(ptr(src), N_SRC, ld_src, ptr(offsets), ptr(idx), n_out, H, ptr(out), ld_out, stream()), "rr_gather_sum_csr_f32")


@pytest.mark.parametrize("H,n_out", [(300, 1), (300, 977), (300, 30011), (30, 1), (30, 977), (30, 70001)])
def test_gather_sum_csr_against_the_sequential_sum(H, n_out):
    """The adjoint of a gather through a generic index table: two sources per iteration with an odd-count tail, added in table order."""
    g = R.geometry(n_out, H, H % 4 == 0)
    assert g["capped"] == (n_out > 30000) and (not g["capped"] or g["passes"] >= 2)
    rng = np.random.default_rng(H + n_out)
    src_h = _src(H)
    tables = [_csr_table(n_out, rng)]
    if n_out == 1:                                         # the only row: empty, odd, even, long
        tables = [(np.array([0, c], np.int32), rng.integers(0, N_SRC, size=max(c, 1)).astype(np.int32)) for c in (0, 1, 3, 4, 1000, 1001)]
    for offsets, idx in tables:
        ref = R.gather_sum_csr(src_h, offsets, idx, H)
        got = Fn.gather_sum_csr(dev(src_h), dev(offsets), dev(idx), n_out, H)
        _bits(got, ref, f"rr_gather_sum_csr_f32 H={H} n_out={n_out} nnz={int(offsets[-1])}")


@pytest.mark.parametrize("H", [300, 30])
def test_index_select_wrappers_backward_is_torch_index_selects(H):
    """functions.GatherSumFn / IndexSelectNDFn (their backward is rr_gather_sum_csr_f32 over a device-built CSR transpose) against
    torch.index_select's own backward in float64: within 2e-6 x the summed magnitudes of the gradient rows a source receives."""
    rng = np.random.default_rng(H)
    n_src, n, K = 301, 977, 5
    src_h = rng.standard_normal((n_src, H)).astype(np.float32)
    index = rng.integers(0, n_src, size=(n, K))
    index[:, 0] = 3                                        # one source read by every destination row: a 977-term segment
    index[index == 17] = 18                                # and one that nobody reads
    go_nd = rng.standard_normal((n, K, H)).astype(np.float32)
    s64 = torch.tensor(src_h, dtype=torch.float64, requires_grad=True)
    ref_fwd = s64.index_select(0, torch.tensor(index).reshape(-1)).view(n, K, H)
    for Fnc, go, fwd in ((Fn.IndexSelectNDFn, go_nd, ref_fwd), (Fn.GatherSumFn, go_nd[:, 0], ref_fwd.sum(1))):
        s = dev(src_h).requires_grad_(True)
        out = Fnc.apply(s, dev(index))
        assert np.allclose(out.detach().cpu().numpy(), fwd.detach().numpy(), rtol=0, atol=1e-5)
        out.backward(dev(go))
        ref, = torch.autograd.grad(fwd, s64, torch.tensor(go, dtype=torch.float64), retain_graph=True)
        mag, = torch.autograd.grad(fwd, s64, torch.tensor(go, dtype=torch.float64).abs(), retain_graph=True)
        err = (s.grad.double().cpu() - ref).abs()
        Hh.record(f"{Fnc.__name__} backward H={H}: |err| / summed magnitudes", float((err / (mag + 1e-30)).max()), 2e-6)
        assert bool((err <= 2e-6 * mag).all()), Fnc.__name__
        assert float(s.grad[17].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ pitched rows
@pytest.mark.parametrize("H,ld", [(300, 304), (30, 32), (30, 31)])
def test_pitched_rows_leave_the_pad_columns_alone(H, ld):
    """Every entry point that takes a pitch, with ld_src / ld_out (and ld_add, ld_mask, ld_partial, ld_y) larger than H: sources whose
    pad columns are NaN, outputs preset to NaN - afterwards the pad columns still are and the payload has none and equals the
    reference bit for bit.  H % 4 != 0 or a pitch that is not: the scalar kernels, or RR_ERR_ALIGN where there are none."""
    n_out, K = 977, 5
    vec = R.vectorised(H, ld)
    g = R.geometry(n_out, H, vec)
    assert not g["capped"] and not g["one_workgroup"]
    rng = np.random.default_rng(H + ld)
    src_h, idx_h = _src(H, ld), _idx(n_out, K, ld)
    src, idx = dev(src_h), dev(idx_h)

    def fresh():
        return torch.full((n_out, ld), float("nan"), device="cuda")

    def held(buf, ref, what):
        a = buf.cpu().numpy()
        assert np.isnan(a[:, H:]).all(), what + ": a pad column was written"
        _bits(a[:, :H], ref, what)
    ref_sum = R.gather_sum(src_h, idx_h, H)
    buf = fresh()
    Fn.gather_sum(src[:, :H], idx, H, out=buf[:, :H])
    held(buf, ref_sum, "gather_sum")
    # padding row with pitched partials
    part_h = rng.standard_normal((257, H)).astype(np.float32)
    pbuf, part = _pitched(part_h, ld)
    buf = fresh()
    Fn.gather_sum(src[:, :H], idx, H, out=buf[:, :H], row0_partial=part)
    _row0_rule(buf[0, :H], part, H, f"pitched padrow H={H} ld={ld}")
    ref = ref_sum.copy()
    ref[0] = buf[0, :H].cpu().numpy()
    held(buf, ref, "gather_sum padrow")
    # the fused epilogue: pitched addends and f32 mask (16-byte chunks only)
    adds_h = [rng.standard_normal((n_out, H)).astype(np.float32) for _ in range(3)]
    mask_h = np.maximum(rng.standard_normal((n_out, H)), 0).astype(np.float32)
    adds = [_pitched(a, ld)[1] for a in adds_h]
    mask = _pitched(mask_h, ld)[1]
    buf = fresh()
    if vec:
        Fn.gather_sum(src[:, :H], idx, H, out=buf[:, :H], row0_partial=part, mask=mask, mask_scale=1.25, adds=adds)
        held(buf, R.epilogue(ref, H, mask_h, 1.25, adds_h), "gather_sum epilogue")
    else:
        with pytest.raises(RuntimeError, match="status -2"):
            Fn.gather_sum(src[:, :H], idx, H, out=buf[:, :H], row0_partial=part, mask=mask, mask_scale=1.25, adds=adds)
    # masked / derived-mask / multi-source sums
    m_h = np.maximum(_src(H, ld, seed=1), 0)               # (NaN pad columns stay NaN)
    buf = fresh()
    Fn.gather_sum_masked(src[:, :H], dev(m_h)[:, :H], 1.0 / 0.9, idx, H, out=buf[:, :H])
    held(buf, R.gather_sum_masked(src_h, m_h, 1.0 / 0.9, idx_h, H), "gather_sum_masked")
    y_h = np.maximum(rng.standard_normal((n_out, H)), 0).astype(np.float32)
    y = _pitched(y_h, ld)[1]
    srcs_h = [_src(H, ld, seed=s) for s in range(3)]
    srcs = [dev(s)[:, :H] for s in srcs_h]
    if vec:
        buf = fresh()
        Fn.gather_sum_dropmask(src[:, :H], y, 1.0 / 0.9, idx, H, 0.1, 77, out=buf[:, :H])
        held(buf, R.gather_sum_dropmask(src_h, y_h, 1.0 / 0.9, idx_h, H, 0.1, 77), "gather_sum_dropmask")
        buf = fresh()
        Fn.gather_sum_multi(srcs, idx, H, out=buf[:, :H])
        held(buf, R.gather_sum_multi(srcs_h, idx_h, H), "gather_sum_multi")
    else:
        buf = fresh()
        with pytest.raises(RuntimeError, match="status -2"):
            Fn.gather_sum_dropmask(src[:, :H], y, 1.0 / 0.9, idx, H, 0.1, 77, out=buf[:, :H])
        arr = (C.c_void_p * 3)(*[t.data_ptr() for t in srcs])
        assert lib().rr_gather_sum_multi_f32(arr, 3, N_SRC, ld, ptr(idx), n_out, K, H, ptr(buf), ld, stream()) == -2
    # difference, dropout copy, CSR sum
    ia, im = _idx(n_out, 1, 5).reshape(-1), _idx(n_out, 1, 6).reshape(-1)
    buf = fresh()
    Fn.gather_diff(src[:, :H], dev(ia), srcs[1], dev(im), H, out=buf[:, :H])
    held(buf, R.gather_diff(src_h, ia, srcs_h[1], im, H), "gather_diff")
    for p in (0.0, 0.1):
        buf = fresh()
        check(lib().rr_gather_dropout_f32(ptr(src), N_SRC, ld, ptr(dev(ia)), n_out, H, p, 99, ptr(buf), ld, stream()), "rr_gather_dropout_f32")
        held(buf, R.gather_dropout(src_h, ia, H, p, 99), f"gather_dropout p={p}")
    offsets, cidx = _csr_table(n_out, rng, big=333)
    buf = fresh()
    _csr_call(src, ld, dev(offsets), dev(cidx), n_out, H, buf, ld)
    held(buf, R.gather_sum_csr(src_h, offsets, cidx, H), "gather_sum_csr")
    torch.cuda.synchronize()
