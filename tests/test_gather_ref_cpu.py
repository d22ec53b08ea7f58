"""The numpy restatement the GPU gather tests compare with (tests/gather_ref.py) must itself be right: here it is held against
float64 sums, against torch's index_add, and its launch arithmetic against hand-worked cases.  No GPU."""
import numpy as np
import torch

from oracle import dropout_ref
from tests import gather_ref as R


def _data(H=12, n_src=50, n_out=40, K=5, seed=0):
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((n_src, H)).astype(np.float32)
    idx = rng.integers(-1, n_src, size=(n_out, K)).astype(np.int32)
    idx[0] = -1
    return rng, src, idx


def test_sums_match_float64_and_turn_negative_zero_sums_into_positive_zero():
    rng, src, idx = _data()
    src[3] = -0.0
    idx[1] = 3
    want = np.where(idx[..., None] >= 0, src[np.maximum(idx, 0)].astype(np.float64), 0).sum(1)
    got = R.gather_sum(src, idx, 12)
    assert got.dtype == np.float32 and np.abs(got - want).max() < 1e-6
    assert not np.signbit(got[0]).any() and not np.signbit(got[1]).any()
    assert R.same_bits(R.gather_sum_multi([src], idx, 12), got)
    assert not R.same_bits(np.float32([-0.0]), np.float32([0.0])) and R.same_bits(np.float32([np.nan]), np.float32([np.nan]))
    mask = np.maximum(rng.standard_normal(src.shape), 0).astype(np.float32)
    masked = np.where(mask > 0, src * np.float32(1.25), 0).astype(np.float32)
    assert R.same_bits(R.gather_sum_masked(src, mask, 1.25, idx, 12), R.gather_sum(masked, idx, 12))
    three = [src, mask, masked]
    want = np.where(idx[..., None] >= 0, sum(t.astype(np.float64) for t in three)[np.maximum(idx, 0)], 0).sum(1)
    assert np.abs(R.gather_sum_multi(three, idx, 12) - want).max() < 2e-6
    ia, im = idx[:, 0], idx[:, 1]
    assert R.same_bits(R.gather_diff(src, ia, mask, im, 12),
                       np.where(ia[:, None] >= 0, src[np.maximum(ia, 0)], 0) - np.where(im[:, None] >= 0, mask[np.maximum(im, 0)], 0))


def test_dropout_forms_use_the_stream_elements_the_kernels_use():
    rng, src, idx = _data(H=8)
    seed, p = 0xABCDEF, 0.3
    owner = rng.integers(-1, 50, size=40).astype(np.int32)
    owner[2] = 3
    src[3] = -0.0
    full = R.gather_dropout(src, owner, 8, p, seed)
    keep = dropout_ref.keep_mask(seed, np.arange(40 * 8, dtype=np.uint64), p).reshape(40, 8)
    assert np.array_equal(full != 0, keep & (owner >= 0)[:, None] & (src[np.maximum(owner, 0)] != 0))
    assert np.signbit(R.gather_dropout(src, owner, 8, 0.0, seed)[2]).all()          # a copy keeps -0.0
    # the derived mask = the materialised one: copies of y rows, each with its own keep bits
    y = np.maximum(rng.standard_normal((10, 8)), 0).astype(np.float32)
    own = rng.integers(0, 10, size=50).astype(np.int32)
    copies = R.gather_dropout(y, own, 8, p, seed)
    table = np.full((10, 50), -1, np.int32)
    for j, u in enumerate(own):
        table[u, np.argmax(table[u] < 0)] = j
    assert R.same_bits(R.gather_sum_dropmask(src, y, 1.5, table, 8, p, seed), R.gather_sum_masked(src, copies, 1.5, table, 8))


def test_csr_sum_is_index_add_and_the_epilogue_is_relu_backward_plus_addends():
    rng, src, _ = _data()
    counts = np.array([0, 1, 2, 3, 4, 37, 0])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    idx = rng.integers(0, 50, size=int(offsets[-1])).astype(np.int32)
    got = R.gather_sum_csr(src, offsets, idx, 12)
    want = torch.zeros(7, 12, dtype=torch.float64).index_add_(0, torch.tensor(np.repeat(np.arange(7), counts)), torch.tensor(src[idx]).double())
    assert np.abs(got - want.numpy()).max() < 1e-5 and np.abs(got[0]).max() == 0 and np.abs(got[-1]).max() == 0
    g = src[:7]
    mask = np.maximum(rng.standard_normal((7, 12)), 0).astype(np.float32)
    adds = [rng.standard_normal((7, 12)).astype(np.float32) for _ in range(3)]
    want = ((adds[0] + adds[1]) + adds[2]) + np.where(mask > 0, g * np.float32(0.5), 0).astype(np.float32)
    assert R.same_bits(R.epilogue(g, 12, mask, 0.5, adds), want)
    assert R.same_bits(R.epilogue(g, 12), g)


def test_launch_arithmetic():
    cap = R.grid_cap()
    assert cap == 8192                                     # RR_NUM_CU * 32 (csrc/rr_common.h); the capped cases below depend on it
    g = R.geometry(977, 300)
    assert (g["HV"], g["blocks"], g["xcd"], g["passes"], g["capped"]) == (75, 287, False, 1, False)
    g = R.geometry(7179, 300)
    assert (g["blocks"], g["xcd"], g["passes"]) == (2104, True, 1)
    g = R.geometry(30011, 300)
    assert (g["blocks"], g["capped"], g["per"], g["passes"]) == (cap, True, 512, 2)
    g = R.geometry(977, 30, vec=False)
    assert (g["HV"], g["blocks"]) == (30, 115)
    assert R.geometry(3, 32)["one_workgroup"] and R.geometry(8200, 1028)["HV"] == 257
    assert R.vectorised(300, 304) and not R.vectorised(30, 32) and not R.vectorised(300, 301)
