"""numpy float32 restatement of the gather kernels of csrc/gather.hip, and of the launch arithmetic of their host shells.

The kernels add in table order starting from +0.0 (the two-at-a-time forms - multi, csr - also add sequentially), so a
column-by-column float32 sum in the same order reproduces them BIT FOR BIT, including the `0 + (-0.0) = +0.0` rule their
comments promise.  Only output row 0 of the padding-row forms is a tree sum (a fixed-order reduction of the partial rows);
everything else is compared through int32 views (`same_bits`).  TEST INFRASTRUCTURE: nothing here is on the product path."""
import os
import re

import numpy as np

from oracle import dropout_ref

F32 = np.float32
_COMMON_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reactranker_amd", "csrc", "rr_common.h")


def grid_cap() -> int:
    """RR_GRID_CAP as csrc/rr_common.h defines it (the library does not export it): read from the header so that the
    geometry classes of tests/test_gpu_gather_geometry.py notice when the cap moves instead of silently testing less."""
    src = open(_COMMON_H).read()
    cu = int(re.search(r"^#define\s+RR_NUM_CU\s+(\d+)", src, re.M).group(1))
    per_cu = int(re.search(r"^#define\s+RR_GRID_CAP\s+\(RR_NUM_CU\s*\*\s*(\d+)\)", src, re.M).group(1))
    return cu * per_cu


def vectorised(H, *lds) -> bool:
    """The 16-byte-chunk forms run when the width and every pitch are multiples of four floats (torch allocations are
    16-byte aligned); otherwise the scalar kernels (or RR_ERR_ALIGN, for the entry points that have none)."""
    return H % 4 == 0 and all(ld % 4 == 0 for ld in lds)


def geometry(n_out: int, H: int, vec: bool = True, cap: int = None) -> dict:
    """What rr_grid_for + gather_block_range give a launch over n_out rows of H floats: gather blocks (without the HV
    padding-row blocks), whether the XCD permutation is active (blocks % 8 == 0), chunks per block and the number of
    256-thread passes the busiest thread makes."""
    cap = grid_cap() if cap is None else cap
    HV = H // 4 if vec else H
    total = n_out * HV
    blocks = min(max(1, -(-total // 256)), cap)
    per = -(-total // blocks)
    per = (per + 255) // 256 * 256
    return dict(HV=HV, total=total, blocks=blocks, capped=-(-total // 256) > cap, xcd=blocks % 8 == 0, per=per,
                passes=min(per, total) // 256 + (1 if min(per, total) % 256 else 0), one_workgroup=total <= 256)


def same_bits(got, ref) -> bool:
    got, ref = np.ascontiguousarray(got, F32), np.ascontiguousarray(ref, F32)
    return got.shape == ref.shape and np.array_equal(got.view(np.int32), ref.view(np.int32))


def _rows(src, j, H):
    """src[j, :H] with the zero chunk (+0.0) for j < 0."""
    return np.where((j >= 0)[:, None], src[np.maximum(j, 0), :H], F32(0.0)).astype(F32, copy=False)


def _table(idx):
    idx = np.asarray(idx, np.int32)
    return idx.reshape(idx.shape[0], -1)


def gather_sum(src, idx, H):
    """rr_gather_sum_f32: ((0 + v0) + v1) + ... in table order."""
    idx = _table(idx)
    acc = np.zeros((idx.shape[0], H), F32)
    for k in range(idx.shape[1]):
        acc = acc + _rows(src, idx[:, k], H)
    return acc


def gather_sum_masked(src, mask, scale, idx, H):
    """rr_gather_sum_masked_f32: terms (mask[j] > 0 ? src[j] * scale : 0)."""
    idx = _table(idx)
    acc = np.zeros((idx.shape[0], H), F32)
    for k in range(idx.shape[1]):
        j = idx[:, k]
        v, m = _rows(src, j, H), _rows(mask, j, H)
        acc = acc + np.where(m > 0, v * F32(scale), F32(0.0)).astype(F32)
    return acc


def gather_sum_dropmask(src, y, scale, idx, H, p, seed):
    """rr_gather_sum_dropmask_f32: terms (j >= 0 and kept(j * H + c) and y[r, c] > 0 ? src[j] * scale : 0)."""
    idx = _table(idx)
    acc = np.zeros((idx.shape[0], H), F32)
    cols = np.arange(H, dtype=np.uint64)[None, :]
    for k in range(idx.shape[1]):
        j = idx[:, k]
        elem = np.maximum(j, 0).astype(np.uint64)[:, None] * np.uint64(H) + cols
        keep = dropout_ref.keep_mask(seed, elem, p) if p > 0 else np.ones(elem.shape, bool)
        on = (j >= 0)[:, None] & keep & (y[:, :H] > 0)
        acc = acc + np.where(on, _rows(src, j, H) * F32(scale), F32(0.0)).astype(F32)
    return acc


def gather_sum_multi(srcs, idx, H):
    """rr_gather_sum_multi_f32: per table entry t = ((s0[j] + s1[j]) + s2[j]) + ..., then acc = acc + t in table order."""
    idx = _table(idx)
    acc = np.zeros((idx.shape[0], H), F32)
    for k in range(idx.shape[1]):
        j = idx[:, k]
        t = _rows(srcs[0], j, H)
        for s in srcs[1:]:
            t = t + _rows(s, j, H)
        acc = acc + t
    return acc


def gather_diff(a, ia, m, im, H):
    """rr_gather_diff_f32: a[ia] - m[im], the zero chunk for negative indices."""
    return _rows(a, np.asarray(ia, np.int32), H) - _rows(m, np.asarray(im, np.int32), H)


def keep_scale(p):
    return F32(1.0) / (F32(1.0) - F32(p))


def gather_dropout(src, idx, H, p, seed):
    """rr_gather_dropout_f32: a copy (the sign of -0.0 survives) with the DESTINATION row's keep bits (element r * H + c)."""
    idx = np.asarray(idx, np.int32).reshape(-1)
    v = _rows(src, idx, H)
    if dropout_ref.threshold(p) == 0:
        return v
    elem = np.arange(idx.shape[0], dtype=np.uint64)[:, None] * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :]
    return np.where(dropout_ref.keep_mask(seed, elem, p), v * keep_scale(p), F32(0.0)).astype(F32)


def gather_sum_csr(src, offsets, idx, H):
    """rr_gather_sum_csr_f32: out[r] = ((0 + src[idx[o]]) + src[idx[o + 1]]) + ... over o in [offsets[r], offsets[r + 1])."""
    offsets, idx = np.asarray(offsets, np.int64), np.asarray(idx, np.int64)
    n_out = offsets.shape[0] - 1
    counts = offsets[1:] - offsets[:-1]
    acc = np.zeros((n_out, H), F32)
    for t in range(int(counts.max()) if n_out else 0):
        rows = np.flatnonzero(counts > t)
        acc[rows] = acc[rows] + src[idx[offsets[rows] + t], :H]
    return acc


def epilogue(g, H, mask=None, scale=1.0, adds=()):
    """The fused epilogue of rr_gather_sum_epi_f32 on a gathered tensor g: v = (mask > 0 ? g * scale : 0) (v = g without a
    mask), then (((0 + add_0) + add_1) + ...) + v when there are addends."""
    v = g[:, :H]
    if mask is not None:
        v = np.where(mask[:, :H] > 0, v * F32(scale), F32(0.0)).astype(F32)
    if len(adds) == 0:
        return v
    s = np.zeros_like(v)
    for a in adds:
        s = s + a[:, :H]
    return s + v
