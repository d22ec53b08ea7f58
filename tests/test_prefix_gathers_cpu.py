"""CPU-side checks of the shared-prefix gathers (rr_gather2_sum_dropmask_f32, rr_gather_sum_dropsrc_f32): the symbols are
declared, exported and bound; each entry refuses bad arguments before any launch; the packer invariant the two-level sum's
padding-row form relies on (the transposed copy table starts with [0, -1, ...] and names copy row 0 nowhere else); and the
numpy restatement of tests/prefix_gathers_ref.py against hand-worked two-row cases."""
import ctypes
import os

import numpy as np

from oracle import dropout_ref
from reactranker_amd import _lib, featurization, synth
from tests import prefix_gathers_ref as P

NEW_SYMBOLS = ["rr_gather2_sum_dropmask_f32", "rr_gather_sum_dropsrc_f32"]
F32 = np.float32


def test_new_symbols_are_declared_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "reactranker_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert f"int {s}(" in header, s
        assert hasattr(raw, s), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert getattr(_lib.lib(), s).argtypes is not None
    assert _lib.lib().rr_version() == _lib.ABI_VERSION == 8          # additive: new symbols only


def _a(l, src=256, in_idx=256, n_mid=4, Ki=2, part=None, n_part=0, ld_part=0, y=256, ld_y=32, out_idx=256, n_out=4, Ko=3, H=32,
       p=0.1, out=256, ld_out=32, ld_src=32):
    v = lambda x: None if x is None else ctypes.c_void_p(x)
    return l.rr_gather2_sum_dropmask_f32(v(src), 8, ld_src, v(in_idx), n_mid, Ki, v(part), n_part, ld_part, v(y), ld_y, v(out_idx),
                                         n_out, Ko, H, p, 7, 1.0, v(out), ld_out, None)


def _b(l, y=256, ld_y=32, cmap=256, idx=256, n_out=4, K=2, H=32, p=0.1, out=256, ld_out=32):
    v = lambda x: None if x is None else ctypes.c_void_p(x)
    return l.rr_gather_sum_dropsrc_f32(v(y), 8, ld_y, v(cmap), 8, v(idx), n_out, K, H, p, 7, v(out), ld_out, None)


def test_entry_points_reject_bad_arguments_before_any_launch():
    l = _lib.lib()
    for null in ("src", "in_idx", "y", "out_idx", "out"):
        assert _a(l, **{null: None}) == -1, null
    assert _a(l, Ki=0) == -1 and _a(l, Ko=0) == -1                   # K < 1
    assert _a(l, ld_src=16) == -1 and _a(l, ld_y=16) == -1 and _a(l, ld_out=16) == -1     # pitch below the width
    assert _a(l, p=1.0) == -1 and _a(l, p=-0.1) == -1
    assert _a(l, H=30) == -2                                         # RR_ERR_ALIGN: H % 4
    assert _a(l, ld_out=34) == -2 and _a(l, ld_src=33) == -2 and _a(l, ld_y=34) == -2    # a pitch that is no whole chunk
    assert _a(l, out=260) == -2 and _a(l, src=264) == -2 and _a(l, y=260) == -2           # misaligned pointers
    assert _a(l, part=256, n_part=1, ld_part=32, n_out=0) == -1      # a padding row of no output
    assert _a(l, part=256, n_part=1, ld_part=16) == -1               # partial pitch below the width
    assert _a(l, part=256, n_part=1, ld_part=34) == -2
    assert _a(l, part=260, n_part=1, ld_part=32) == -2
    assert _a(l, n_out=0) == 0                                       # no rows: nothing launched
    for null in ("y", "cmap", "idx", "out"):
        assert _b(l, **{null: None}) == -1, null
    assert _b(l, K=0) == -1
    assert _b(l, ld_y=16) == -1 and _b(l, ld_out=16) == -1
    assert _b(l, p=1.0) == -1
    assert _b(l, H=30) == -2
    assert _b(l, ld_y=34) == -2 and _b(l, ld_out=33) == -2
    assert _b(l, y=260) == -2 and _b(l, out=264) == -2
    assert _b(l, n_out=0) == 0


def _invariant(batch):
    bmap, bmap_t = batch.unique_bonds()
    assert bmap_t.shape[0] >= 1 and bmap_t[0, 0] == 0 and (bmap_t[0, 1:] == -1).all(), bmap_t[0]
    assert not (bmap_t[1:] == 0).any()
    assert bmap[0] == 0 and (bmap[1:] >= 1).all()


def test_copy_row_zero_is_listed_by_the_first_table_row_only():
    for seed, nq, nc in ((3, 3, [4, 2, 5]), (5, 2, [1, 1]), (9, 1, [7])):
        qb = synth.make_queries(seed, nq, nc, atoms_lo=5, atoms_hi=9)
        _invariant(featurization.BatchMolGraph(qb.r_specs, K=4))
    qb = synth.make_queries(1, 1, [1], atoms_lo=5, atoms_hi=6)
    _invariant(featurization.BatchMolGraph(qb.r_specs[:1], K=4))     # a batch of a single molecule


def test_restatement_against_a_hand_worked_case():
    H = 4
    src = np.array([[1, 2, 3, 4], [10, 20, 30, 40], [-1, -2, -3, -4]], F32)
    in_idx = np.array([[0, 1], [2, -1]], np.int32)                   # intermediate: [11 22 33 44], [-1 -2 -3 -4]
    y = np.array([[1, -1, 0, 2], [1, 1, 1, 1]], F32)
    out_idx = np.array([[0, 1], [1, -1]], np.int32)
    got = P.gather2_sum_dropmask(src, in_idx, y, 2.0, out_idx, H, 0.0, 7)
    assert np.array_equal(got, np.array([[20, 0, 0, 80], [-2, -4, -6, -8]], F32))
    got = P.gather2_sum_dropmask(src, in_idx, y, 2.0, out_idx, H, 0.0, 7, row0=np.full(H, 100, F32))
    assert np.array_equal(got, np.array([[198, 0, 0, 192], [-2, -4, -6, -8]], F32))
    # with dropout: the keep bit of intermediate row j, column c is element j * H + c of the stream
    keep = dropout_ref.keep_mask(7, np.arange(2 * H, dtype=np.uint64).reshape(2, H), 0.5)
    mid = np.array([[11, 22, 33, 44], [-1, -2, -3, -4]], F32)
    want0 = sum(np.where(keep[j] & (y[0] > 0), mid[j] * F32(2.0), F32(0)) for j in (0, 1))
    want1 = np.where(keep[1], mid[1] * F32(2.0), F32(0))
    got = P.gather2_sum_dropmask(src, in_idx, y, 2.0, out_idx, H, 0.5, 7)
    assert np.array_equal(got, np.stack([want0, want1]).astype(F32))

    yb = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], F32)
    copies = np.array([1, 0, 1], np.int32)                           # copies: y[1], y[0], y[1]
    idx = np.array([[0, 1], [2, -1]], np.int32)
    assert np.array_equal(P.gather_sum_dropsrc(yb, copies, idx, H, 0.0, 7), np.array([[6, 8, 10, 12], [5, 6, 7, 8]], F32))
    keep = dropout_ref.keep_mask(11, np.arange(3 * H, dtype=np.uint64).reshape(3, H), 0.5)
    c = [np.where(keep[j], yb[copies[j]] * F32(2.0), F32(0)) for j in range(3)]
    assert np.array_equal(P.gather_sum_dropsrc(yb, copies, idx, H, 0.5, 11), np.stack([c[0] + c[1], c[2]]).astype(F32))
