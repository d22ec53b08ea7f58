"""Circular fingerprints from the packed graph and Tanimoto search on them: structural features and a
structural notion of similarity that need neither RDKit nor a trained model.

The fingerprint is a definition of this library (include/reactranker_hip.h states it; tests/fingerprint_ref.py restates it in
numpy), computed on the GPU from the packed graph the encoder reads.  It is Morgan-STYLE: atom ids are hashed from the atom
features, refined `radius` times over the incoming bonds, and every id of every round sets a bit.  It is NOT bit-compatible with
RDKit's Morgan / ECFP fingerprints (other invariants, another hash, no duplicate-substructure removal), so fingerprints made here
and fingerprints made by RDKit must never be mixed in one bank or one model.

  circular_fingerprint   packed batch -> bit words int32 [n_mols, num_bits / 32] or counts int32 [n_mols, num_bits]
  feature_generate       the reference's feature names -> float32 [n_mols, num_bits], ready for model(..., add_features=)
  unpack_bits/pack_bits  words <-> 0/1 float rows
  reaction_fingerprint   product against reactant: 'difference' (xor: what the reaction changed) or 'concat'
  row_popcount           bits set per row (rr_row_popcount_u32): what the searches take as `bank_popcount`
  tanimoto_knn           the k nearest bank rows under d = 1 - Tanimoto similarity (rr_tanimoto_knn_u32)
  tanimoto_count         bank rows within a Tanimoto distance (rr_tanimoto_count_u32)
  structure_overlap      the structural twin of neighbors.split_overlap: nearest bank row, similarity, identical fingerprints

Bit j of a row is bit j & 31 of word j >> 5; torch has no uint32, so words travel as int32 with the same bits.
There is no CPU path: tensors on the CPU raise."""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import torch

from . import _embed, _lib, featurization
from ._lib import check, lib, ptr, stream

MAX_K = _lib.RR_KNN_MAX_K
MAX_RADIUS = _lib.RR_FP_MAX_RADIUS
MAX_BITS = _lib.RR_FP_MAX_BITS
MAX_WORDS = _lib.RR_TANIMOTO_MAX_WORDS
FEATURE_NAMES = ("binary_morgan_fingerprint", "counts_based_morgan_fingerprint")
REACTION_MODES = ("difference", "concat")


def geometry() -> Tuple[int, int, int, int]:
    """(query rows per workgroup, bank rows per tile, largest k, most words per row) of the compiled library"""
    v = [C.c_int() for _ in range(4)]
    lib().rr_tanimoto_geometry(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


# ------------------------------------------------------------------------------------------------ the fingerprint
def _check_shape(radius, num_bits, who: str) -> Tuple[int, int]:
    r, nb = int(radius), int(num_bits)
    if r != radius or not (0 <= r <= MAX_RADIUS):
        raise ValueError(f"{who}: radius must be an integer in [0, {MAX_RADIUS}] (got {radius!r})")
    if nb != num_bits or nb % 32 != 0 or not (32 <= nb <= MAX_BITS):
        raise ValueError(f"{who}: num_bits must be a multiple of 32 in [32, {MAX_BITS}] (got {num_bits!r})")
    return r, nb


def _fingerprint(batch, radius, num_bits, counts: bool, gpu, who: str) -> torch.Tensor:
    r, nb = _check_shape(radius, num_bits, who)
    if not isinstance(batch, (featurization.BatchMolGraph, featurization.DeviceBatch, featurization.DeviceGraph)):
        raise ValueError(f"{who}: `batch` must be a BatchMolGraph, a DeviceBatch or a DeviceGraph (got {type(batch).__name__})")
    g = featurization.device_graph_of(batch, gpu)
    dev = g.device
    out = torch.empty(g.M, nb if counts else nb // 32, dtype=torch.int32, device=dev)
    if g.M == 0:
        return out
    if g._f_bonds is None:                                 # only the bond columns travel with the batch: read them as they are
        bond, ld_bc = C.c_void_p(g.fbond.data_ptr()), g.fbond.stride(0)
    else:
        bond, ld_bc = C.c_void_p(g._f_bonds.data_ptr() + 4 * g.atom_fdim), g._f_bonds.stride(0)
    with torch.cuda.device(dev):
        ws, nbytes = _embed.scratch("rr_circular_fp_workspace_bytes", dev, g.nA, g.nB)
        check(lib().rr_circular_fp_u32(ptr(g.f_atoms), g.f_atoms.stride(0), g.atom_fdim, bond, ld_bc, g.bond_fdim, ptr(g.a2b),
                                       g.K, ptr(g.b2a), ptr(g.a_scope), g.nA, g.nB, g.M, r, nb,
                                       None if counts else ptr(out), out.stride(0), ptr(out) if counts else None, out.stride(0),
                                       ptr(ws), nbytes, stream()), "rr_circular_fp_u32")
    return out


def circular_fingerprint(batch, radius: int = 2, num_bits: int = 2048, counts: bool = False, gpu=None) -> torch.Tensor:
    """The circular fingerprint of every molecule of a packed batch (a featurization.BatchMolGraph or DeviceBatch), on the GPU.

    counts False: the bit words, int32 [n_mols, num_bits / 32] (bit j of a row = bit j & 31 of word j >> 5); counts True: how
    many (atom, round) pairs fell into each of the num_bits bins, int32 [n_mols, num_bits].  A row depends on its molecule only
    - not on the numbering of its atoms and bonds, its position in the batch or the other molecules - and a molecule without
    atoms gives a zero row.  NOT RDKit's Morgan fingerprint: see the module docstring.
    A DeviceBatch that carries only the bond columns (`fbond`) is read as it is; f_bonds is not materialised for this.
    The call is ordered on the current stream; scratch comes from torch's allocator.
    ValueError - before the library is touched - for a radius outside [0, 8], a num_bits that is not a multiple of 32 in
    [32, 8192], or a batch of another type."""
    return _fingerprint(batch, radius, num_bits, bool(counts), gpu, "circular_fingerprint")


def feature_generate(name: str, batch, radius: int = 2, num_bits: int = 2048, gpu=None) -> torch.Tensor:
    """The reference's feature_generate names on this library's fingerprint: float32 [n_mols, num_bits] on the device, ready for
    model(..., add_features=) with add_features_dim = num_bits.  'binary_morgan_fingerprint' gives 0/1,
    'counts_based_morgan_fingerprint' the counts.  'MACCS_keys_fingerprint' raises: MACCS keys are 166 substructure patterns, and
    matching a substructure needs RDKit, which this library does not have."""
    if name == "MACCS_keys_fingerprint":
        raise ValueError("feature_generate: 'MACCS_keys_fingerprint' is not available: MACCS keys are substructure patterns, and "
                         "substructure matching needs RDKit, which cannot be installed here; use one of " + repr(FEATURE_NAMES))
    if name not in FEATURE_NAMES:
        raise ValueError(f"feature_generate: name must be one of {FEATURE_NAMES} (got {name!r})")
    if name == "binary_morgan_fingerprint":
        return unpack_bits(_fingerprint(batch, radius, num_bits, False, gpu, "feature_generate"))
    return _fingerprint(batch, radius, num_bits, True, gpu, "feature_generate").to(torch.float32)


def unpack_bits(words: torch.Tensor) -> torch.Tensor:
    """int32 words [rows, W] -> float32 0/1 [rows, 32 W] (column j = bit j & 31 of word j >> 5); any device"""
    _embed.word_matrix(words, "words", "unpack_bits", min_width=0)
    shifts = torch.arange(32, dtype=torch.int32, device=words.device)
    return ((words.unsqueeze(-1) >> shifts) & 1).reshape(words.shape[0], -1).to(torch.float32)


def pack_bits(rows: torch.Tensor) -> torch.Tensor:
    """0/1 rows [rows, num_bits] (non-zero = set; num_bits a multiple of 32) -> int32 words [rows, num_bits / 32]"""
    if not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[1] % 32 != 0:
        got = f"of shape {tuple(rows.shape)}" if torch.is_tensor(rows) else type(rows).__name__
        raise ValueError(f"pack_bits: `rows` must be a matrix [rows, num_bits] with num_bits a multiple of 32 (got {got})")
    on = (rows != 0).reshape(rows.shape[0], -1, 32).to(torch.int64)
    v = (on << torch.arange(32, dtype=torch.int64, device=rows.device)).sum(dim=-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def reaction_fingerprint(r_batch, p_batch, radius: int = 2, num_bits: int = 2048, mode: str = "difference", gpu=None) -> torch.Tensor:
    """One row of bit words per reaction from the reactant and the product batch (molecule i of one belongs to molecule i of
    the other).  mode 'difference': the xor of the two bitsets, int32 [n, num_bits / 32] - the substructures the reaction made or
    destroyed; 'concat': [reactant | product], int32 [n, 2 num_bits / 32]."""
    if mode not in REACTION_MODES:
        raise ValueError(f"reaction_fingerprint: mode must be one of {REACTION_MODES} (got {mode!r})")
    r = _fingerprint(r_batch, radius, num_bits, False, gpu, "reaction_fingerprint")
    p = _fingerprint(p_batch, radius, num_bits, False, gpu, "reaction_fingerprint")
    if r.shape != p.shape:
        raise ValueError(f"reaction_fingerprint: {r.shape[0]} reactants for {p.shape[0]} products")
    return torch.bitwise_xor(r, p) if mode == "difference" else torch.cat([r, p], dim=1)


# ------------------------------------------------------------------------------------------------ the search
def row_popcount(x: torch.Tensor) -> torch.Tensor:
    """bits set per row of int32 words [rows, W]: int32 [rows] (rr_row_popcount_u32) - what the searches take as `bank_popcount`"""
    x = _embed.word_rows(x, "x", "row_popcount")
    out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    if x.shape[0] == 0:
        return out
    with torch.cuda.device(x.device):
        check(lib().rr_row_popcount_u32(ptr(x), _embed.pitch(x), x.shape[0], x.shape[1], ptr(out), stream()), "rr_row_popcount_u32")
    return out


def _search_args(queries, bank, q_group, b_group, bank_popcount, who: str):
    """the checks both searches share -> (q, b, M, N, W, dev, qg, bg, bp); an empty bank is replaced by a placeholder row"""
    if (q_group is None) != (b_group is None):
        raise ValueError(f"{who}: q_group and b_group go together (both or neither)")
    _embed.word_matrix(queries, "queries", who, max_width=MAX_WORDS)
    _embed.word_matrix(bank, "bank", who, max_width=MAX_WORDS)
    q = _embed.word_rows(queries, "queries", who, max_width=MAX_WORDS)
    b = _embed.word_rows(bank, "bank", who, max_width=MAX_WORDS)
    if q.shape[1] != b.shape[1]:
        raise ValueError(f"{who}: queries have {q.shape[1]} words per row, the bank {b.shape[1]}")
    if q.device != b.device:
        raise ValueError(f"{who}: queries on {q.device}, bank on {b.device}")
    M, N, W, dev = q.shape[0], b.shape[0], q.shape[1], q.device
    if max(M, N) > 2 ** 31 - 1:
        raise ValueError(f"{who}: {max(M, N)} rows (at most 2^31 - 1)")
    qg = bg = None
    if q_group is not None:
        qg, bg = _embed.group(q_group, M, dev, "q_group", who), _embed.group(b_group, N, dev, "b_group", who)
    bp = None if bank_popcount is None else _embed.per_row(bank_popcount, N, None, "bank_popcount", who, dtype=torch.int32)
    if N == 0:                                             # (the C entries want a bank pointer even when it holds no row)
        b, bg = _embed.empty_bank(W, dev, bg is not None, dtype=torch.int32)
        bp = None
    return q, b, M, N, W, dev, qg, bg, bp


def tanimoto_knn(queries: torch.Tensor, bank: torch.Tensor, k: int, q_group=None, b_group=None,
                 bank_popcount=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k nearest bank rows of every query row under the Tanimoto distance: (dist [M, k] float32 ascending, idx [M, k] int64).

    With c = popcount(q & b) and u = |q| + |b| - c: dist = (u - c) / u, one f32 division of exact integers (0 when both rows are
    empty), i.e. 1 - Tanimoto similarity.  Ties go to the lower bank index.  A pair is excluded when q_group[m] == b_group[n] >= 0
    (both or neither given).  When fewer than k rows qualify the remaining slots hold dist = +inf, idx = -1; an empty bank is
    allowed.  bank_popcount: row_popcount(bank) kept from an earlier call.  Rows are int32 words [rows, W], W <= 256, with
    contiguous rows at any pitch.  The call is ordered on the current stream.
    ValueError - before any launch - for CPU tensors, another dtype, k outside [1, 64], widths that differ or one group array
    without the other."""
    who = "tanimoto_knn"
    kk = int(k)
    if kk != k or not (1 <= kk <= MAX_K):
        raise ValueError(f"{who}: k must be an integer in [1, {MAX_K}] (got {k!r})")
    q, b, M, N, W, dev, qg, bg, bp = _search_args(queries, bank, q_group, b_group, bank_popcount, who)
    dist = torch.empty(M, kk, dtype=torch.float32, device=dev)
    idx = torch.empty(M, kk, dtype=torch.int32, device=dev)
    if M == 0:
        return dist, idx.to(torch.int64)
    with torch.cuda.device(dev):
        ws, nbytes = _embed.scratch("rr_tanimoto_knn_workspace_bytes", dev, M, N, kk)
        check(lib().rr_tanimoto_knn_u32(ptr(q), _embed.pitch(q), M, ptr(b), _embed.pitch(b), N, W, kk, ptr(qg), ptr(bg), ptr(bp),
                                        ptr(dist), ptr(idx), ptr(ws), nbytes, stream()), "rr_tanimoto_knn_u32")
    return dist, idx.to(torch.int64)


def tanimoto_count(queries: torch.Tensor, bank: torch.Tensor, radius, q_group=None, b_group=None,
                   bank_popcount=None) -> torch.Tensor:
    """How many bank rows lie within the Tanimoto distance `radius` of every query row: int64 [M].  count[m] = #{n : dist(m, n)
    <= float32(radius), (m, n) not excluded}, dist and the exclusion as in tanimoto_knn, bit for bit (radius 0.25 counts the
    rows with a similarity of at least 0.75).  ValueError for a radius that is negative or a NaN, and for what tanimoto_knn
    rejects."""
    who = "tanimoto_count"
    rad = float(radius)
    if not rad >= 0.0:
        raise ValueError(f"{who}: radius must be >= 0 (got {radius!r})")
    q, b, M, N, W, dev, qg, bg, bp = _search_args(queries, bank, q_group, b_group, bank_popcount, who)
    count = torch.empty(M, dtype=torch.int32, device=dev)
    if M == 0:
        return count.to(torch.int64)
    with torch.cuda.device(dev):
        ws, nbytes = _embed.scratch("rr_tanimoto_count_workspace_bytes", dev, M, N)
        check(lib().rr_tanimoto_count_u32(ptr(q), _embed.pitch(q), M, ptr(b), _embed.pitch(b), N, W, C.c_float(rad), ptr(qg),
                                          ptr(bg), ptr(bp), ptr(count), ptr(ws), nbytes, stream()), "rr_tanimoto_count_u32")
    return count.to(torch.int64)


def structure_overlap(bank_bits: torch.Tensor, bits: torch.Tensor, bank_popcount=None) -> dict:
    """Structural leakage between a bank of fingerprints and another split, before any model exists: dict(count, rows [count]
    int64, nearest [M] int64, similarity [M] float32) - every row's nearest bank row (-1 for an empty bank) and its Tanimoto
    similarity 1 - dist (-inf for an empty bank), and `rows`, the rows of `bits` whose nearest bank row has the identical
    fingerprint (dist == 0: exact, the distance is a ratio of integers).  The structural twin of neighbors.split_overlap."""
    dist, idx = tanimoto_knn(bits, bank_bits, 1, bank_popcount=bank_popcount)
    dist, idx = dist[:, 0], idx[:, 0]
    rows = ((idx >= 0) & (dist == 0)).nonzero().reshape(-1)
    return dict(count=int(rows.numel()), rows=rows, nearest=idx, similarity=1.0 - dist)
