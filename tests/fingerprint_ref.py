"""numpy restatement of the circular fingerprint (csrc/fingerprint.hip) and of the Tanimoto search (csrc/tanimoto.hip); DESIGN.md
section 4l and include/reactranker_hip.h state the definitions.  Section 1 works on uint64 masked to 32 bits with np.add.at /
np.bitwise_xor.at; section 2 counts bits with np.unpackbits, divides in f32 (one correctly rounded division of exact integers,
which is what the kernel's __fdiv_rn does) and orders with np.lexsort on (d, n)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
GOLD = np.uint64(0x9E3779B9)
XOR = np.uint64(0x7F4A7C15)


# ---------------------------------------------------------------------------------------------- 1. the fingerprint
def fmix(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def step(h, w):
    return fmix(((np.asarray(h, np.uint64) ^ np.asarray(w, np.uint64)) + GOLD) & M32)


def f32_bits(v):
    """the f32 patterns as uint64, -0.0 taken as +0.0"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u == np.uint64(0x80000000), np.uint64(0), u)


def rowhash(v):
    """[rows, n] float32 -> [rows] uint64 (32 bits used)"""
    bits = f32_bits(v)
    h = np.zeros(bits.shape[0], np.uint64)
    for c in range(bits.shape[1]):
        h = step(h, bits[:, c])
    return h


def atom_ids(f_atoms, bond_cols, a2b, b2a, radius):
    """ids [radius + 1, nA] uint64 of every atom row of a packed batch (row 0, the padding atom, included: nobody reads it).
    f_atoms [nA, atom_fdim], bond_cols [nB, bond_fdim] (the bond-only columns), a2b [nA, K] incoming bonds (0 = padding),
    b2a [nB] the atom a bond leaves."""
    a2b = np.asarray(a2b, np.int64)
    b2a = np.asarray(b2a, np.int64)
    nA, K = a2b.shape
    ids = np.zeros((radius + 1, nA), np.uint64)
    ids[0] = rowhash(f_atoms)
    bh = rowhash(bond_cols)
    atom = np.repeat(np.arange(nA), K)
    bond = a2b.reshape(-1)
    real = bond != 0
    atom, bond = atom[real], bond[real]
    for r in range(1, radius + 1):
        prev = ids[r - 1]
        m = step(bh[bond], prev[b2a[bond]])
        S = np.zeros(nA, np.uint64)
        X = np.zeros(nA, np.uint64)
        np.add.at(S, atom, m)
        np.bitwise_xor.at(X, atom, fmix(m ^ XOR))
        ids[r] = step(step(step(prev, np.uint64(r)), S & M32), X)
    return ids


def fingerprint_ref(f_atoms, bond_cols, a2b, b2a, a_scope, radius, num_bits):
    """(words [M, num_bits / 32] uint32, counts [M, num_bits] int32)"""
    ids = atom_ids(f_atoms, bond_cols, a2b, b2a, radius)
    scope = np.asarray(a_scope, np.int64).reshape(-1, 2)
    M = scope.shape[0]
    counts = np.zeros((M, num_bits), np.int32)
    for m, (start, size) in enumerate(scope):
        j = (ids[:, start:start + size] % np.uint64(num_bits)).astype(np.int64).reshape(-1)
        np.add.at(counts[m], j, 1)
    return pack_bits_ref(counts > 0), counts


def batch_arrays(batch):
    """(f_atoms, bond_cols, a2b, b2a, a_scope) of a featurization.BatchMolGraph, from its packed host arrays"""
    h = batch._host
    fa, fd = int(h["atom_fdim"]), int(h["bond_fdim"])
    return h["f_atoms"][:, :fa], h["f_bonds"][:, fa:fd], h["a2b"], h["b2a"], h["a_scope"]


def batch_fingerprint_ref(batch, radius, num_bits):
    return fingerprint_ref(*batch_arrays(batch), radius, num_bits)


def pack_bits_ref(on):
    """[M, num_bits] bool -> [M, num_bits / 32] uint32, bit j in word j >> 5 at position j & 31"""
    on = np.asarray(on, bool)
    M, nb = on.shape
    w = on.reshape(M, nb // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return w.sum(axis=2).astype(np.uint32)


def unpack_bits_ref(words):
    words = np.ascontiguousarray(words).view(np.uint32)
    return ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(words.shape[0], -1).astype(bool)


# ---------------------------------------------------------------------------------------------- 2. the search
def popcount_rows(words):
    """[rows, W] uint32 -> [rows] int64"""
    w = np.ascontiguousarray(words).view(np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=1).sum(axis=1).astype(np.int64) if w.shape[1] else np.zeros(len(w), np.int64)


def tanimoto_distances(q, b):
    """d [M, N] float32: (u - c) / u in f32 from exact integers, 0 where u == 0"""
    q = np.ascontiguousarray(q).view(np.uint32)
    b = np.ascontiguousarray(b).view(np.uint32)
    qb = np.unpackbits(q.view(np.uint8), axis=1).astype(np.float32)   # (0/1 sums up to 8192: exact in f32, and a BLAS product)
    bb = np.unpackbits(b.view(np.uint8), axis=1).astype(np.float32)
    c = (qb @ bb.T).astype(np.int64)
    u = popcount_rows(q)[:, None] + popcount_rows(b)[None, :] - c
    num, den = (u - c).astype(np.float32), np.where(u == 0, 1, u).astype(np.float32)
    return np.where(u == 0, np.float32(0), num / den).astype(np.float32)


def excluded(M, N, q_group=None, b_group=None):
    if q_group is None:
        return np.zeros((M, N), bool)
    qg, bg = np.asarray(q_group, np.int64), np.asarray(b_group, np.int64)
    return (qg[:, None] == bg[None, :]) & (qg[:, None] >= 0)


def tanimoto_knn_ref(q, b, k, q_group=None, b_group=None, D=None):
    """(dist [M, k] float32, idx [M, k] int64): d ascending, then n ascending; empty slots +inf / -1.  D: tanimoto_distances(q, b)
    kept from an earlier call"""
    D = tanimoto_distances(q, b) if D is None else D
    M, N = D.shape
    out = excluded(M, N, q_group, b_group)
    dist = np.full((M, k), np.inf, np.float32)
    idx = np.full((M, k), -1, np.int64)
    for m in range(M):
        cand = np.flatnonzero(~out[m])
        order = cand[np.lexsort((cand, D[m, cand]))][:k]
        dist[m, :len(order)] = D[m, order]
        idx[m, :len(order)] = order
    return dist, idx


def tanimoto_count_ref(q, b, radius, q_group=None, b_group=None):
    D = tanimoto_distances(q, b)
    return ((D <= np.float32(radius)) & ~excluded(*D.shape, q_group, b_group)).sum(axis=1).astype(np.int32)
