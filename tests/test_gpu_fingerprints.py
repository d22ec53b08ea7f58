"""Circular fingerprints and Tanimoto search on the GPU (reactranker_amd.fingerprints; rr_circular_fp_u32, rr_tanimoto_knn_u32,
rr_tanimoto_count_u32, rr_row_popcount_u32) against the numpy restatement of tests/fingerprint_ref.py.

Every comparison is on integers or on bit-exact f32 (the Tanimoto distance is one correctly rounded division of exact integers),
so there are no tolerances: words, counts, distance bits and indices are compared for equality."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from reactranker_amd import _lib, featurization, synth
from reactranker_amd import fingerprints as FP
from reactranker_amd.base_model import build_model
from oracle import ref_cpu as O
from tests import fingerprint_ref as R
from tests import poison, streams

pytestmark = pytest.mark.gpu

RT, BT, MAXK, MAXW = FP.geometry()
STAGE = 256                                                           # atoms of a molecule whose ids stay on chip (csrc/fingerprint.hip)


def words_of(t):
    return t.cpu().numpy().view(np.uint32)


def dev_words(w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int32)).cuda()


def gpu_fp(batch, radius, num_bits):
    bits = FP.circular_fingerprint(batch, radius, num_bits, gpu=0)
    counts = FP.circular_fingerprint(batch, radius, num_bits, counts=True, gpu=0)
    torch.cuda.synchronize()
    assert bits.dtype == counts.dtype == torch.int32
    assert tuple(bits.shape) == (batch.n_mols, num_bits // 32) and tuple(counts.shape) == (batch.n_mols, num_bits)
    return words_of(bits), counts.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. the fingerprint
@functools.lru_cache(maxsize=None)
def query_batch():
    qb = synth.make_queries(17, 6, 6)                                 # 36 products of 10 - 24 atoms
    return featurization.BatchMolGraph(qb.p_specs)


@functools.lru_cache(maxsize=None)
def query_ids(radius):
    fa, bc, a2b, b2a, scope = R.batch_arrays(query_batch())
    return R.atom_ids(fa, bc, a2b, b2a, radius), scope


def ref_from_ids(ids, scope, num_bits):
    counts = np.zeros((len(scope), num_bits), np.int32)
    for m, (start, size) in enumerate(scope):
        np.add.at(counts[m], (ids[:, start:start + size] % np.uint64(num_bits)).astype(np.int64).reshape(-1), 1)
    return R.pack_bits_ref(counts > 0), counts


@pytest.mark.parametrize("num_bits", [32, 64, 2048, 8192])
@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_fingerprint_equals_the_reference_in_both_forms(radius, num_bits, parity_log):
    batch = query_batch()
    ids, scope = query_ids(radius)
    want_w, want_c = ref_from_ids(ids, scope, num_bits)
    got_w, got_c = gpu_fp(batch, radius, num_bits)
    parity_log(f"radius {radius}, {num_bits} bits, {batch.n_mols} molecules: {int((got_w != want_w).sum())} words and "
               f"{int((got_c != want_c).sum())} bins differ; bits set per row {R.popcount_rows(want_w).mean():.1f} of "
               f"{want_c.sum(axis=1).mean():.1f} features")
    assert np.array_equal(got_w, want_w) and np.array_equal(got_c, want_c)
    assert (want_c.sum(axis=1) == (radius + 1) * scope[:, 1]).all()
    if num_bits == 32:
        assert (want_c > 1).any()                                     # collisions: the bitset and the counts say different things


def _spec(n, edges, rng):
    e = np.array(sorted(edges), np.int32).reshape(-1, 2)
    return synth.MolSpec(n, synth._atom_features(rng, n), e, synth._bond_features(rng, len(e)))


@functools.lru_cache(maxsize=None)
def odd_specs():
    rng = np.random.default_rng(23)
    single = _spec(1, [], rng)
    star = _spec(7, [(0, j) for j in range(1, 7)], rng)               # atom 0 has the batch's maximum degree
    big = synth.random_reactant(rng, 65)                              # more atoms than a wavefront has lanes
    chain = _spec(1600, [(j, j + 1) for j in range(1599)], rng)       # more atoms than stay on chip
    empty = synth.MolSpec(0, np.zeros((0, synth.ATOM_FDIM), np.float32), np.zeros((0, 2), np.int32),
                          np.zeros((0, synth.BOND_FDIM), np.float32))
    edge = _spec(STAGE, [(j, j + 1) for j in range(STAGE - 1)], rng)  # the largest molecule that stays on chip, and one more atom
    over = _spec(STAGE + 1, [(j, j + 1) for j in range(STAGE)], rng)
    small = synth.random_reactant(rng, 12)
    return dict(single=single, star=star, big=big, chain=chain, empty=empty, edge=edge, over=over, small=small)


def test_shapes_that_can_break_the_kernel(parity_log):
    s = odd_specs()
    assert s["chain"].n_atoms >= 1500 > STAGE
    order = ["single", "chain", "star", "empty", "big", "edge", "over", "small", "empty", "single"]
    batch = featurization.BatchMolGraph([s[k] for k in order])
    assert batch.max_num_bonds == 6 and batch._host["a_scope"][3, 1] == 0
    for radius, num_bits in ((2, 2048), (3, 64), (8, 8192)):
        want_w, want_c = R.batch_fingerprint_ref(batch, radius, num_bits)
        got_w, got_c = gpu_fp(batch, radius, num_bits)
        assert np.array_equal(got_w, want_w) and np.array_equal(got_c, want_c), (radius, num_bits)
        assert not got_w[3].any() and not got_c[8].any()              # a molecule without atoms: a zero row
        assert got_c[0].sum() == radius + 1 and got_c[1].sum() == 1600 * (radius + 1)
        assert np.array_equal(got_c[0], got_c[9])
        parity_log(f"radius {radius}, {num_bits} bits: the chain of 1600 sets {R.popcount_rows(got_w)[1]} bits, 0 words differ")


def test_negative_zero_hashes_as_zero():
    s = odd_specs()["small"]
    fa = s.f_atoms.copy()
    zeros = np.argwhere(fa == 0)
    assert len(zeros) > 10
    for a, c in zeros[::3]:
        fa[a, c] = -0.0
    fb = s.f_bond.copy()
    fb[fb == 0] = -0.0
    assert np.signbit(fa).any() and np.signbit(fb).any()
    neg = featurization.BatchMolGraph([synth.MolSpec(s.n_atoms, fa, s.edges, fb)])
    assert np.signbit(neg._host["f_atoms"]).any() and np.signbit(neg._host["f_bonds"]).any()
    a, b = gpu_fp(neg, 2, 2048), gpu_fp(featurization.BatchMolGraph([s]), 2, 2048)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    want = R.batch_fingerprint_ref(neg, 2, 2048)
    assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1])


def _fbond_only(batch, pitch):
    """a DeviceBatch over `batch`'s device tensors that carries the bond-only columns (at `pitch` floats per row), no f_bonds"""
    g = batch.device_graph(0)
    tensors = {k: getattr(g, k) for k in featurization._GRAPH_KEYS}
    wide = torch.full((g.nB, pitch), float("nan"), device=g.device)
    wide[:, :g.bond_fdim] = g._f_bonds[:, g.atom_fdim:g.atom_fdim + g.bond_fdim]
    tensors["fbond"] = wide[:, :g.bond_fdim]
    dg = featurization.DeviceGraph.from_device(tensors, g.nA, g.nB, g.K, g.M, g.device, g.atom_fdim, g.bond_fdim)
    return featurization.DeviceBatch(dg), dg


@pytest.mark.parametrize("pitch", [22, 24, 27])                        # 4-byte loads, 16-byte loads, 4-byte loads with a pad
def test_device_batch_that_carries_only_the_bond_columns(pitch):
    batch = query_batch()
    db, dg = _fbond_only(batch, pitch)
    want = gpu_fp(batch, 2, 2048)
    bits = FP.circular_fingerprint(db, 2, 2048)
    counts = FP.circular_fingerprint(db, 2, 2048, counts=True)
    assert dg._f_bonds is None                                        # f_bonds was not materialised for this
    assert np.array_equal(words_of(bits), want[0]) and np.array_equal(counts.cpu().numpy(), want[1])


def _renumbered(spec, rng):
    n = spec.n_atoms
    new_of_old = rng.permutation(n)
    e = np.sort(new_of_old[spec.edges.astype(np.int64)], axis=1)
    order = np.lexsort((e[:, 1], e[:, 0]))
    return synth.MolSpec(n, spec.f_atoms[np.argsort(new_of_old)], e[order].astype(np.int32), spec.f_bond[order], spec.smiles)


def test_renumbered_atoms_and_bonds_give_identical_rows():
    rng = np.random.default_rng(29)
    s = odd_specs()
    specs = [s["small"], s["big"], s["star"], s["over"]] + synth.make_queries(31, 4, 1).p_specs
    perm = [_renumbered(x, rng) for x in specs]
    for radius in (1, 3):
        a = gpu_fp(featurization.BatchMolGraph(specs), radius, 2048)
        b = gpu_fp(featurization.BatchMolGraph(perm), radius, 2048)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_row_is_the_same_alone_first_or_last_in_a_batch():
    s = odd_specs()
    others = synth.make_queries(37, 5, 1).p_specs
    for key in ("small", "over"):
        alone = gpu_fp(featurization.BatchMolGraph([s[key]]), 2, 2048)
        first = gpu_fp(featurization.BatchMolGraph([s[key]] + others), 2, 2048)
        last = gpu_fp(featurization.BatchMolGraph(others + [s["chain"], s[key]]), 2, 2048)
        for f in (0, 1):
            assert np.array_equal(alone[f][0], first[f][0]) and np.array_equal(alone[f][0], last[f][-1]), key


def test_reaction_fingerprint_and_feature_generate():
    qb = synth.make_queries(41, 3, 4)
    rb, pb = featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs)
    r, p = R.batch_fingerprint_ref(rb, 2, 256), R.batch_fingerprint_ref(pb, 2, 256)
    diff = FP.reaction_fingerprint(rb, pb, 2, 256, gpu=0)
    cat = FP.reaction_fingerprint(rb, pb, 2, 256, mode="concat", gpu=0)
    assert np.array_equal(words_of(diff), r[0] ^ p[0]) and np.array_equal(words_of(cat), np.concatenate([r[0], p[0]], axis=1))
    assert (R.popcount_rows(r[0] ^ p[0]) > 0).all()                   # every product differs from its reactant
    binary = FP.feature_generate("binary_morgan_fingerprint", pb, 2, 256, gpu=0)
    cnt = FP.feature_generate("counts_based_morgan_fingerprint", pb, 2, 256, gpu=0)
    assert binary.dtype == cnt.dtype == torch.float32 and binary.is_cuda and tuple(binary.shape) == tuple(cnt.shape) == (12, 256)
    assert np.array_equal(binary.cpu().numpy(), (p[1] > 0).astype(np.float32)) and np.array_equal(cnt.cpu().numpy(), p[1])
    assert torch.equal(FP.pack_bits(binary), FP.circular_fingerprint(pb, 2, 256, gpu=0))
    assert torch.equal(FP.row_popcount(FP.pack_bits(binary)).cpu(), torch.from_numpy(R.popcount_rows(p[0])).to(torch.int32))


def test_c_entry_limits_launch_nothing():
    g = query_batch().device_graph(0)
    out = torch.zeros(g.M, 512, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")

    def call(radius, num_bits, bits=True, nbytes=1 << 20):
        return _lib.lib().rr_circular_fp_u32(
            _lib.ptr(g.f_atoms), g.f_atoms.stride(0), g.atom_fdim, C.c_void_p(g._f_bonds.data_ptr() + 4 * g.atom_fdim),
            g._f_bonds.stride(0), g.bond_fdim, _lib.ptr(g.a2b), g.K, _lib.ptr(g.b2a), _lib.ptr(g.a_scope), g.nA, g.nB, g.M,
            radius, num_bits, _lib.ptr(out) if bits else None, 512, None, 0, _lib.ptr(ws), C.c_size_t(nbytes), _lib.stream())
    assert call(2, 64) == 0
    assert call(-1, 64) == -1 and call(2, 48) == -1 and call(2, 0) == -1 and call(2, 64, bits=False) == -1
    assert call(9, 64) == -4 and call(2, 8224) == -4 and call(2, 64, nbytes=16) == -5
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. the search
def bit_rows(rng, rows, W, density):
    """random words of the given bit density (a number, or one per row)"""
    d = np.broadcast_to(np.asarray(density, np.float64).reshape(-1, 1), (rows, 1))
    return R.pack_bits_ref(rng.random((rows, 32 * W)) < d)


def search_case(seed, M, N, W):
    """queries and bank with every density from empty to full, all-zero rows on both sides and planted duplicates"""
    rng = np.random.default_rng(seed)
    q = bit_rows(rng, M, W, rng.choice([0.05, 0.2, 0.5, 0.9], M))
    b = bit_rows(rng, N, W, rng.choice([0.05, 0.2, 0.5, 0.9], N)) if N else np.zeros((0, W), np.uint32)
    q[::7] = 0
    if N:
        b[3 % N::11] = 0
        for j in range(min(9, N)):
            b[(7 * j + 5) % N] = q[(5 * j + 1) % M]
    return q, b


def run_knn(q, b, k, **kw):
    kw = {key: (torch.from_numpy(np.asarray(v, np.int32)).cuda() if v is not None else None) for key, v in kw.items()}
    d, i = FP.tanimoto_knn(dev_words(q), dev_words(b), k, **kw)
    torch.cuda.synchronize()
    assert d.dtype == torch.float32 and i.dtype == torch.int64 and tuple(d.shape) == tuple(i.shape) == (len(q), k)
    return d.cpu().numpy(), i.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class splits:
    def __init__(self, s):
        self.s = s

    def __enter__(self):
        assert _lib.lib().rr_tanimoto_set_splits(self.s) == 0

    def __exit__(self, *a):
        assert _lib.lib().rr_tanimoto_set_splits(0) == 0


BANKS = (0, 1, BT - 1, BT, 8 * BT + 76)


@pytest.mark.parametrize("W", [1, 2, 3, 64, 256])                      # 3: not a multiple of four words, the 4-byte loads
def test_knn_equals_the_reference_bit_for_bit(W, parity_log):
    ties = cut_ties = cases = 0
    for M in (1, RT - 1, RT + 6):
        for N in BANKS:
            q, b = search_case(100 * W + M + N, M, N, W)
            D = R.tanimoto_distances(q, b)
            for k in (1, 5, 64):
                want_d, want_i = R.tanimoto_knn_ref(q, b, k, D=D)
                got_d, got_i = run_knn(q, b, k)
                assert np.array_equal(got_i, want_i), (M, N, k)
                assert same_bits(got_d, want_d), (M, N, k)
                cases += 1
                if N > k:
                    srt = np.sort(D, axis=1)
                    cut_ties += int((srt[:, k - 1] == srt[:, k]).sum())
            if N > 1:
                ties += int((np.diff(np.sort(D, axis=1), axis=1) == 0).sum())
            if N >= BT:
                assert (D == 0).any() and (D == 1).any()                  # a planted duplicate or two empty rows; disjoint rows
    parity_log(f"W {W}: {cases} searches, dist bits and idx equal; {ties} tied neighbours in the sorted rows, "
               f"{cut_ties} rows whose k-th and (k+1)-th distance tie")
    if W == 1:
        assert cut_ties > 100                                         # 32-bit rows: the index tie-break carries the test


def test_group_exclusion_against_the_reference():
    q, b = search_case(7, RT + 6, 5 * BT + 60, 2)
    M, N = len(q), len(b)
    qg = (np.arange(M) % 8).astype(np.int32)
    for bg in ((np.arange(N) // 100).astype(np.int32), (np.arange(N) // (2 * BT)).astype(np.int32)):
        want_d, want_i = R.tanimoto_knn_ref(q, b, 7, qg, bg)
        for s in (0, 3):
            with splits(s):
                got_d, got_i = run_knn(q, b, 7, q_group=qg, b_group=bg)
            assert np.array_equal(got_i, want_i) and same_bits(got_d, want_d)
    bg = np.full(N, 5, np.int32)                                      # everything excluded for one query, negative ids match nothing
    bg[:3] = -1
    qg3 = np.array([5, 1, -1], np.int32)
    want_d, want_i = R.tanimoto_knn_ref(q[:3], b, 4, qg3, bg)
    got_d, got_i = run_knn(q[:3], b, 4, q_group=qg3, b_group=bg)
    assert np.array_equal(got_i, want_i) and same_bits(got_d, want_d)
    assert want_i[0, 3] == -1 and set(want_i[0, :3].tolist()) == {0, 1, 2}
    g = np.arange(N, dtype=np.int32)                                  # leave-one-out of a bank against itself
    want_d, want_i = R.tanimoto_knn_ref(b, b, 3, g, g)
    got_d, got_i = run_knn(b, b, 3, q_group=g, b_group=g)
    assert np.array_equal(got_i, want_i) and same_bits(got_d, want_d) and not (got_i == np.arange(N)[:, None]).any()


def test_splits_pitch_alignment_and_position_do_not_show():
    W, k = 6, 16
    q, b = search_case(9, RT + 6, 8 * BT + 76, W)
    tq, tb = dev_words(q), dev_words(b)
    base = FP.tanimoto_knn(tq, tb, k)
    want_d, want_i = R.tanimoto_knn_ref(q, b, k)
    assert np.array_equal(base[1].cpu().numpy(), want_i) and same_bits(base[0].cpu().numpy(), want_d)
    radius = 0.75
    base_c = FP.tanimoto_count(tq, tb, radius)
    assert np.array_equal(base_c.cpu().numpy(), R.tanimoto_count_ref(q, b, radius))

    def same(got, got_c, what):
        assert torch.equal(got[0].view(torch.int32), base[0].view(torch.int32)) and torch.equal(got[1], base[1]), what
        assert torch.equal(got_c, base_c), what
    for s in (1, 2, 7):
        with splits(s):
            assert _lib.lib().rr_tanimoto_splits() == s
            same(FP.tanimoto_knn(tq, tb, k), FP.tanimoto_count(tq, tb, radius), f"{s} splits")
    assert _lib.lib().rr_tanimoto_splits() == 0
    # row views with an odd pitch (the pad words are all ones: they never reach a result) and a misaligned base
    for pitch in (W + 1, W + 2, W + 5):                               # 7: 4-byte loads; 8: 16-byte loads; 11: 4-byte loads
        wide = torch.full((len(b), pitch), -1, dtype=torch.int32, device="cuda")
        wide[:, :W] = tb
        wq = torch.full((len(q), pitch), -1, dtype=torch.int32, device="cuda")
        wq[:, :W] = tq
        same(FP.tanimoto_knn(wq[:, :W], wide[:, :W], k), FP.tanimoto_count(wq[:, :W], wide[:, :W], radius), f"pitch {pitch}")
        assert torch.equal(FP.row_popcount(wide[:, :W]), FP.row_popcount(tb))
    flat = torch.full((len(b) * 8 + 1,), -1, dtype=torch.int32, device="cuda")
    off = flat[1:].view(len(b), 8)
    off[:, :W] = tb
    assert off.data_ptr() % 16 == 4
    same(FP.tanimoto_knn(tq, off[:, :W], k), FP.tanimoto_count(tq, off[:, :W], radius), "misaligned base")
    bp = FP.row_popcount(off[:, :W])
    assert bp.dtype == torch.int32 and np.array_equal(bp.cpu().numpy(), R.popcount_rows(b))
    same(FP.tanimoto_knn(tq, off[:, :W], k, bank_popcount=bp), FP.tanimoto_count(tq, off[:, :W], radius, bank_popcount=bp),
         "bank_popcount given")
    # the same query rows at other positions of a larger M
    rng = np.random.default_rng(10)
    big = dev_words(bit_rows(rng, 3 * RT + 9, W, 0.3))
    pos = torch.from_numpy(rng.permutation(big.shape[0])[:len(q)]).cuda()
    big[pos] = tq
    got, got_c = FP.tanimoto_knn(big, tb, k), FP.tanimoto_count(big, tb, radius)
    same((got[0][pos], got[1][pos]), got_c[pos], "position")


@pytest.mark.parametrize("W", [1, 3, 64, 256])
def test_count_equals_the_reference_at_radii_that_sit_on_a_similarity(W, parity_log):
    q, b = search_case(50 + W, RT + 6, 3 * BT + 5, W)
    q[1], b[0], b[1], b[2] = 0, 0, 0, 0
    q[1, 0], b[0, 0], b[1, 0], b[2, 0] = 0b1111, 0b0011, 0b0111, 0b11110000   # d = 1/2, 1/4 and 1 from integers
    D = R.tanimoto_distances(q, b)
    assert D[1, 0] == 0.5 and D[1, 1] == 0.25 and D[1, 2] == 1.0
    qg, bg = (np.arange(len(q)) % 5).astype(np.int32), (np.arange(len(b)) % 7).astype(np.int32)
    on_radius = 0
    for radius in (0.0, 0.25, 0.5, float(np.nextafter(np.float32(0.5), np.float32(0))), 2.0 / 3.0, 0.9, 1.0, float("inf")):
        want = R.tanimoto_count_ref(q, b, radius)
        got = FP.tanimoto_count(dev_words(q), dev_words(b), radius)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), radius
        on_radius += int((D == np.float32(radius)).sum())
        want = R.tanimoto_count_ref(q, b, radius, qg, bg)
        got = FP.tanimoto_count(dev_words(q), dev_words(b), radius, q_group=torch.from_numpy(qg), b_group=torch.from_numpy(bg))
        assert np.array_equal(got.cpu().numpy(), want), radius
    parity_log(f"W {W}: counts equal at 8 radii, {on_radius} pairs sit exactly on a radius")
    assert on_radius > 0
    assert (FP.tanimoto_count(dev_words(q), dev_words(b[:0]), 0.5) == 0).all()
    assert FP.tanimoto_count(dev_words(q[:0]), dev_words(b), 0.5).shape == (0,)


def test_structure_overlap_finds_exactly_the_planted_duplicates():
    rng = np.random.default_rng(61)
    train = synth.make_queries(62, 10, 3).p_specs
    val = synth.make_queries(63, 8, 2).p_specs
    planted = {2: 4, 7: 29, 8: 0, 15: 17}                             # validation row -> the training molecule it repeats
    for row, src in planted.items():
        val[row] = _renumbered(train[src], rng)                       # the same molecule under another numbering
    bank = FP.circular_fingerprint(featurization.BatchMolGraph(train), 2, 2048, gpu=0)
    bits = FP.circular_fingerprint(featurization.BatchMolGraph(val), 2, 2048, gpu=0)
    res = FP.structure_overlap(bank, bits)
    want_d, want_i = R.tanimoto_knn_ref(words_of(bits), words_of(bank), 1)
    assert res["rows"].cpu().tolist() == sorted(planted) and res["count"] == len(planted)
    assert np.array_equal(res["nearest"].cpu().numpy(), want_i[:, 0])
    # (a training molecule appears three times in a row - the candidates of one query share products only by chance - so the
    # nearest twin is the lowest index with the same fingerprint)
    tw = words_of(bank)
    for row, src in planted.items():
        assert np.array_equal(tw[int(res["nearest"][row])], tw[src])
    assert same_bits(res["similarity"].cpu().numpy(), np.float32(1.0) - want_d[:, 0])
    assert (res["similarity"][sorted(planted)] == 1).all()
    empty = FP.structure_overlap(bank[:0], bits)
    assert empty["count"] == 0 and (empty["nearest"] == -1).all()


# ---------------------------------------------------------------------------------------------- 3. what memory held, stream order
def test_nothing_depends_on_what_memory_held():
    s = odd_specs()
    batch = featurization.BatchMolGraph([s["small"], s["over"], s["empty"], s["star"]])
    batch.device_graph(0)
    q, b = search_case(71, RT + 6, 8 * BT + 76, 4)
    tq, tb = dev_words(q), dev_words(b)

    def fn():
        with splits(3):
            split = FP.tanimoto_knn(tq, tb, 16) + (FP.tanimoto_count(tq, tb, 0.8),)
        return dict(bits=FP.circular_fingerprint(batch, 3, 2048, gpu=0), counts=FP.circular_fingerprint(batch, 3, 64, True, gpu=0),
                    knn=FP.tanimoto_knn(tq, tb, 16), padded=FP.tanimoto_knn(tq[:3], tb[:5], 8), split=split,
                    count=FP.tanimoto_count(tq, tb, 0.8), pop=FP.row_popcount(tb), none=FP.tanimoto_knn(tq[:3], tb[:0], 2))
    report, counters, last = poison.fill_dependence(fn, sync=torch.cuda.synchronize)
    assert not report, report
    assert counters[0xFF].buffers >= 16                                # every output and every workspace was poisoned
    assert (last["padded"][1][:, 5:] == -1).all() and torch.isinf(last["padded"][0][:, 5:]).all()
    assert (last["none"][1] == -1).all()


def _stream_cases():
    def build_fp():
        batch = featurization.BatchMolGraph([odd_specs()["over"]] + synth.make_queries(81, 5, 2).p_specs)
        g = batch.device_graph(0)

        def fn(inputs):
            bits = FP.circular_fingerprint(batch, 2, 2048, gpu=0)
            return bits, FP.circular_fingerprint(batch, 2, 256, counts=True, gpu=0), FP.tanimoto_knn(bits, bits, 3)
        return [g.f_atoms], fn

    def build_search(with_popcount):
        def build():
            # words whose patterns read as floats in [1, 2): the harness stages float tensors in place, and a convex combination
            # of such floats is another one - the same storage, viewed as int32, is what the search reads
            rng = np.random.default_rng(83)
            q = torch.from_numpy(1.0 + rng.random((RT + 6, 4), np.float32)).cuda()
            b = torch.from_numpy(1.0 + rng.random((8 * BT + 76, 4), np.float32)).cuda()

            def fn(inputs):
                tq, tb = (t.view(torch.int32) for t in inputs)
                bp = FP.row_popcount(tb) if with_popcount else None
                return FP.tanimoto_knn(tq, tb, 8, bank_popcount=bp) + (FP.tanimoto_count(tq, tb, 0.45, bank_popcount=bp), bp)
            return [q, b], fn
        return build
    return [streams.Case("rr_circular_fp_u32+rr_tanimoto_knn_u32", build_fp),
            streams.Case("rr_tanimoto_knn_u32+rr_tanimoto_count_u32", build_search(False)),
            streams.Case("rr_row_popcount_u32+searches", build_search(True))]


@pytest.mark.parametrize("case", _stream_cases(), ids=lambda c: c.name)
def test_entry_points_are_ordered_on_the_callers_stream(case, parity_log):
    streams.check_table("fingerprints", _stream_cases())
    res = streams.staged(case, log=parity_log)
    assert res.status == "armed"


# ---------------------------------------------------------------------------------------------- 4. add_features
def test_add_features_from_the_device_equals_the_same_values_from_numpy():
    cfg = dict(hidden_size=64, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, task_num=1,
               ffn_last_layer="with_softplus", add_features_dim=64)
    model = build_model(dropout=0.0, **cfg)
    w = synth.seeded_weights(O.model_shapes(64, 3, 3, 3, 1, 64, True), 5)
    model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    model = model.cuda().eval()
    qb = synth.make_queries(91, 3, [4, 2, 5])
    rb, pb = featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs)
    for name in FP.FEATURE_NAMES:
        feat = FP.feature_generate(name, pb, num_bits=64, gpu=0)
        assert feat.is_cuda and tuple(feat.shape) == (11, 64)
        with torch.no_grad():
            on_device = model(rb, pb, gpu=0, add_features=feat)
            from_numpy = model(rb, pb, gpu=0, add_features=feat.cpu().numpy())
            without = model(rb, pb, gpu=0, add_features=np.zeros((11, 64), np.float32))
        assert torch.equal(on_device, from_numpy) and torch.isfinite(on_device).all()
        assert not torch.equal(on_device, without)                    # the features reach the score
