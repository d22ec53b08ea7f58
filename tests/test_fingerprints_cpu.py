"""The numpy restatement of the circular fingerprint and of the Tanimoto search (tests/fingerprint_ref.py) held to the definition
itself, and the Python layer's argument errors (reactranker_amd.fingerprints) that are raised before the library is touched.
No GPU needed."""
import numpy as np
import pytest
import torch

from reactranker_amd import _lib, featurization, synth
from reactranker_amd import fingerprints as FP
from tests import fingerprint_ref as R

NEW_SYMBOLS = ("rr_circular_fp_workspace_bytes", "rr_circular_fp_u32", "rr_row_popcount_u32", "rr_tanimoto_knn_workspace_bytes",
               "rr_tanimoto_knn_u32", "rr_tanimoto_count_workspace_bytes", "rr_tanimoto_count_u32", "rr_tanimoto_geometry",
               "rr_tanimoto_splits", "rr_tanimoto_set_splits")


# ---------------------------------------------------------------------------------------------- a scalar restatement
def _fmix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _step(h, w):
    return _fmix(((h ^ w) + 0x9E3779B9) & 0xFFFFFFFF)


def _rowhash(row):
    h = 0
    for v in row:
        u = int(np.float32(v).view(np.uint32))
        h = _step(h, 0 if u == 0x80000000 else u)
    return h


def scalar_ids(fa, bc, a2b, b2a, radius):
    """the definition, one atom and one bond at a time in Python integers"""
    nA = len(fa)
    ids = [[_rowhash(fa[a]) for a in range(nA)]]
    bh = [_rowhash(bc[b]) for b in range(len(bc))]
    for r in range(1, radius + 1):
        prev, cur = ids[-1], []
        for a in range(nA):
            S = X = 0
            for b in a2b[a]:
                if b != 0:
                    m = _step(bh[b], prev[int(b2a[b])])
                    S = (S + m) & 0xFFFFFFFF
                    X ^= _fmix(m ^ 0x7F4A7C15)
            cur.append(_step(_step(_step(prev[a], r), S), X))
        ids.append(cur)
    return ids


def hand_molecule():
    """a chain 1 - 2 - 3 (row 0 is the padding atom, bond 0 the padding bond); atom 3 equals atom 1 up to the sign of a zero"""
    fa = np.zeros((4, 2), np.float32)
    fa[1], fa[2], fa[3] = [1, 0], [0, 1], [1, -0.0]
    bc = np.zeros((5, 1), np.float32)
    bc[1] = bc[2] = 1.0                                               # bonds 1: 1->2, 2: 2->1, 3: 2->3, 4: 3->2
    bc[3] = bc[4] = 2.0
    b2a = np.array([0, 1, 2, 2, 3], np.int32)
    a2b = np.array([[0, 0], [2, 0], [1, 4], [3, 0]], np.int32)
    return fa, bc, a2b, b2a


def test_literal_ids_of_a_hand_written_molecule():
    assert _fmix(1) == 0x514E28B7                                     # murmur3's finaliser, a published value
    fa, bc, a2b, b2a = hand_molecule()
    ids = R.atom_ids(fa, bc, a2b, b2a, 2)
    want = [[0xECD1134D, 0xECA81E2F, 0xECD1134D],
            [0xE186BF11, 0x3F9EDD0A, 0xD10AD237],
            [0x2C80DB1F, 0x4F4DD61C, 0xCE9F073A]]
    assert [[int(v) for v in row[1:]] for row in ids] == want
    assert [row[1:] for row in scalar_ids(fa, bc, a2b, b2a, 2)] == want
    assert ids[0][1] == ids[0][3]                                     # -0.0 hashes as +0.0 ...
    assert ids[1][1] != ids[1][3]                                     # ... and the two ends differ once their bonds are seen
    words, counts = R.fingerprint_ref(fa, bc, a2b, b2a, [[1, 3]], 2, 64)
    assert counts.sum() == 9 and words.tolist() == [[2416059392, 75530240]]
    assert np.array_equal(R.unpack_bits_ref(words), counts > 0)


def _batch(seed=3, n=5, lo=10, hi=24):
    qb = synth.make_queries(seed, n, 2, atoms_lo=lo, atoms_hi=hi)
    return qb.p_specs[::2]


def test_vectorised_reference_equals_the_scalar_one_on_packed_batches():
    batch = featurization.BatchMolGraph(_batch())
    fa, bc, a2b, b2a, scope = R.batch_arrays(batch)
    assert bc.shape[1] == synth.BOND_FDIM and fa.shape[1] == synth.ATOM_FDIM
    ids = R.atom_ids(fa, bc, a2b, b2a, 3)
    assert [[int(v) for v in row] for row in ids] == scalar_ids(fa, bc, a2b, b2a, 3)


def _renumbered(spec, rng):
    """the same molecule with its atoms permuted (the sorted edge list then permutes the bonds as well)"""
    n = spec.n_atoms
    new_of_old = rng.permutation(n)
    old_of_new = np.argsort(new_of_old)
    e = np.sort(new_of_old[spec.edges.astype(np.int64)], axis=1)
    order = np.lexsort((e[:, 1], e[:, 0]))
    return synth.MolSpec(n, spec.f_atoms[old_of_new], e[order].astype(np.int32), spec.f_bond[order], spec.smiles)


def test_renumbering_atoms_and_bonds_leaves_the_counts_unchanged():
    rng = np.random.default_rng(5)
    specs = _batch(7, 6)
    perm = [_renumbered(s, rng) for s in specs]
    assert any(not np.array_equal(a.edges, b.edges) for a, b in zip(specs, perm))
    for radius in (0, 2, 3):
        a = R.batch_fingerprint_ref(featurization.BatchMolGraph(specs), radius, 2048)
        b = R.batch_fingerprint_ref(featurization.BatchMolGraph(perm), radius, 2048)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_radius_zero_is_the_histogram_of_atom_hashes():
    batch = featurization.BatchMolGraph(_batch(9, 4))
    fa, bc, a2b, b2a, scope = R.batch_arrays(batch)
    _, counts = R.fingerprint_ref(fa, bc, a2b, b2a, scope, 0, 64)
    h = R.rowhash(fa)
    for m, (start, size) in enumerate(scope):
        want = np.bincount((h[start:start + size] % np.uint64(64)).astype(np.int64), minlength=64)
        assert np.array_equal(counts[m], want) and counts[m].sum() == size


def test_a_row_does_not_depend_on_the_rest_of_the_batch_and_a_change_stays_local():
    specs = _batch(11, 6)
    whole = R.batch_fingerprint_ref(featurization.BatchMolGraph(specs), 2, 2048)
    for i in (0, 3, 5):
        alone = R.batch_fingerprint_ref(featurization.BatchMolGraph([specs[i]]), 2, 2048)
        assert np.array_equal(alone[0][0], whole[0][i]) and np.array_equal(alone[1][0], whole[1][i])
    last = R.batch_fingerprint_ref(featurization.BatchMolGraph(specs[::-1]), 2, 2048)
    assert np.array_equal(last[1][::-1], whole[1])
    # one atom feature flipped: only the ids within two bonds of it move, every other bin keeps its count
    s = specs[0]
    fa2 = s.f_atoms.copy()
    fa2[0, 0] = 1.0 - fa2[0, 0]
    changed = R.batch_fingerprint_ref(featurization.BatchMolGraph([synth.MolSpec(s.n_atoms, fa2, s.edges, s.f_bond)]), 2, 2048)
    moved = int((changed[1][0] != whole[1][0]).sum())
    assert 2 <= moved < 2 * 3 * s.n_atoms and changed[1][0].sum() == whole[1][0].sum() == 3 * s.n_atoms


def test_pack_and_unpack_round_trip_and_agree_with_the_python_layer():
    rng = np.random.default_rng(13)
    on = rng.random((7, 96)) < 0.4
    on[0] = False
    on[1] = True
    words = R.pack_bits_ref(on)
    assert words.dtype == np.uint32 and np.array_equal(R.unpack_bits_ref(words), on)
    assert words[1].tolist() == [0xFFFFFFFF] * 3 and np.array_equal(R.popcount_rows(words), on.sum(axis=1))
    t = torch.from_numpy(words.view(np.int32))
    assert torch.equal(FP.unpack_bits(t), torch.from_numpy(on.astype(np.float32)))
    assert torch.equal(FP.pack_bits(torch.from_numpy(on.astype(np.float32))), t)


def test_tanimoto_reference_on_cases_worked_by_hand():
    q = np.array([[0b1111], [0], [0b0011]], np.uint32)
    b = np.array([[0b0011], [0b1100], [0], [0b1111], [0b0011]], np.uint32)
    D = R.tanimoto_distances(q, b)
    assert D.dtype == np.float32
    assert D[0].tolist() == [0.5, 0.5, 1.0, 0.0, 0.5] and D[1].tolist() == [1.0, 1.0, 0.0, 1.0, 1.0]
    assert D[2, 1] == 1.0 and D[2, 0] == 0.0
    d, i = R.tanimoto_knn_ref(q, b, 3)
    assert i.tolist() == [[3, 0, 1], [2, 0, 1], [0, 4, 3]] and d[0].tolist() == [0.0, 0.5, 0.5]
    d, i = R.tanimoto_knn_ref(q, b, 6, q_group=[0, -1, 7], b_group=[7, 0, 0, 0, -1])
    assert i[0].tolist() == [0, 4, -1, -1, -1, -1] and np.isinf(d[0, 2:]).all() and i[1, 5] == -1 and i[2].tolist()[:2] == [4, 3]
    assert R.tanimoto_count_ref(q, b, 0.5).tolist() == [4, 1, 3]
    assert R.tanimoto_count_ref(q, b, np.nextafter(np.float32(0.5), np.float32(0))).tolist() == [1, 1, 2]
    third = R.tanimoto_distances(np.array([[0b0111]], np.uint32), np.array([[0b0001]], np.uint32))[0, 0]
    assert third == np.float32(2) / np.float32(3)


def test_bindings_are_declared():
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS, s
    l = _lib.lib()
    assert FP.geometry() == (64, 128, 64, 256)
    assert l.rr_tanimoto_splits() == 0 and l.rr_tanimoto_set_splits(-1) != 0 and l.rr_tanimoto_set_splits(1025) != 0
    assert l.rr_tanimoto_set_splits(3) == 0 and l.rr_tanimoto_splits() == 3 and l.rr_tanimoto_set_splits(0) == 0


# ---------------------------------------------------------------------------------------------- argument errors
def test_fingerprint_argument_errors_name_the_public_function():
    batch = featurization.BatchMolGraph(_batch(3, 2))
    for kw in (dict(radius=-1), dict(radius=9), dict(radius=1.5), dict(num_bits=0), dict(num_bits=48), dict(num_bits=8224),
               dict(num_bits=16)):
        with pytest.raises(ValueError, match="^circular_fingerprint: "):
            FP.circular_fingerprint(batch, **kw)
        with pytest.raises(ValueError, match="^feature_generate: "):
            FP.feature_generate("binary_morgan_fingerprint", batch, **kw)
        with pytest.raises(ValueError, match="^reaction_fingerprint: "):
            FP.reaction_fingerprint(batch, batch, **kw)
    with pytest.raises(ValueError, match="^circular_fingerprint: `batch`"):
        FP.circular_fingerprint([1, 2, 3])
    with pytest.raises(ValueError, match="^feature_generate: 'MACCS_keys_fingerprint'.*RDKit"):
        FP.feature_generate("MACCS_keys_fingerprint", batch)
    with pytest.raises(ValueError, match="^feature_generate: name must be one of"):
        FP.feature_generate("morgan", batch)
    with pytest.raises(ValueError, match="^reaction_fingerprint: mode"):
        FP.reaction_fingerprint(batch, batch, mode="sum")


def test_search_argument_errors_name_the_public_function():
    q = torch.zeros(3, 2, dtype=torch.int32)
    for fn, extra in ((FP.tanimoto_knn, (1,)), (FP.tanimoto_count, (0.5,))):
        name = fn.__name__
        with pytest.raises(ValueError, match=f"^{name}: .*must live on the GPU"):
            fn(q, q, *extra)
        with pytest.raises(ValueError, match=f"^{name}: `queries` must be int32 words"):
            fn(q.float(), q, *extra)
        with pytest.raises(ValueError, match=f"^{name}: `bank` must be a matrix of words"):
            fn(q, q[0], *extra)
        with pytest.raises(ValueError, match=f"^{name}: q_group and b_group go together"):
            fn(q, q, *extra, q_group=[0, 1, 2])
        with pytest.raises(ValueError, match=f"^{name}: `queries` has rows of 257 words"):
            fn(torch.zeros(1, 257, dtype=torch.int32), q, *extra)
    for k in (0, 65, 2.5):
        with pytest.raises(ValueError, match="^tanimoto_knn: k must be"):
            FP.tanimoto_knn(q, q, k)
    for r in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="^tanimoto_count: radius"):
            FP.tanimoto_count(q, q, r)
    with pytest.raises(ValueError, match="^row_popcount: .*must live on the GPU"):
        FP.row_popcount(q)
    with pytest.raises(ValueError, match="^unpack_bits: "):
        FP.unpack_bits(q.float())
    with pytest.raises(ValueError, match="^pack_bits: "):
        FP.pack_bits(torch.zeros(2, 33))


def test_host_side_under_address_and_ub_sanitizers(tmp_path):
    """tools/fingerprint_host_check.cpp as its header says: a stand-alone program, every call returns before a launch"""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "fingerprint_host_check")
    srcs = [os.path.join("reactranker_amd", "csrc", u + ".hip") for u in ("fingerprint", "tanimoto")]
    build = subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host",
                            "-fsanitize=address,undefined", *srcs, os.path.join("tools", "fingerprint_host_check.cpp"), "-o", exe],
                           cwd=repo, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], cwd=repo, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "host checks clean" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
