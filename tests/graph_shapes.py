"""Hand-built query batches with the graph shapes reactranker_amd/synth.py never draws (it makes connected trees of 5 to 24
atoms, degree at most 4): hubs with five and six neighbours, molecules without bonds, two-atom molecules, disconnected
molecules, a pad width wider than any atom needs, and ragged lists with one and with seventy candidates.  Real reaction data
has all of them (hypervalent S and P, counter-ions, A.B>>C).  A product keeps its reactant's atoms in the same order and the
features of the bonds it keeps, as synth.random_product does; the candidates of a query repeat the SAME reactant object (the
reactant de-duplication and the shared prefix key on identity).  TEST INFRASTRUCTURE."""
import numpy as np

from reactranker_amd import synth

NAMES = ("wide6", "wide5", "lone", "lone_only", "pairs", "fragments", "padded8", "ragged")


def _edges(pairs):
    return sorted({(min(a, b), max(a, b)) for a, b in pairs})


def molecule(rng, n_atoms, pairs):
    e = _edges(pairs)
    assert all(0 <= a < b < n_atoms for a, b in e)
    return synth.MolSpec(n_atoms, synth._atom_features(rng, n_atoms), synth._sorted_edges(set(e)), synth._bond_features(rng, len(e)), "R")


def product(rng, r, remove=(), add=()):
    """The reactant with the bonds `remove` taken out and `add` formed: same atoms, same order, kept bonds keep their features."""
    feat = {tuple(int(v) for v in e): r.f_bond[i] for i, e in enumerate(r.edges)}
    for e in _edges(remove):
        del feat[e]                                        # (KeyError: the bond was not there)
    for e in _edges(add):
        assert e not in feat
        feat[e] = synth._bond_features(rng, 1)[0]
    e = synth._sorted_edges(set(feat))
    fb = np.stack([feat[tuple(int(v) for v in row)] for row in e]) if len(e) else np.zeros((0, synth.BOND_FDIM), np.float32)
    return synth.MolSpec(r.n_atoms, r.f_atoms, e, fb.astype(np.float32), "P")


def max_degree(spec):
    return int(np.bincount(spec.edges.reshape(-1), minlength=spec.n_atoms).max()) if len(spec.edges) else 0


def n_components(spec):
    comp = list(range(spec.n_atoms))

    def find(a):
        while comp[a] != a:
            a = comp[a]
        return a
    for a, b in spec.edges:
        comp[find(int(a))] = find(int(b))
    return len({find(a) for a in range(spec.n_atoms)})


def _batch(rng, queries):
    """queries: [(reactant, [products])] -> QueryBatch with distinct targets per query and one add-feature column."""
    r_specs, p_specs, scope, targets = [], [], [], []
    for r, ps in queries:
        for p in ps:
            assert p.n_atoms == r.n_atoms and p.f_atoms is r.f_atoms
            r_specs.append(r)
            p_specs.append(p)
        scope.append(len(ps))
        t = rng.standard_normal(len(ps)).astype(np.float32)
        assert len(np.unique(t)) == len(t)
        targets.append(t)
    m = sum(scope)
    assert m <= 80 and max(s.n_atoms for s in r_specs) <= 16
    return synth.QueryBatch(r_specs, p_specs, scope, np.concatenate(targets), rng.random((m, 1)).astype(np.float32))


def _connected(n_atoms, pairs):
    """`pairs` plus a bond (a - 1, a) for every atom they leave without one."""
    pairs = list(pairs)
    touched = {a for e in pairs for a in e}
    return pairs + [(a - 1, a) for a in range(1, n_atoms) if a not in touched]


def _wide(rng, w):
    """Reactants with a hub of w neighbours and an atom of w - 1 elsewhere; products move one spoke of the hub to another atom, or
    move a bond that is not the hub's (so the product batch keeps a hub of full width too)."""
    # 14 atoms: hub 0 with spokes 1..w; atom 7 with w - 1 neighbours; a tail 2 - 12 - 13
    r1 = molecule(rng, 14, _connected(14, [(0, s) for s in range(1, w + 1)] + [(7, 1)] + [(7, a) for a in range(8, 6 + w)] + [(12, 2), (12, 13)]))
    p1 = [product(rng, r1, [(0, 3)], [(3, 13)]), product(rng, r1, [(0, 1)], [(1, 12)]), product(rng, r1, [(12, 13)], [(13, 4)]),
          product(rng, r1, [(7, 8)], [(8, 9)]), product(rng, r1, [(0, w)], [(w, 2)])]
    # 9 atoms, the hub in the middle of the numbering: its incoming bonds are not one run of rows
    spokes = [0, 1, 2, 3, 5, 6][:w]
    r2 = molecule(rng, 9, _connected(9, [(4, s) for s in spokes] + [(0, 1), (2, 3), (7, 8), (3, 8)]))
    p2 = [product(rng, r2, [(4, 0)], [(0, 8)]), product(rng, r2, [(0, 1)], [(1, 2)]), product(rng, r2, [(4, spokes[-1])], [(spokes[-1], 7)])]
    # two hubs that share a bond: a bond-to-bond table row that is full once the reverse bond is left out
    r3 = molecule(rng, 12, _connected(12, [(0, s) for s in range(1, w + 1)] + [(1, a) for a in range(w + 1, 2 * w)]))
    p3 = [product(rng, r3, [(0, 1)], [(2, 3)]), product(rng, r3, [(1, w + 1)], [(w + 1, 2)]), product(rng, r3, [(0, 2)], [(2, 2 * w - 1)]),
          product(rng, r3, [(0, w)], [(w, w - 1)])]
    return _batch(rng, [(r1, p1), (r2, p2), (r3, p3)])


def _lone(rng):
    o1, o2 = synth.random_reactant(rng, 7), synth.random_reactant(rng, 11)
    a1, a2 = molecule(rng, 1, []), molecule(rng, 1, [])
    return _batch(rng, [(o1, [synth.random_product(rng, o1) for _ in range(3)]), (a1, [product(rng, a1), product(rng, a1)]),
                        (o2, [synth.random_product(rng, o2) for _ in range(4)]), (a2, [product(rng, a2)])])


def _lone_only(rng):
    atoms = [molecule(rng, 1, []) for _ in range(3)]
    return _batch(rng, [(atoms[0], [product(rng, atoms[0]) for _ in range(2)]), (atoms[1], [product(rng, atoms[1])]),
                        (atoms[2], [product(rng, atoms[2]) for _ in range(3)])])


def _pairs(rng):
    bonded, other, apart = molecule(rng, 2, [(0, 1)]), molecule(rng, 2, [(0, 1)]), molecule(rng, 2, [])
    return _batch(rng, [(bonded, [product(rng, bonded, [(0, 1)]), product(rng, bonded), product(rng, bonded, [(0, 1)], [(0, 1)])]),
                        (apart, [product(rng, apart, [], [(0, 1)]), product(rng, apart)]),
                        (other, [product(rng, other, [(0, 1)]), product(rng, other)])])


def _fragments(rng):
    # A.B: a chain 0-1-2-3 with a branch, and a lone atom 5 (a counter-ion); A.B.C: 0-1-2, 3 alone, 4-5-6-7
    two = molecule(rng, 6, [(0, 1), (1, 2), (2, 3), (1, 4)])
    three = molecule(rng, 8, [(0, 1), (1, 2), (4, 5), (5, 6), (6, 7)])
    first = molecule(rng, 5, [(1, 2), (2, 3), (3, 4)])                      # the lone atom is the molecule's FIRST row
    return _batch(rng, [(two, [product(rng, two, [(2, 3)], [(3, 5)]), product(rng, two, [], [(5, 0)]), product(rng, two, [(1, 4)], [(4, 3)]),
                               product(rng, two, [(0, 1)])]),
                        (three, [product(rng, three, [], [(2, 3)]), product(rng, three, [(5, 6)], [(3, 6)]), product(rng, three, [(0, 1)], [(0, 2)])]),
                        (first, [product(rng, first, [], [(0, 1)]), product(rng, first, [(2, 3)])])])


def make(name):
    """-> (QueryBatch, pad width override or None)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "wide6":
        return _wide(rng, 6), None
    if name == "wide5":
        return _wide(rng, 5), None
    if name == "lone":
        return _lone(rng), None
    if name == "lone_only":
        return _lone_only(rng), None
    if name == "pairs":
        return _pairs(rng), None
    if name == "fragments":
        return _fragments(rng), None
    if name == "padded8":
        return synth.make_queries(21, 3, [4, 5, 3], atoms_lo=5, atoms_hi=9), 8
    if name == "ragged":
        return synth.make_queries(23, 4, [1, 70, 1, 2], atoms_lo=5, atoms_hi=10), None
    raise KeyError(name)
