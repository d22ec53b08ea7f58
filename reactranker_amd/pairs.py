"""Pair batches for the baseline pair model: what `DataProcessor.generate_query_pairs` / `generate_query_pair_batch` of the
reference (data/load_reactions.py:470-538) hand to `baseline_pairwise_training_loop` and `pairwise_baseline_acc`, built
from per-candidate molecule graphs instead of a DataFrame of SMILES (that side stays the reference's).

Inside a query the pairs come in the reference's order: for every distinct target value in order of first appearance, each
row holding that value against each row holding another value - so both directions of every unequal pair appear, and a
query with one distinct value gives none.  Queries follow each other in the order given (the reference shuffles the
reactants with numpy's global generator first, :513-515); the pairs of all queries are cut into batches of `batch_size`,
and what remains is the last, short batch: the accuracy uses it, training skips it (train_pairwise.py:24)."""
from __future__ import annotations

from typing import Iterator, List, Sequence, Tuple

import numpy as np

from .featurization import BatchMolGraph, MolGraph


def query_pairs(targets) -> Tuple[np.ndarray, np.ndarray]:
    """(i, j) row indices of one query's pairs in the reference's order (load_reactions.py:484-495)."""
    t = np.asarray(targets).reshape(-1)
    _, first, inv = np.unique(t, return_index=True, return_inverse=True)
    rows = np.arange(len(t))
    ii: List[np.ndarray] = []
    jj: List[np.ndarray] = []
    for u in np.argsort(first, kind="stable"):            # distinct values by first appearance
        a, b = rows[inv == u], rows[inv != u]
        ii.append(np.repeat(a, len(b)))
        jj.append(np.tile(b, len(a)))
    if not ii:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    return np.concatenate(ii).astype(np.int32), np.concatenate(jj).astype(np.int32)


def window_pairs(scope: Sequence[int], targets) -> Tuple[np.ndarray, np.ndarray]:
    """The pairs of every query of a window, as indices into the window's candidate list."""
    t = np.asarray(targets).reshape(-1)
    ii, jj, off = [], [], 0
    for c in scope:
        a, b = query_pairs(t[off:off + c])
        ii.append(a + off)
        jj.append(b + off)
        off += int(c)
    if not ii:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    return np.concatenate(ii).astype(np.int32), np.concatenate(jj).astype(np.int32)


def _spec(m):
    return m.spec if isinstance(m, MolGraph) else m


def _atom_rows(batch: BatchMolGraph) -> Tuple[np.ndarray, np.ndarray]:
    sc = np.asarray(batch._host["a_scope"], np.int64).reshape(-1, 2)
    return sc[:, 0], sc[:, 1]


def pair_batch(mols_r, mols_p, ii, jj, targets) -> dict:
    """One batch of pairs (candidate ii[b] against candidate jj[b]): r / p1 / p2 graphs with one common pad width, targets
    [B, 2] = (t[ii], t[jj]), and `index` = (u, ir, i1, i2) for the pair model's de-duplicated path: u holds every distinct
    molecule of the batch once, and atom row a of the pair batch is row ir[a] / i1[a] / i2[a] of u for its reactant / first
    product / second product (row 0, the padding row, maps to row 0)."""
    t = np.asarray(targets, np.float32).reshape(-1)
    rs = [_spec(mols_r[i]) for i in ii]
    p1s = [_spec(mols_p[i]) for i in ii]
    p2s = [_spec(mols_p[j]) for j in jj]
    first, distinct = {}, []
    for s in rs + p1s + p2s:
        if id(s) not in first:
            first[id(s)] = len(distinct)
            distinct.append(s)
    u = BatchMolGraph(distinct)
    K = u.max_num_bonds                                   # the widest atom of the batch: one pad width for all four graphs
    r, p1, p2 = (BatchMolGraph(x, K=K) for x in (rs, p1s, p2s))
    if not (r.max_num_bonds == p1.max_num_bonds == p2.max_num_bonds == K):
        raise RuntimeError("pair_batch: pad widths differ")
    ustart, usize = _atom_rows(u)
    rstart, rsize = _atom_rows(r)
    nA = r.n_atoms
    within = np.arange(int(rsize.sum())) - np.repeat(np.cumsum(rsize) - rsize, rsize)
    rows = np.repeat(rstart, rsize) + within

    def index(specs):
        uid = np.asarray([first[id(s)] for s in specs], np.int64)
        if not np.array_equal(usize[uid], rsize):
            raise ValueError("pair_batch: reactant and products of a pair must hold the same atoms in the same order")
        out = np.zeros(nA, np.int32)
        out[rows] = (np.repeat(ustart[uid], rsize) + within).astype(np.int32)
        return out
    return dict(r=r, p1=p1, p2=p2, targets=np.stack([t[ii], t[jj]], axis=1).astype(np.float32),
                index=(u, index(rs), index(p1s), index(p2s)), pairs=(np.asarray(ii, np.int32), np.asarray(jj, np.int32)))


def pair_windows(mols_r, mols_p, scope: Sequence[int], targets, batch_size: int) -> Iterator[dict]:
    """Pair batches of a window of whole queries (mols_r / mols_p: the reactant / product graph of every candidate, MolGraph or
    MolSpec; repeated reactants should be the same object, as synth.make_queries and mol2graph's cache make them).  Yields
    whole batches of `batch_size` pairs and then the last short one, each with `full` = whether it holds batch_size pairs."""
    if batch_size < 1:
        raise ValueError("pair_windows: batch_size must be at least 1")
    ii, jj = window_pairs(scope, targets)
    for lo in range(0, len(ii), batch_size):
        b = pair_batch(mols_r, mols_p, ii[lo:lo + batch_size], jj[lo:lo + batch_size], targets)
        b["full"] = len(b["targets"]) == batch_size
        yield b
