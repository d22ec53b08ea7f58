"""Sphere-exclusion clustering on the GPU (reactranker_amd.clusters, rr_radius_count_f32 / rr_sphere_exclusion_f32, DESIGN.md
section 4k) against the numpy oracle of tests/cluster_ref.py.

Integer coordinates in [-3, 3] make every operation of both distance forms exact in f32, and r2 = floor(a quantile of the pair
distances) + 0.5 keeps every distance away from r2: those cases must equal the float64 rounds exactly, ties included.  On random
floats the labels must be the bits of the oracle's f32 restatement of the chain (exclusion32) under the GPU's own counts as key,
and are replayed against float64 under the project's derived bounds: gamma(H) = 2 (H + 3) 2^-24 of tests/selection_ref.py for
the difference chain, tol(q, b) = 2 (H + 3) 2^-24 (|q|^2 + |b|^2) of tests/neighbors_ref.py for knn's form.  No other tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from reactranker_amd import _lib
from reactranker_amd import clusters as K
from reactranker_amd import neighbors as N
from tests import cluster_ref as CR
from tests import helpers as Hh
from tests import neighbors_ref as R
from tests import poison, streams
from tests import selection_ref as S
from tests.test_gpu_kcenter import bank_case, float_case, int_case  # noqa: F401  (bank_case is a fixture)

pytestmark = pytest.mark.gpu

RT, BT, _ = N.geometry()
W = K.ROWS_PER_WORKGROUP
SPLITS = (0, 1, 2, 3, 7)                                             # every setting tests/test_gpu_neighbors.py uses
QUANTILE_ROWS = 600                                                  # the pair distances of at most this many leading rows


def dev(x, dtype=np.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


class blocks:
    def __init__(self, b):
        self.b = b

    def __enter__(self):
        assert _lib.lib().rr_sphere_exclusion_set_blocks(self.b) == 0 and _lib.lib().rr_sphere_exclusion_blocks() == self.b

    def __exit__(self, *a):
        assert _lib.lib().rr_sphere_exclusion_set_blocks(0) == 0


class splits:
    def __init__(self, s):
        self.s = s

    def __enter__(self):
        assert _lib.lib().rr_knn_set_splits(self.s) == 0

    def __exit__(self, *a):
        assert _lib.lib().rr_knn_set_splits(0) == 0


def exact_radius(x, q):
    """(radius, r2) with r2 = floor(q-quantile of the pair distances) + 0.5: no integer distance equals it, and the package's
    rule float32(float64(radius) ** 2) gives it back exactly"""
    head = np.asarray(x[:QUANTILE_ROWS], np.float64)
    r2 = np.float32(np.floor(np.quantile(R.distances64(head, head), q)) + 0.5)
    radius = float(np.sqrt(np.float64(r2)))
    assert CR.r2_of(radius) == r2 and K.radius_squared(radius) == float(r2)
    return radius, r2


def cluster(tx, radius, **kw):
    res = K.sphere_exclusion(tx, radius, **kw)
    torch.cuda.synchronize()
    P = tx.shape[0]
    assert res["labels"].dtype == res["centres"].dtype == res["sizes"].dtype == torch.int64
    assert tuple(res["labels"].shape) == (P,) and res["centres"].shape == res["sizes"].shape
    out = {k: (None if res[k] is None else res[k].cpu().numpy()) for k in ("labels", "centres", "sizes", "key")}
    out["n_clusters"], out["n_unassigned"] = int(res["n_clusters"]), int(res["n_unassigned"])
    lab, cen = out["labels"], out["centres"]
    assert out["n_clusters"] == (cen >= 0).sum() and out["n_unassigned"] == (lab == -1).sum()
    assert np.array_equal(out["sizes"], np.bincount(lab[lab >= 0], minlength=len(cen))[:len(cen)])
    assert (lab[cen[cen >= 0]] == np.nonzero(cen >= 0)[0]).all()     # a centre is a member of its own cluster
    return out


def same_as(got, want, what=""):
    assert np.array_equal(got["labels"], want["labels"]), (what, "labels")
    assert np.array_equal(got["centres"], want["centres"]), (what, "centres")


def raw_rounds(tx, r2, key, pieces, block_settings=(0,)):
    """rr_sphere_exclusion_f32 itself, one call per entry of `pieces` (rounds per call), each continuing the one before it
    through first_round; labels, centres and the workspace start as garbage"""
    P, H = tx.shape
    l = _lib.lib()
    labels = torch.full((max(P, 1),), 7, dtype=torch.int32, device="cuda")
    nbytes = C.c_size_t()
    assert l.rr_sphere_exclusion_workspace_bytes(P, C.byref(nbytes)) == 0
    ws = torch.full((nbytes.value,), 0xAB, dtype=torch.uint8, device="cuda")
    k32 = None if key is None else dev(key, np.int32)
    cents, first = [], 0
    for j, n in enumerate(pieces):
        out = torch.full((max(n, 1),), 99, dtype=torch.int32, device="cuda")
        with blocks(block_settings[j % len(block_settings)]):
            st = l.rr_sphere_exclusion_f32(_lib.ptr(tx), tx.stride(0) if P > 1 else H, P, H, C.c_float(float(r2)), _lib.ptr(k32),
                                           first, n, _lib.ptr(labels), _lib.ptr(out), _lib.ptr(ws), C.c_size_t(nbytes.value),
                                           _lib.stream())
        assert st == 0
        cents.append(out[:n])
        first += n
    torch.cuda.synchronize()
    return dict(labels=labels[:P].cpu().numpy().astype(np.int64), centres=torch.cat(cents).cpu().numpy().astype(np.int64))


# ---------------------------------------------------------------------------------------------- 1. exact inputs, exact answer
def _exact_cases():
    cases = [dict(P=131, H=h, q=0.1, B=0) for h in (1, 3, 4, 5, 30, 252, 256, 257, 260, 300, 322, 600)]
    cases += [dict(P=131, H=300, q=0.02, B=0), dict(P=517, H=30, q=0.05, B=0), dict(P=517, H=4, q=0.05, B=3)]
    cases += [dict(P=67, H=h, q=0.1, B=0) for h in (1024, 1025, 1100)]        # the last register width, then the loop for wider rows
    for B in (1, 2, 4096):
        cases += [dict(P=P, H=30 if B < 4096 or P < 100 else 5, q=0.1, B=B) for P in (1, W - 1, W, W + 1, 3 * W * B + 5)]
    return cases


@pytest.mark.parametrize("c", _exact_cases(), ids=lambda c: "P{P}_H{H}_q{q}_B{B}".format(**c))
def test_exact_inputs_give_the_exact_answer(c):
    P, H = c["P"], c["H"]
    x = int_case(11 + P + H, P, H)[0]
    radius, r2 = exact_radius(x, c["q"])
    tx = dev(x)
    rng = np.random.default_rng(P + H)
    if P <= 1000:                                                    # the density key needs the [P, P] float64 distances
        key = CR.count64(x, x, r2)
        cnt = K.radius_count(tx, tx, radius)
        assert cnt.dtype == torch.int64 and np.array_equal(cnt.cpu().numpy(), key)
        assert (key >= 1).all()                                      # a row counts itself
        want = CR.exclusion64(x, r2, key)
        with blocks(c["B"]):
            got = cluster(tx, radius)
        same_as(got, want, "density")
        assert np.array_equal(got["key"], key) and got["n_unassigned"] == 0 and got["n_clusters"] == len(want["centres"])
        if P >= 100:
            assert want["by_index"].any()                            # at least one round was decided by the index
            assert 7 <= len(want["centres"]) < P // 2 + 20           # (7 .. 91 clusters over the cases, singletons in all but one)
    explicit = rng.integers(0, 5, P)
    for what, k, kw in (("index", None, dict(order="index")), ("key", explicit, dict(key=dev(explicit, np.int64)))):
        want = CR.exclusion64(x, r2, k)
        with blocks(c["B"]):
            got = cluster(tx, radius, **kw)
        same_as(got, want, what)
        assert (got["key"] is None) == (k is None) and got["n_unassigned"] == 0
        assert k is not None or P < 2 or want["by_index"].any()      # (equal keys: the index decides whenever two rows are left)


@pytest.mark.parametrize("c", [dict(P=131, H=30, q=0.1), dict(P=517, H=4, q=0.05), dict(P=67, H=1025, q=0.1)],
                         ids=lambda c: "P{P}_H{H}".format(**c))
def test_round_counts_padding_and_continued_calls(c):
    x = int_case(11 + c["P"] + c["H"], c["P"], c["H"])[0]
    radius, r2 = exact_radius(x, c["q"])
    tx = dev(x)
    key = CR.count64(x, x, r2)
    n_k = len(CR.exclusion64(x, r2, key)["centres"])
    assert n_k >= 7
    for n in (0, 1, n_k - 1, n_k, n_k + 3):
        want = CR.exclusion64(x, r2, key, n=n)
        got = cluster(tx, radius, max_clusters=n)
        same_as(got, want, f"max_clusters {n}")
        assert got["centres"].shape == (n,) and got["n_clusters"] == min(n, n_k)
        assert (got["n_unassigned"] == 0) == (n >= n_k) and (got["sizes"][n_k:] == 0).all()
    # one call of n_k + 3 rounds against the same rounds in calls of 1, 2 and 7 (and what is left), under changing grids
    total = n_k + 3
    want = CR.exclusion64(x, r2, key, n=total)
    same_as(raw_rounds(tx, r2, key, [total]), want, "one call")
    for step in (1, 2, 7):
        pieces = [step] * (total // step) + ([total % step] if total % step else [])
        same_as(raw_rounds(tx, r2, key, pieces, block_settings=(0, 1, 3)), want, f"calls of {step}")
    same_as(raw_rounds(tx, r2, key, [0, 3, 0, total - 3]), want, "empty calls in between")


TILE_SIZES = (63, 64, 65, 127, 128, 129, 300)


@pytest.mark.parametrize("shape", [(m, 300) for m in TILE_SIZES] + [(65, n) for n in TILE_SIZES] + [(129, 3 * BT + 5)],
                         ids=lambda s: f"M{s[0]}_N{s[1]}")
def test_counts_around_the_tiles_at_every_split_setting(shape):
    M, Nb = shape
    rng = np.random.default_rng(M + Nb)
    q = rng.integers(-3, 4, (M, 30)).astype(np.float32)
    b = rng.integers(-3, 4, (Nb, 30)).astype(np.float32)
    for j in range(9):
        b[(7 * j + 3) % Nb] = q[(5 * j) % M]                         # duplicates of query rows: d = 0
    radius, r2 = exact_radius(np.concatenate([q, b]), 0.1)
    qg, bg = (np.arange(M) % 8).astype(np.int32), ((np.arange(Nb) // 50) % 9 - 1).astype(np.int32)
    want = CR.count64(q, b, r2)
    want_g = CR.count64(q, b, r2, qg, bg)
    assert want.max() > want.min() and (want_g < want).any() and (want_g > 0).any()
    tq, tb = dev(q), dev(b)
    bn = N.row_sqnorm(tb)
    for s in SPLITS:
        with splits(s):
            got = K.radius_count(tq, tb, radius)
            got_g = K.radius_count(tq, tb, radius, q_group=dev(qg, np.int32), b_group=dev(bg, np.int32), bank_sqnorm=bn)
        assert np.array_equal(got.cpu().numpy(), want), s
        assert np.array_equal(got_g.cpu().numpy(), want_g), s


# ---------------------------------------------------------------------------------------------- 2. random floats
@pytest.mark.parametrize("H", [1, 3, 4, 30, 300, 322, 600])
def test_random_floats_are_the_chains_bits_and_mean_what_float64_says(H, parity_log):
    P = 517
    g = S.gamma(H)
    worst_member = worst_centre = worst_band = 0.0
    for kind in ("normal", "shifted", "scaled"):
        x = float_case(200 + H, P, H, kind)[0]
        D = R.distances64(x, x)
        radius = float(np.sqrt(np.quantile(D, 0.05)))
        r2 = CR.r2_of(radius)
        assert r2 > 0
        tx = dev(x)
        cnt = K.radius_count(tx, tx, radius)
        key = cnt.cpu().numpy()
        # (c) the counts, against float64 under knn's bound: every pair is either surely inside, surely outside or in the band
        T = R.tol(x, x)
        lo, hi = (D + T <= np.float64(r2)).sum(axis=1), (D - T <= np.float64(r2)).sum(axis=1)
        assert (lo <= key).all() and (key <= hi).all()
        band = float((hi - lo).sum()) / D.size
        # (a) the clustering under the GPU's own counts: the bits of the f32 chain
        got = cluster(tx, radius, key=cnt)
        want = CR.exclusion32(x, r2, key)
        same_as(got, want, kind)
        assert got["n_unassigned"] == 0 and np.array_equal(cluster(tx, radius)["labels"], got["labels"])   # 'density' is that key
        # (b) what it means in float64
        member_d, held = CR.replay64(x, got["centres"], got["labels"], key)
        assert held.all()                                            # every centre held the largest key when it was taken
        assert (member_d <= np.float64(r2) * (1 + g)).all()
        cen = got["centres"]
        between = D[np.ix_(cen, cen)] + np.where(np.eye(len(cen), dtype=bool), np.inf, 0.0)
        assert (between > np.float64(r2) * (1 - g)).all()
        r_member = float(max(0.0, (member_d / np.float64(r2) - 1).max()) / g)
        r_centre = float(max(0.0, (1 - between.min() / np.float64(r2))) / g) if len(cen) > 1 else 0.0
        # how near a decision came to r2, in units of gamma (large: no member and no pair of centres was a close call)
        near_member = float(np.nanmin(np.abs(member_d / np.float64(r2) - 1)) / g)
        near_centre = float(np.abs(between / np.float64(r2) - 1).min() / g) if len(cen) > 1 else np.inf
        parity_log(f"H {H} {kind}: {len(cen)} clusters, {int((got['sizes'] == 1).sum())} singletons, "
                   f"{int(want['by_index'].sum())} rounds by index; worst (d64 / r2 - 1) / gamma of a member = {r_member:.4f} "
                   f"(nearest to r2: {near_member:.3g} gamma), worst (1 - d64 / r2) / gamma between centres = {r_centre:.4f} "
                   f"(nearest: {near_centre:.3g} gamma); pairs inside the count's band: {band:.2e}")
        worst_member, worst_centre, worst_band = max(worst_member, r_member), max(worst_centre, r_centre), max(worst_band, band)
    Hh.record(f"sphere_exclusion H={H}: worst (d64 / r2 - 1) / gamma of a member", worst_member, 1.0)
    Hh.record(f"sphere_exclusion H={H}: worst (1 - d64 / r2) / gamma between centres", worst_centre, 1.0)
    Hh.record(f"radius_count H={H}: fraction of pairs inside the band of tol", worst_band, None)


# ---------------------------------------------------------------------------------------------- 3. planted clusters
def test_planted_clusters_come_back_largest_first():
    rng = np.random.default_rng(5)
    sizes = np.array([65, 61, 52, 47, 40, 33, 29, 24, 19, 15, 12, 10])
    H, radius = 30, 1.0
    order = rng.permutation(len(sizes))                              # the cluster ids are not in order of size
    member = np.repeat(order, sizes)
    centres = 100.0 * rng.standard_normal((len(sizes), H))
    x = (centres[member] + 0.005 * rng.standard_normal((member.size, H))).astype(np.float32)
    perm = rng.permutation(member.size)
    x, member = x[perm], member[perm]
    D = R.distances64(x, x)
    same_cluster = member[:, None] == member[None, :]
    assert D[same_cluster].max() * 100 < radius ** 2 and D[~same_cluster].min() > 100 * radius ** 2   # the oracle's own precondition
    tx = dev(x)
    cnt = K.radius_count(tx, tx, radius).cpu().numpy()
    size_of = np.zeros(len(sizes), np.int64)
    size_of[order] = sizes
    assert np.array_equal(cnt, size_of[member])                      # the density of a row is the size of its cluster
    got = cluster(tx, radius)
    assert got["n_clusters"] == len(sizes) == len(got["centres"]) and got["n_unassigned"] == 0
    assert np.array_equal(got["sizes"], sizes)                       # largest first
    assert np.array_equal(member[got["centres"]], order)
    rank = np.empty(len(sizes), np.int64)
    rank[order] = np.arange(len(sizes))
    assert np.array_equal(got["labels"], rank[member])               # labels are membership
    for t, c in enumerate(got["centres"]):
        assert c == np.nonzero(member == order[t])[0][0]             # equal keys inside a cluster: its first row


# ---------------------------------------------------------------------------------------------- 4. nothing shows that must not
@pytest.mark.parametrize("H", [322, 300])
def test_position_pitch_alignment_grid_splits_and_repetition_do_not_show(H):
    rng = np.random.default_rng(9 + H)
    P = 301
    x = rng.standard_normal((P, H)).astype(np.float32)
    for j in range(6):
        x[(11 * j + 2) % P] = x[(3 * j) % P]
    radius = float(np.sqrt(np.quantile(R.distances64(x, x), 0.05)))
    tx = dev(x)

    def call(xx):
        r = K.sphere_exclusion(xx, radius)
        return dict(count=K.radius_count(xx, xx, radius), labels=r["labels"], centres=r["centres"], sizes=r["sizes"], key=r["key"])

    def equal(a, b, what):
        for k in a:
            assert torch.equal(a[k], b[k]), (what, k)
    base = call(tx)
    assert 3 <= base["centres"].numel() < P and torch.equal(base["key"], base["count"])
    equal(call(tx), base, "run twice")
    for b in (1, 3, 4096):
        with blocks(b):
            equal(call(tx), base, f"blocks {b}")
    assert _lib.lib().rr_sphere_exclusion_blocks() == 0
    for s in (1, 2, 3, 7):
        with splits(s):
            equal(call(tx), base, f"splits {s}")
    assert _lib.lib().rr_knn_splits() == 0
    # the same rows, in the same order, scattered inside a larger pool whose other rows are non-finite
    big = torch.full((3 * P + 7, H), float("nan"), device="cuda")
    big[::5] = float("inf")
    pos = torch.from_numpy(np.sort(rng.permutation(big.shape[0])[:P])).cuda()
    big[pos] = tx
    got = call(big)
    assert torch.equal(got["centres"], pos[base["centres"]]) and torch.equal(got["sizes"], base["sizes"])
    assert torch.equal(got["labels"][pos], base["labels"]) and torch.equal(got["count"][pos], base["count"])
    other = torch.ones(big.shape[0], dtype=torch.bool, device="cuda")
    other[pos] = False
    assert (got["labels"][other] == -2).all() and (got["count"][other] == 0).all()
    # other pitches (the pad columns hold NaN: they never reach a result) and a base pointer 4 bytes off a 16-byte boundary
    for pitch in (H + 2, H + 5, H + 6):
        wide = torch.full((P, pitch), float("nan"), device="cuda")
        wide[:, :H] = tx
        view = wide[:, :H]
        assert view.stride(0) == pitch
        equal(call(view), base, f"pitch {pitch}")
    for pitch in (H, H + 2):
        flat = torch.full((P * pitch + 1,), float("nan"), device="cuda")
        off = flat[1:].view(P, pitch)
        off[:, :H] = tx
        assert off.data_ptr() % 16 == 4
        equal(call(off[:, :H]), base, f"pointer + 4, pitch {pitch}")


# ---------------------------------------------------------------------------------------------- 5. rows that cannot be taken
def test_rows_that_cannot_be_taken_and_degenerate_inputs():
    P, H = 200, 30
    x = int_case(23, P, H)[0]
    x[17] = np.nan
    x[40, 3] = np.nan
    x[50, 29] = np.inf
    x[51, 0] = -np.inf
    bad = [17, 40, 50, 51]
    radius, _ = exact_radius(int_case(23, P, H)[0], 0.1)
    r2 = CR.r2_of(radius)
    tx = dev(x)
    cnt = K.radius_count(tx, tx, radius).cpu().numpy()
    assert np.array_equal(cnt, CR.count64(x, x, r2)) and (cnt[bad] == 0).all()
    for kw, key in ((dict(), cnt), (dict(order="index"), None)):
        got = cluster(tx, radius, **kw)
        same_as(got, CR.exclusion64(x, r2, key), str(kw))
        assert (got["labels"][bad] == -2).all() and not np.isin(got["centres"], bad).any() and got["n_unassigned"] == 0
        assert got["sizes"].sum() == P - 4
    more = cluster(tx, radius, max_clusters=P + 3)
    same_as(more, CR.exclusion64(x, r2, cnt, n=P + 3), "padded")
    assert (more["centres"][more["n_clusters"]:] == -1).all() and more["n_clusters"] < P
    # r2 = 0: exact duplicates cluster together, every other row is a singleton
    zero = cluster(tx, 0.0)
    same_as(zero, CR.exclusion64(x, 0.0, CR.count64(x, x, 0.0)), "r2 = 0")
    twins = zero["sizes"] > 1
    assert 1 <= twins.sum() <= 9 and (zero["sizes"][~twins] == 1).all()
    for t in np.nonzero(twins)[0]:
        rows = np.nonzero(zero["labels"] == t)[0]
        assert (x[rows] == x[rows[0]]).all()
    assert (np.diff(zero["sizes"]) <= 0).all()                       # Butina: the duplicates, being denser, come first
    # r2 = +inf: one cluster of everything finite
    # (in index order: against a row that holds an infinity knn's form gives +inf or a NaN by the sign of the other row's
    # column, so at r2 = +inf the density keys of this pool are not worth stating; on finite rows every pair counts)
    one = cluster(tx, float("inf"), order="index")
    assert one["centres"].tolist() == [0] and one["sizes"].tolist() == [P - 4] and (one["labels"][bad] == -2).all()
    clean = dev(int_case(23, P, H)[0])
    assert (K.radius_count(clean, clean, float("inf")) == P).all()
    assert cluster(clean, float("inf"))["sizes"].tolist() == [P]
    # nobody can be taken: all padding
    nan = dev(np.full((5, 4), np.nan, np.float32))
    got = cluster(nan, 1.0)
    assert got["centres"].shape == (0,) and (got["labels"] == -2).all() and got["n_clusters"] == 0
    got = cluster(nan, 1.0, max_clusters=3)
    assert got["centres"].tolist() == [-1] * 3 and got["sizes"].tolist() == [0] * 3 and (got["labels"] == -2).all()
    assert (K.radius_count(nan, nan, 1.0) == 0).all()
    # no rows at all
    empty = dev(np.zeros((0, H), np.float32))
    got = cluster(empty, 1.0)
    assert got["labels"].shape == (0,) and got["centres"].shape == (0,) and got["key"] is None
    got = cluster(empty, 1.0, max_clusters=3)
    assert got["centres"].tolist() == [-1] * 3 and got["labels"].shape == (0,)
    assert cluster(empty, 1.0, max_clusters=0)["centres"].shape == (0,)
    assert K.radius_count(empty, tx, 1.0).shape == (0,)                       # M == 0
    assert K.radius_count(tx, empty, 1.0).cpu().tolist() == [0] * P           # N == 0


# ---------------------------------------------------------------------------------------------- 6. what memory held, stream order
@pytest.mark.parametrize("shape", [(RT + 6, 8 * BT + 76), (3, 5)], ids=["split", "small"])
def test_counts_do_not_depend_on_what_memory_held(shape):
    M, Nb = shape
    rng = np.random.default_rng(31)
    tq, tb = dev(rng.standard_normal((M, 30))), dev(rng.standard_normal((Nb, 30)))
    report, counters, last = poison.fill_dependence(lambda: K.radius_count(tq, tb, 7.0), sync=torch.cuda.synchronize)
    assert not report, report
    assert counters[0xFF].buffers >= 2                               # the counts and the workspace were both poisoned
    assert (last >= 0).all() and (last <= Nb).all() and 0 < int(last.sum()) < M * Nb


@pytest.mark.parametrize("shape", [(301, 16, 0), (3, 8, 0), (301, None, 3)], ids=["auto", "padded", "blocks3_batches"])
def test_clusters_do_not_depend_on_what_memory_held(shape):
    P, n, b = shape
    rng = np.random.default_rng(31)
    tx = dev(rng.standard_normal((P, 30)))
    with blocks(b):
        report, counters, last = poison.fill_dependence(lambda: K.sphere_exclusion(tx, 6.5, max_clusters=n),
                                                        sync=torch.cuda.synchronize)
    assert not report, report
    assert counters[0xFF].buffers >= 5                               # counts, labels, centres and both workspaces were poisoned
    assert (last["labels"] >= -1).all() and int(last["n_clusters"]) >= 3
    if n is not None and P < n:
        assert (last["centres"][P:] == -1).all() and (last["sizes"][P:] == 0).all()


def _stream_cases():
    def build_count():
        rng = np.random.default_rng(41)
        q, b = dev(rng.standard_normal((RT + 6, 30))), dev(rng.standard_normal((8 * BT + 76, 30)))
        return [q, b], lambda inputs: K.radius_count(inputs[0], inputs[1], 7.0)

    def build_for(order):
        def build():
            x = dev(np.random.default_rng(41).standard_normal((600, 30)))
            return [x], lambda inputs: K.sphere_exclusion(inputs[0], 6.5, order=order, max_clusters=32)
        return build
    return [streams.Case("rr_radius_count_f32", build_count), streams.Case("rr_sphere_exclusion_f32 density", build_for("density")),
            streams.Case("rr_sphere_exclusion_f32 index", build_for("index"))]


@pytest.mark.parametrize("case", _stream_cases(), ids=lambda c: c.name)
def test_the_calls_are_ordered_on_the_callers_stream(case, parity_log):
    streams.check_table("clusters", _stream_cases())
    res = streams.staged(case, log=parity_log)
    assert res.status == "armed"


# ---------------------------------------------------------------------------------------------- 7. end to end
def test_cluster_split_of_a_models_queries_end_to_end(bank_case, parity_log):
    model, train, bank = bank_case
    qv = K.query_vectors(bank.vectors, bank.group)
    n_q = int(bank.group.max()) + 1
    assert tuple(qv.shape) == (n_q, bank.vectors.shape[1]) and qv.dtype == torch.float32
    for j in (0, 5, n_q - 1):                                        # the f32 rounding of a float64 mean against torch's f32 mean
        want = bank.vectors[bank.group == j].mean(dim=0)
        assert torch.allclose(qv[j], want, rtol=1e-5, atol=1e-6 * float(want.abs().max()))
    radius = K.suggest_radius(qv, k=2, quantile=0.5)
    assert np.isfinite(radius) and radius > 0
    res = K.sphere_exclusion(qv, radius)
    labels = res["labels"]
    assert int(res["n_unassigned"]) == 0 and 1 < int(res["n_clusters"]) <= n_q and int(res["sizes"].sum()) == n_q
    folds = K.cluster_split(labels, (0.6, 0.2, 0.2), seed=0)
    assert folds.is_cuda and folds.dtype == torch.int64 and (folds >= 0).all()
    for c in range(int(res["n_clusters"])):
        assert len(set(folds[labels == c].cpu().tolist())) == 1      # no cluster is cut
    assert (folds == 0).any()
    rep = K.split_report(qv, folds, k=1)
    assert rep["levels"] == K.REPORT_LEVELS and rep["folds"] == sorted(set(folds[folds >= 1].cpu().tolist()))
    assert tuple(rep["quantiles"].shape) == (len(rep["folds"]), len(K.REPORT_LEVELS)) and sum(rep["n"]) == int((folds >= 1).sum())
    assert torch.isfinite(rep["quantiles"]).all() and (rep["quantiles"] > 0).all() and (rep["quantiles"].diff(dim=1) >= 0).all()
    # a held-out row's nearest training row lies outside its own cluster's sphere only if ... nothing is promised; it is reported
    kf = K.cluster_kfold(labels, 3, seed=1)
    assert sorted(set(kf.cpu().tolist())) == [0, 1, 2] or int(res["n_clusters"]) < 3
    parity_log(f"{n_q} queries, radius {radius:.4f}: {int(res['n_clusters'])} clusters, sizes {res['sizes'].cpu().tolist()}, "
               f"folds {torch.bincount(folds).cpu().tolist()}, median distance to fold 0: {rep['quantiles'][:, 2].tolist()}")
