"""The embedding Gaussian on the GPU (reactranker_amd.latent_gaussian, rr_col_moments_f64 / rr_center_project_f32, DESIGN.md
section 4j) against the numpy restatement of tests/moments_ref.py.

Exact cases.  Integer rows in [-3, 3] plus an integer offset per column, laid out as pairs (v, -v): the column sums are N times
the offset, so the mean, every centred value, every product and every sum are exact in f64 (and, for the projection, in f32 as
long as the row norm stays below 2^24, which the test asserts) - those cases are compared EXACTLY.

Bounds on floats, derived in tests/moments_ref.py (u = 2^-53):
  |mean' - mean|_h  <= 1.01 (N + 20) u mean_n |x_nh| =: d_h
  |S' - S|_ij       <= 1.01 (N + 68) u A_ij + N d_i d_j,  A_ij = sum_n |c_ni| |c_nj| + d_i sum_n |c_nj| + d_j sum_n |c_ni| + N d_i d_j
the chain of a scatter element being at most N products (one or two roundings each, fused or not), N + 64 additions and the two
roundings of its centred factors; the shift of the mean enters in second order only because the exactly centred rows sum to 0.
Projection (u = 2^-24), DESIGN 4g's form extended by the R-term norm:
  |y' - y|_r   <= 2 (H + 3) u sum_h |x_h - center_h| |W_hr| =: b_r
  |sq' - sq|   <= sum_r (2 |y_r| b_r + b_r^2) + 2 (R + 3) u sum_r (|y_r| + b_r)^2
knn over whitened rows: |d' - D| <= 2 (R + 3) u (|zq|^2 + |zb|^2) [rr_knn_f32's bound on the rows it was given] +
2 |zq - zb| (|eq| + |eb|) + (|eq| + |eb|)^2, e the row's vector of bounds b_r."""
import ctypes as C

import numpy as np
import pytest
import torch

from reactranker_amd import _lib, featurization
from reactranker_amd import latent_gaussian as G
from reactranker_amd import neighbors as N
from reactranker_amd.base_model import build_model
from reactranker_amd.utils import save_checkpoint
from oracle import ref_cpu as O
from tests import helpers as Hh
from tests import moments_ref as R
from tests import poison, streams

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -4, -5
NS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 257) + tuple(n + k for n in R.chunk_boundaries(33) for k in (0, 1))
HS = (1, 3, 4, 15, 16, 17, 31, 33, 300, 322)
SHAPES = sorted(set([(n, 33) for n in NS] + [(n, h) for n in (65, 1025) for h in HS] + [(2049, 300), (5, 322), (0, 1)]))
FLOAT_SHAPES = sorted(set([(n, 33) for n in NS if n > 0] + [(257, h) for h in HS] + [(1025, 64)]))


def dev(x, dtype=np.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def run(x):
    """(mean, scatter, n_used) of rr_col_moments_f64 as numpy float64 / int"""
    t = dev(x) if isinstance(x, np.ndarray) else x
    mean, sc, n = G.scatter(t)
    torch.cuda.synchronize()
    H = t.shape[1]
    assert mean.dtype == sc.dtype == torch.float64 and n.dtype == torch.int64
    assert tuple(mean.shape) == (H,) and tuple(sc.shape) == (H, H) and n.dim() == 0
    return mean.cpu().numpy(), sc.cpu().numpy(), int(n)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class blocks:
    def __init__(self, b):
        self.b = b

    def __enter__(self):
        assert _lib.lib().rr_moments_set_blocks(self.b) == 0 and _lib.lib().rr_moments_blocks() == self.b

    def __exit__(self, *a):
        assert _lib.lib().rr_moments_set_blocks(0) == 0


def int_rows(seed, n, H):
    """(x float32 [n, H], offset [H]): pairs (v, -v) of integer rows (one zero row when n is odd), shuffled, plus an integer offset"""
    rng = np.random.default_rng(seed)
    half = rng.integers(-3, 4, (n // 2, H))
    c = np.concatenate([half, -half, np.zeros((n % 2, H), np.int64)])
    c = c[rng.permutation(n)]
    off = rng.integers(-2, 3, H)
    return (c + off).astype(np.float32), off.astype(np.float64), c


def float_rows(seed, n, H, kind):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, H))
    if kind == "shifted":
        x = x + 3.0
    elif kind == "scaled":
        x = x * 30.0
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1. exact inputs, exact answer
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N{}_H{}".format(*s))
def test_moments_exact_inputs_give_the_exact_answer(shape):
    n, H = shape
    x, off, c = int_rows(7 + n + H, n, H)
    mean, sc, used = run(x)
    assert used == n
    if n == 0:
        assert not mean.any() and not sc.any() and not np.signbit(mean).any() and not np.signbit(sc).any()
        return
    assert np.array_equal(mean, off)
    assert np.array_equal(sc, c.astype(np.float64).T @ c.astype(np.float64))     # (small integers: exact in float64)
    assert bits_equal(sc, sc.T.copy())
    m2, cov, n2 = G.moments(dev(x), ddof=1)
    assert n2 == n and np.array_equal(m2.cpu().numpy(), off)
    if n > 1:
        assert np.array_equal(cov.cpu().numpy(), sc / float(n - 1))
    else:
        assert torch.isnan(cov).all() and not torch.isnan(G.moments(dev(x), ddof=0)[1]).any()


# ---------------------------------------------------------------------------------------------- 2. random floats, derived bound
@pytest.mark.parametrize("shape", FLOAT_SHAPES, ids=lambda s: "N{}_H{}".format(*s))
def test_moments_random_floats_within_the_derived_bound(shape, parity_log):
    n, H = shape
    worst_m = worst_s = 0.0
    for kind in ("normal", "shifted", "scaled"):
        x = float_rows(100 + n + H, n, H, kind)
        mean, sc, used = run(x)
        want_m, want_s, want_n = R.moments_ref(x)
        bm, bs = R.moments_bounds(x)
        assert used == want_n == n
        em = np.abs((mean.astype(R.LD) - want_m).astype(np.float64))
        es = np.abs((sc.astype(R.LD) - want_s).astype(np.float64))
        rm = float((em / np.where(bm > 0, bm, 1.0)).max())
        rs = float((es / np.where(bs > 0, bs, 1.0)).max())
        parity_log(f"N {n} H {H} {kind}: worst |mean err| / bound = {rm:.4f}, worst |scatter err| / bound = {rs:.4f}")
        worst_m, worst_s = max(worst_m, rm), max(worst_s, rs)
        assert (em <= bm).all() and (es <= bs).all()
        assert bits_equal(sc, sc.T.copy())
    Hh.record(f"moments N={n} H={H}: worst |mean err| / bound", worst_m, 1.0)
    Hh.record(f"moments N={n} H={H}: worst |scatter err| / bound", worst_s, 1.0)


# ---------------------------------------------------------------------------------------------- 3. rows that are left out
@pytest.mark.parametrize("shape", [(261, 33), (1030, 17), (70, 300)], ids=lambda s: "N{}_H{}".format(*s))
def test_non_finite_rows_take_part_in_nothing(shape):
    """Bit equality with the call WITHOUT the planted rows is asserted on exact inputs: the chunking is a function of the row count,
    so on floats the shorter call adds the same terms in another order; there the result is held to the derived bound."""
    n, H = shape
    bad = sorted({0, 5, n // 2, n - 6, n - 1, min(n - 1, 1024)})
    keep = np.setdiff1d(np.arange(n), bad)
    clean, off, c = int_rows(31 + n, n - len(bad), H)
    x = np.zeros((n, H), np.float32)
    x[keep] = clean
    fills = (np.nan, np.inf, -np.inf)
    for k, r in enumerate(bad):
        x[r] = 1e30 if k % 2 else 7.0                               # what else the row holds must not matter
        x[r, (3 * k) % H] = fills[k % 3]
    x[bad[0], H - 1] = np.nan                                        # the last column, and a row that is all NaN
    x[bad[1]] = np.nan
    got = run(x)
    want = run(clean)
    assert got[2] == want[2] == n - len(bad)
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])
    assert np.array_equal(got[0], off) and np.array_equal(got[1], c.astype(np.float64).T @ c.astype(np.float64))
    # floats: the same rows against the restatement, which filters them itself
    xf = float_rows(32 + n, n, H, "shifted")
    xf[bad, 0] = np.inf
    mean, sc, used = run(xf)
    want_m, want_s, want_n = R.moments_ref(xf)
    bm, bs = R.moments_bounds(xf)
    assert used == want_n == n - len(bad)
    assert (np.abs((mean.astype(R.LD) - want_m).astype(np.float64)) <= bm).all()
    assert (np.abs((sc.astype(R.LD) - want_s).astype(np.float64)) <= bs).all()
    # no usable row at all
    mean, sc, used = run(np.full((9, H), np.nan, np.float32))
    assert used == 0 and not mean.any() and not sc.any() and not np.signbit(sc).any()
    m2, cov, n2 = G.moments(dev(np.full((9, H), np.inf, np.float32)))
    assert n2 == 0 and torch.isnan(cov).all() and not m2.any()


# ---------------------------------------------------------------------------------------------- 4. pitch, alignment, grid, repetition
def placements(t):
    """every pitch / misalignment form of tests/streaming_edges.py for a matrix: the pointer off a 16-byte boundary by 1, 2, 3
    elements, pitches that are and are not multiples of four, both; the pad columns and the gaps hold NaN"""
    P, H = t.shape
    out = []
    for pitch in (H + 1, H + 2, H + 3, H + 4, H + 7, (H + 3) // 4 * 4 + 4):
        wide = torch.full((P, pitch), float("nan"), device="cuda")
        wide[:, :H] = t
        out.append((f"pitch {pitch}", wide[:, :H]))
    for off in (1, 2, 3):
        for pitch in (H, (H + 3) // 4 * 4, (H + 3) // 4 * 4 + 1):
            flat = torch.full((P * pitch + 8,), float("nan"), device="cuda")
            view = flat[off:off + P * pitch].view(P, pitch)
            view[:, :H] = t
            assert view.data_ptr() % 16 == 4 * off
            out.append((f"pointer + {off}, pitch {pitch}", view[:, :H]))
    return out


@pytest.mark.parametrize("shape", [(1030, 33), (301, 300), (67, 322)], ids=lambda s: "N{}_H{}".format(*s))
def test_moments_pitch_alignment_grid_and_repetition_do_not_show(shape):
    n, H = shape
    x = float_rows(9 + H, n, H, "shifted")
    x[n // 3, 1] = np.nan
    t = dev(x)
    base = G.scatter(t)

    def equal(got, what):
        for a, b, name in zip(got, base, ("mean", "scatter", "n_used")):
            assert streams.same_bits(a, b), (what, name)
    equal(G.scatter(t), "run twice")
    for b in (1, 3, 4096):
        with blocks(b):
            equal(G.scatter(t), f"blocks {b}")
    assert _lib.lib().rr_moments_blocks() == 0
    for what, view in placements(t):
        assert view.stride(0) >= H and view.stride(1) == 1
        equal(G.scatter(view), what)


# ---------------------------------------------------------------------------------------------- 5. what memory held, stream order
@pytest.mark.parametrize("shape", [(1030, 33, 0), (3, 8, 0), (301, 70, 3), (0, 5, 0)], ids=["chunks", "tiny", "blocks3", "empty"])
def test_moments_do_not_depend_on_what_memory_held(shape):
    n, H, b = shape
    t = dev(float_rows(41, n, H, "normal"))
    with blocks(b):
        report, counters, last = poison.fill_dependence(lambda: G.scatter(t), sync=torch.cuda.synchronize)
    assert not report, report
    assert counters[0xFF].buffers >= 4                               # mean, scatter, n_used and the workspace were all poisoned
    assert not torch.isnan(last[0]).any() and not torch.isnan(last[1]).any() and int(last[2]) == n


def test_projection_does_not_depend_on_what_memory_held():
    rng = np.random.default_rng(43)
    t, c, W = dev(rng.standard_normal((131, 33))), dev(rng.standard_normal(33)), dev(rng.standard_normal((33, 17)))
    report, counters, last = poison.fill_dependence(lambda: G.center_project(t, c, W, want_y=True, want_sq=True),
                                                    sync=torch.cuda.synchronize)
    assert not report, report
    assert counters[0xFF].buffers >= 2 and not torch.isnan(last[0]).any() and not torch.isnan(last[1]).any()


def _stream_cases():
    def build_moments():
        x = dev(float_rows(51, 2100, 70, "shifted"))
        return [x], lambda inputs: G.scatter(inputs[0])

    def build_project(want_y):
        def build():
            rng = np.random.default_rng(52)
            x, c, W = dev(rng.standard_normal((700, 70))), dev(rng.standard_normal(70)), dev(rng.standard_normal((70, 33)))
            return [x, c, W], lambda inputs: G.center_project(inputs[0], inputs[1], inputs[2], want_y=want_y, want_sq=True)
        return build
    return [streams.Case("rr_col_moments_f64", build_moments), streams.Case("rr_center_project_f32", build_project(True)),
            streams.Case("rr_center_project_f32 sq only", build_project(False))]


@pytest.mark.parametrize("case", _stream_cases(), ids=lambda c: c.name)
def test_entry_points_are_ordered_on_the_callers_stream(case, parity_log):
    streams.check_table("moments", _stream_cases())
    res = streams.staged(case, log=parity_log)
    assert res.status == "armed"


# ---------------------------------------------------------------------------------------------- 6. status codes through ctypes
def test_status_codes_through_ctypes():
    l = _lib.lib()
    x = torch.zeros(8, 8, device="cuda")
    mean, sc = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(8, 8, dtype=torch.float64, device="cuda")
    n = torch.zeros((), dtype=torch.int64, device="cuda")
    need = C.c_size_t()
    assert l.rr_moments_workspace_bytes(8, 8, C.byref(need)) == OK
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    p, s = _lib.ptr, _lib.stream()

    def mo(x_=p(x), ld=8, N_=8, H=8, mean_=p(mean), sc_=p(sc), n_=p(n), ws_=p(ws), nbytes=need.value):
        return l.rr_col_moments_f64(x_, ld, N_, H, mean_, sc_, n_, ws_, C.c_size_t(nbytes), s)
    for name in ("x_", "mean_", "sc_", "n_", "ws_"):
        assert mo(**{name: None}) == ARG, name
    assert mo(N_=-1) == ARG and mo(H=0) == ARG and mo(ld=7) == ARG
    assert mo(H=1025, ld=1025) == UNSUPPORTED and mo(N_=1 << 31) == UNSUPPORTED
    assert mo(nbytes=need.value - 1) == WORKSPACE
    assert mo() == OK and mo(N_=0) == OK
    torch.cuda.synchronize()
    assert int(n) == 0 and not sc.any() and not mean.any()
    W, y, sq = torch.zeros(8, 4, device="cuda"), torch.zeros(8, 4, device="cuda"), torch.zeros(8, device="cuda")

    def cp(x_=p(x), ld=8, N_=8, H=8, c_=None, W_=p(W), R_=4, y_=p(y), sq_=p(sq)):
        return l.rr_center_project_f32(x_, ld, N_, H, c_, W_, R_, y_, sq_, s)
    assert cp(x_=None) == ARG and cp(W_=None) == ARG and cp(y_=None, sq_=None) == ARG
    assert cp(N_=-1) == ARG and cp(H=0) == ARG and cp(ld=7) == ARG and cp(R_=0) == ARG and cp(R_=9) == ARG
    assert cp(N_=1 << 31) == UNSUPPORTED
    assert cp() == OK and cp(y_=None) == OK and cp(sq_=None) == OK and cp(N_=0) == OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 7. the projection
def ranks_of(H):
    return sorted({r for r in (1, 3, 16, 17, H) if r <= H})


PROJ_SHAPES = sorted(set([(n, 33) for n in (1, 2, 5, 63, 64, 65, 255, 257)] + [(65, h) for h in HS] + [(130, 322)]))


def project(x, c, W, **kw):
    y, sq = G.center_project(x if torch.is_tensor(x) else dev(x), dev(c), dev(W), **kw)
    torch.cuda.synchronize()
    return (None if y is None else y.cpu().numpy()), (None if sq is None else sq.cpu().numpy())


@pytest.mark.parametrize("shape", PROJ_SHAPES, ids=lambda s: "N{}_H{}".format(*s))
def test_projection_exact_on_integers_and_bounded_on_floats(shape, parity_log):
    n, H = shape
    worst_y = worst_s = 0.0
    for Rk in ranks_of(H):
        rng = np.random.default_rng(17 + n + 3 * H + Rk)
        # integers: x - c in [-2, 2], W in {-1, 0, 1} with three zeros in four
        c = rng.integers(-2, 3, H).astype(np.float32)
        x = (rng.integers(-2, 3, (n, H)) + c).astype(np.float32)
        W = (rng.integers(-1, 2, (H, Rk)) * (rng.integers(0, 4, (H, Rk)) == 0)).astype(np.float32)
        want_y, want_sq = R.project_ref(x, c, W)
        assert want_sq.max() < 2 ** 24                               # the precondition of exactness in f32
        y, sq = project(x, c, W, want_y=True, want_sq=True)
        assert np.array_equal(y.astype(np.float64), want_y) and np.array_equal(sq.astype(np.float64), want_sq)
        assert np.array_equal(project(x, c, W, want_y=False, want_sq=True)[1], sq)
        y0, sq0 = project(x, None, W, want_y=True, want_sq=True)
        assert np.array_equal(y0.astype(np.float64), R.project_ref(x, None, W)[0])
        assert np.array_equal(sq0, R.sq_chain32(y0))
        # floats
        x = (rng.standard_normal((n, H)) * 2.0 + 3.0).astype(np.float32)
        c = (rng.standard_normal(H) + 3.0).astype(np.float32)
        W = rng.standard_normal((H, Rk)).astype(np.float32)
        tx = dev(x)
        y, sq = project(tx, c, W, want_y=True, want_sq=True)
        y_only = project(tx, c, W)[0]
        sq_only = project(tx, c, W, want_y=False, want_sq=True)[1]
        assert project(tx, c, W)[1] is None and project(tx, c, W, want_y=False, want_sq=True)[0] is None
        assert bits_equal(y, y_only) and bits_equal(sq, sq_only)      # the variants agree bit for bit
        assert bits_equal(sq, R.sq_chain32(y))                       # sq is the stated chain over the returned y
        want_y, want_sq = R.project_ref(x, c, W)
        by, bs = R.project_bounds(x, c, W)
        ry = float((np.abs(y - want_y) / by).max())
        rs = float((np.abs(sq - want_sq) / bs).max())
        parity_log(f"N {n} H {H} R {Rk}: worst |y err| / bound = {ry:.4f}, worst |sq err| / bound = {rs:.4f}")
        worst_y, worst_s = max(worst_y, ry), max(worst_s, rs)
        assert (np.abs(y - want_y) <= by).all() and (np.abs(sq - want_sq) <= bs).all()
        y0, sq0 = project(tx, None, W, want_y=True, want_sq=True)
        b0y, b0s = R.project_bounds(x, None, W)
        w0y, w0s = R.project_ref(x, None, W)
        assert (np.abs(y0 - w0y) <= b0y).all() and (np.abs(sq0 - w0s) <= b0s).all() and bits_equal(sq0, R.sq_chain32(y0))
    Hh.record(f"center_project N={n} H={H}: worst |y err| / bound", worst_y, 1.0)
    Hh.record(f"center_project N={n} H={H}: worst |sq err| / bound", worst_s, 1.0)


@pytest.mark.parametrize("shape", [(131, 33, 17), (70, 322, 322)], ids=lambda s: "N{}_H{}_R{}".format(*s))
def test_projection_position_pitch_alignment_grid_and_repetition_do_not_show(shape):
    n, H, Rk = shape
    rng = np.random.default_rng(61 + H)
    t, c, W = dev(rng.standard_normal((n, H))), dev(rng.standard_normal(H)), dev(rng.standard_normal((H, Rk)))

    def call(xx):
        return G.center_project(xx, c, W, want_y=True, want_sq=True)
    base = call(t)

    def equal(got, what):
        assert streams.same_bits(got[0], base[0]) and streams.same_bits(got[1], base[1]), what
    equal(call(t), "run twice")
    for b in (1, 3, 4096):
        with blocks(b):
            equal(call(t), f"blocks {b}")
    for what, view in placements(t):
        equal(call(view), what)
    # the same rows at other positions of a larger matrix
    big = torch.randn(3 * n + 7, H, device="cuda")
    pos = torch.from_numpy(rng.permutation(big.shape[0])[:n]).cuda()
    big[pos] = t
    got = call(big)
    assert streams.same_bits(got[0][pos], base[0]) and streams.same_bits(got[1][pos], base[1])
    # a NaN propagates to its own row only; an infinity leaves nothing finite in its row's norm
    t2 = t.clone()
    t2[3, 1], t2[9, 0] = float("nan"), float("inf")
    y2, sq2 = call(t2)
    assert torch.isnan(sq2[3]) and torch.isnan(y2[3]).all() and not torch.isfinite(sq2[9])
    rest = torch.ones(n, dtype=torch.bool, device="cuda")
    rest[[3, 9]] = False
    assert streams.same_bits(sq2[rest], base[1][rest]) and streams.same_bits(y2[rest], base[0][rest])
    assert tuple(G.center_project(t[:0], c, W)[0].shape) == (0, Rk)


# ---------------------------------------------------------------------------------------------- 8. EmbeddingGaussian end to end
def gaussian_rows(seed, n, H, cond=10.0):
    rng = np.random.default_rng(seed)
    scale = np.logspace(0, np.log10(cond), H)
    mix = np.linalg.qr(rng.standard_normal((H, H)))[0]
    return ((rng.standard_normal((n, H)) * scale) @ mix + 3.0).astype(np.float32)


@pytest.fixture(scope="module")
def fitted():
    x = gaussian_rows(71, 600, 24)
    return x, G.EmbeddingGaussian.fit(dev(x)), R.fit_ref(x)


def test_fit_agrees_with_the_restatement(fitted):
    x, g, ref = fitted
    H = x.shape[1]
    assert g.n_ == ref["n"] == 600 and g.rank_ == ref["rank"] == H
    bm, bs = R.moments_bounds(x)
    assert (np.abs(g.mean_.numpy() - ref["mean"]) <= bm).all()
    assert (np.abs(g.cov_.numpy() - ref["cov"]) <= bs / 599 * 1.01).all()
    lam = ref["eigenvalues"]
    assert np.abs(g.eigenvalues_.numpy() - lam).max() <= 1e-10 * lam[0] and (np.diff(g.eigenvalues_.numpy()) <= 0).all()
    assert np.abs(g.explained_variance_ratio_.numpy() - ref["explained_variance_ratio"]).max() <= 1e-10
    comp, wh = g.components_.cpu().numpy(), g.whitener_.cpu().numpy()
    assert comp.dtype == wh.dtype == np.float32 and comp.shape == wh.shape == (H, H)
    assert np.abs(comp - ref["components_r"]).max() <= 1e-6                    # (the sign rule: no sign is free)
    assert (np.abs(wh - ref["whitener"]) <= 1e-6 * np.abs(ref["whitener"]).max(axis=0)).all()
    big = np.abs(comp).argmax(axis=0)
    assert (comp[big, np.arange(H)] > 0).all()
    # options
    g2 = G.EmbeddingGaussian.fit(dev(x), shrinkage=0.25, rank=5)
    assert g2.rank_ == 5 and tuple(g2.whitener_.shape) == (H, 5)
    assert np.allclose(g2.eigenvalues_.numpy(), 0.75 * lam + 0.25 * lam.mean(), rtol=1e-9)
    dup = np.concatenate([x, x[:, :3]], axis=1)
    assert G.EmbeddingGaussian.fit(dev(dup)).rank_ == H == R.fit_ref(dup)["rank"]
    assert G.EmbeddingGaussian.fit(dev(x[:9])).rank_ == 8
    with pytest.raises(ValueError, match="usable rows"):
        G.EmbeddingGaussian.fit(dev(x[:1]))
    with pytest.raises(ValueError, match="width"):
        g.mahalanobis(dev(x[:, :5]))
    with pytest.raises(ValueError, match="n_components"):
        g.project(dev(x), 0)


def test_mahalanobis_identity_project_and_round_trip(fitted, tmp_path, parity_log):
    x, g, ref = fitted
    n, H = x.shape
    tx = dev(x)
    d2 = g.mahalanobis(tx)
    assert d2.dtype == torch.float32 and tuple(d2.shape) == (n,)
    c32, W32 = g.center_.cpu().numpy(), g.whitener_.cpu().numpy()
    want = R.project_ref(x, c32, W32)[1]
    bound = R.project_bounds(x, c32, W32)[1]
    err = np.abs(d2.cpu().numpy() - want)
    parity_log(f"mahalanobis 600 x 24: worst |err| / bound = {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    # the bank's own mean squared distance is rank (n - 1) / n; the float64 model agrees to 1e-5 relative
    assert abs(float(d2.double().mean()) - H * (n - 1) / n) <= float(bound.mean()) + 1e-5 * H
    assert np.abs(want - R.mahalanobis_ref(x, ref)).max() <= 1e-5 * want.max()
    z = g.whiten(tx)
    assert tuple(z.shape) == (n, H) and z.dtype == torch.float32
    assert bits_equal(d2.cpu().numpy(), R.sq_chain32(z.cpu().numpy()))            # mahalanobis is the norm of whiten's rows
    # PCA scores: the derived bound under the model's own f32 matrices, and the restatement's scores up to the sign rule
    for k in (1, 2, 5, H):
        y = g.project(tx, k).cpu().numpy()
        C32 = g.components_.cpu().numpy()[:, :k]
        wy = R.project_ref(x, c32, C32)[0]
        assert (np.abs(y - wy) <= R.project_bounds(x, c32, C32)[0]).all()
        ry = R.project_ref(x, ref["mean"], ref["components_r"][:, :k])[0]
        tol = R.project_bounds(x, c32, C32)[0] + 2e-6 * (np.abs(x.astype(np.float64) - ref["mean"]).sum(axis=1, keepdims=True)
                                                         + np.abs(ref["mean"]).sum())
        assert (np.abs(y - ry) <= tol).all()
    var = g.project(tx, H).double().var(dim=0, unbiased=True).cpu().numpy()
    assert np.abs(var - ref["eigenvalues"]).max() <= 1e-4 * ref["eigenvalues"][0]
    # save / load
    path = str(tmp_path / "gaussian.pt")
    g.save(path)
    back = G.EmbeddingGaussian.load(path, "cuda")
    assert back.n_ == g.n_ and back.rank_ == g.rank_
    for name in ("mean_", "cov_", "eigenvalues_", "explained_variance_ratio_", "components_", "whitener_", "center_"):
        assert streams.same_bits(getattr(back, name), getattr(g, name)), name
    assert back.whitener_.is_cuda and streams.same_bits(back.mahalanobis(tx), d2)
    bank = N.ReactionBank(tx, torch.zeros(n), torch.arange(n) // 10)
    g3 = G.EmbeddingGaussian.from_bank(bank)
    assert streams.same_bits(g3.whitener_, g.whitener_) and streams.same_bits(g3.mean_, g.mean_)


def test_knn_on_whitened_rows_is_the_mahalanobis_search(fitted, parity_log):
    x, g, ref = fitted
    H = x.shape[1]
    q = gaussian_rows(72, 70, H)
    zq, zb = g.whiten(dev(q)), g.whiten(dev(x))
    k = 8
    dist, idx = N.knn(zq, zb, k)
    dist, idx = dist.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    c32, W32 = g.center_.cpu().numpy(), g.whitener_.cpu().numpy()
    Zq, Zb = R.project_ref(q, c32, W32)[0], R.project_ref(x, c32, W32)[0]
    eq = np.linalg.norm(R.project_bounds(q, c32, W32)[0], axis=1)
    eb = np.linalg.norm(R.project_bounds(x, c32, W32)[0], axis=1)
    D = ((Zq[:, None, :] - Zb[None, :, :]) ** 2).sum(-1)                           # float64 Mahalanobis distances of all pairs
    e = eq[:, None] + eb[None, :]
    tol = 2 * (H + 3) * R.U24 * ((Zq ** 2).sum(1)[:, None] + (Zb ** 2).sum(1)[None, :]) * 1.01 + 2 * np.sqrt(D) * e + e * e
    rows = np.arange(len(q))[:, None]
    assert (idx >= 0).all()
    err = np.abs(dist - D[rows, idx])
    parity_log(f"knn over whitened rows, H {H}: worst |dist - D64| / tol = {float((err / tol[rows, idx]).max()):.4f}")
    assert (err <= tol[rows, idx]).all()
    # nothing closer was left out, and the distances are those of the float64 model of the restatement too
    kth = idx[:, k - 1]
    m = np.arange(len(q))
    cut = (D[m, kth] - tol[m, kth])[:, None] - tol
    left = np.ones_like(D, bool)
    left[rows, idx] = False
    assert not (left & (D < cut)).any()
    Dref = ((R.project_ref(q, ref["mean"], ref["whitener"])[0][:, None, :]
             - R.project_ref(x, ref["mean"], ref["whitener"])[0][None, :, :]) ** 2).sum(-1)
    assert np.abs(Dref - D).max() <= 1e-5 * D.max()
    sel = N.kcenter_greedy(zb, 4)                                                  # the Mahalanobis k-center runs on the same rows
    assert (sel["picks"] >= 0).all()


CFG_KEYS = ("hidden_size", "mpnn_depth", "mpnn_diff_depth", "ffn_depth", "use_bias", "task_num", "ffn_last_layer", "task_type",
            "add_features_dim")


def test_evaluate_applicability_with_the_mahalanobis_distance_on_a_golden_model(tmp_path):
    path = [p for p in Hh.model_case_files() if "model_A_" in p][0]
    d, cfg = Hh.load_case(path)
    shapes = O.model_shapes(cfg["hidden_size"], cfg["mpnn_depth"], cfg["mpnn_diff_depth"], cfg["ffn_depth"], cfg["task_num"],
                            cfg["add_features_dim"], cfg["use_bias"])
    model = build_model(dropout=0.0, **{k: cfg[k] for k in CFG_KEYS})
    model.load_state_dict({k: torch.tensor(v) for k, v in Hh.case_weights(d, cfg, shapes).items()})
    model = model.cuda()
    qb = Hh.case_queries(cfg)
    rb, pb = featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs)
    add = d["add_features"] if "add_features" in d.files else None
    targets = torch.tensor(d["targets"])
    bank = N.ReactionBank.from_batches(model, [(rb, pb, cfg["scope"], targets, add)], 0)
    ck = str(tmp_path / "ck" / "0.pt")
    save_checkpoint(ck, model, 0.0, 1.0)
    test_b = [dict(r=rb, p=pb, scope=cfg["scope"], targets=targets, add=add)]
    g = G.EmbeddingGaussian.from_bank(bank)
    assert 1 <= g.rank_ <= min(len(bank) - 1, cfg["hidden_size"])
    res = N.evaluate_applicability(model, bank, test_b, ck, 0, method="mahalanobis")
    res_g = N.evaluate_applicability(model, bank, test_b, ck, 0, method="mahalanobis", gaussian=g)
    n = sum(cfg["scope"])
    assert tuple(res["distance"].shape) == (n,) and torch.isfinite(res["distance"]).all() and (res["distance"] >= 0).all()
    assert streams.same_bits(res["distance"], res_g["distance"])
    assert streams.same_bits(res["distance"], g.mahalanobis(bank.vectors).sqrt())      # the test set IS the bank here
    # the identity rank (n - 1) / n, loosely: f32 rounding is not small against the directions just above the eigenvalue floor
    assert abs(float(res["distance"].double().pow(2).mean()) - g.rank_ * (n - 1) / n) <= 0.05 * g.rank_
    assert tuple(res["qstats"].shape) == (len(cfg["scope"]), 12) and "spearman" in res["calibration"]
    # the default is what it was: the latent distance, under the criterion of tests/test_gpu_neighbors.py (the same bits)
    base = N.evaluate_applicability(model, bank, test_b, ck, 0, k=4)
    knn_ = N.evaluate_applicability(model, bank, test_b, ck, 0, k=4, method="knn")
    assert streams.same_bits(base["distance"], N.latent_distance(bank, bank.vectors, 4))
    assert streams.same_bits(base["distance"], knn_["distance"]) and streams.same_bits(base["pred"], res["pred"])
