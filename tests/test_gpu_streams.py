"""Where and when the work is enqueued: every entry point on a NON-default stream, behind a delayed producer, against the
same call on the default stream - bit for bit (tests/streams.py says how and what a failure means).  Sections: A the per-op
entry points, B the losses, C the evaluation kernels, D the whole model (plan and per-op mirror), E training steps without a
host synchronisation, F two caller streams (the workspace pool, the shared side / aux streams), G the shard prefetcher with a
consumer off the default stream.  The case tables are plain data (tests/test_streams_cpu.py checks their exemption cap)."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from reactranker_amd import attribution, featurization, shards, synth
from reactranker_amd import eval as EV
from reactranker_amd import functions as Fn
from reactranker_amd import loss as RL
from reactranker_amd import uncertainty as UQ
from reactranker_amd._lib import check, lib, ptr, stream
from reactranker_amd.train_utils import HipAdam
from tests import streams as S
from tests.streams import Case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def gemm(f16=False):
    """the split-GEMM arithmetic for the duration (three bf16 terms, or two f16 terms)"""
    old = Fn.SplitGemm.f16
    Fn.SplitGemm.f16 = f16
    try:
        yield
    finally:
        Fn.SplitGemm.f16 = old


def rnd(seed, *shape, positive=False, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(*shape, generator=g) + 0.5 if positive else torch.randn(*shape, generator=g)
    return (t * scale).to(DEV)


def index(seed, n_src, *shape, lo=-1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, n_src, shape, generator=g, dtype=torch.int32).to(DEV)


def run(case, parity_log):
    return S.staged(case, log=parity_log)


# ============================================================================================== the harness itself (pure torch)
def test_harness_passes_an_ordered_op_and_flags_a_misordered_one_and_an_unarmed_one(parity_log):
    probe = rnd(0, 1000)
    # the mis-ordered op's stream must be able to run while the caller's stream is held up (two streams may share a queue)
    caller, side = S.concurrent_pair(lambda: probe * 2, log=parity_log)

    def ordered():
        return [rnd(1, 1000)], lambda inp: inp[0] * 2

    def misordered():
        def fn(inp):
            with torch.cuda.stream(side):                          # no side.wait_stream(current): the entry wait is missing
                y = inp[0] * 2
            torch.cuda.current_stream().wait_stream(side)          # (the exit join is there)
            return y
        return [rnd(1, 1000)], fn

    def blocking():
        def fn(inp):
            inp[0].sum().item()                                    # blocks the host until the delay has passed
            return inp[0] * 2
        return [rnd(1, 1000)], fn

    r = S.staged(Case("ordered x*2", ordered), log=parity_log)
    assert r.status == "armed" and S.MIN_DELAY_MS <= r.delay_ms <= S.MAX_DELAY_MS
    with pytest.raises(S.OrderingViolation) as e:
        S.staged(Case("misordered x*2", misordered), log=parity_log, stream=caller)
    assert e.value.kind == "entry"
    with pytest.raises(S.OrderingViolation) as e:
        S.staged(Case("blocking x*2", blocking), log=parity_log)
    assert e.value.kind == "not armed"
    r = S.staged(Case("blocking x*2, declared", blocking, True, "calls .item() first"), log=parity_log)
    assert r.status == "exempt"
    parity_log(f"torch.cuda._sleep: {S.cycles_per_ms():.0f} cycles per ms")


# ============================================================================================== A. per-op entry points
def _a_linear_f32():
    a, w, b = rnd(1, 65, 32), rnd(2, 32, 32, scale=0.2), rnd(3, 32)
    return [a, w, b], lambda i: Fn.linear(65, 32, i[1], a1=i[0], k1=32, bias=i[2], act=Fn.ACT_RELU)


def _a_linear_split():
    M = 8256
    assert M >= Fn.SPLIT_MIN_ROWS
    a, w, b = rnd(4, M, 32), rnd(5, 32, 32, scale=0.2), rnd(6, 32)

    def fn(i):
        W = Fn.LinW(i[1], i[2])                                    # (a fresh pack per call: it is part of what is ordered)
        pk = W.pk(32)
        assert pk.dtype == torch.uint8
        return Fn.linear(M, 32, pk, a1=i[0], k1=32, bias=W.b, act=Fn.ACT_RELU)
    return [a, w, b], fn


def _a_wgrad(M, k2):
    def build():
        N, k1 = 32, 32
        dy, y, x1 = rnd(7 + M, M, N), torch.relu(rnd(8 + M, M, N)), rnd(9 + M, M, k1)
        x2 = rnd(10 + M, M, (k2 + 3) // 4 * 4) if k2 else None
        ins = [dy, y, x1] + ([x2] if k2 else [])

        def fn(i):
            dw, db = torch.empty(N, k1 + k2, device=DEV), torch.empty(N, device=DEV)
            Fn.wgrad(M, N, i[0], dw, dbias=db, mask=i[1], mask_scale=0.5, x1=i[2], k1=k1, x2=i[3] if k2 else None, k2=k2,
                     side=True)
            Fn.SideStream.join(dw.device)
            return [dw, db]
        return ins, fn
    return build


H, K, ROWS, NSRC = 32, 4, 50, 70


def _a_gather(kind):
    def build():
        src, idx = rnd(20, NSRC, H), index(21, NSRC, ROWS, K)
        if kind == "plain":
            return [src], lambda i: Fn.gather_sum(i[0], idx, H)
        if kind == "masked":
            mask = torch.relu(rnd(22, NSRC, H))
            return [src, mask], lambda i: Fn.gather_sum_masked(i[0], i[1], 1.25, idx, H)
        if kind == "adds":
            mask, a1, a2 = torch.relu(rnd(23, ROWS, H)), rnd(24, ROWS, H), rnd(25, ROWS, H)
            return [src, mask, a1, a2], lambda i: Fn.gather_sum(i[0], idx, H, mask=i[1], mask_scale=1.25, adds=[i[2], i[3]])
        if kind == "row0_partial":
            part = rnd(26, 3, H)
            return [src, part], lambda i: Fn.gather_sum(i[0], idx, H, row0_partial=i[1])
        if kind == "multi":
            s2, s3 = rnd(27, NSRC, H), rnd(28, NSRC, H)
            return [src, s2, s3], lambda i: Fn.gather_sum_multi([i[0], i[1], i[2]], idx, H)
        assert kind == "dropmask"
        y = rnd(29, ROWS, H)
        return [src, y], lambda i: Fn.gather_sum_dropmask(i[0], i[1], 1.25, idx, H, 0.2, 77)
    return build


def _a_gather_diff():
    a, m, ia, im = rnd(30, NSRC, H), rnd(31, NSRC, H), index(32, NSRC, ROWS), index(33, NSRC, ROWS)
    return [a, m], lambda i: Fn.gather_diff(i[0], ia, i[1], im, H)


_GRAPH = {}


def small_graph():
    """one product graph of three queries (a real DeviceGraph: a_scope, atom2mol and the bond tables are consistent)"""
    if "g" not in _GRAPH:
        qb = synth.make_queries(1, 3, [5, 3, 6], atoms_lo=5, atoms_hi=12)
        pb = featurization.BatchMolGraph(qb.p_specs, K=4)
        _GRAPH["g"], _GRAPH["pb"] = pb.device_graph(0), pb
    return _GRAPH["g"]


def _a_segment_mean_fwd():
    g = small_graph()
    x, feat = rnd(40, g.nA, H), rnd(41, g.M, 1)
    return [x, feat], lambda i: Fn.segment_mean_fwd(i[0], g, H, i[1], 1, 0.1, 5)


def _a_segment_mean_bwd(masked):
    def build():
        g = small_graph()
        dout = rnd(42, g.M, H + 1)
        if not masked:
            return [dout], lambda i: Fn.segment_mean_bwd(i[0], g, H, 1, 0.1, 5)
        mask = torch.relu(rnd(43, g.nA, H))
        return [dout, mask], lambda i: Fn.segment_mean_bwd(i[0], g, H, 1, 0.1, 5, mask=i[1], mask_scale=1.25)
    return build


def _a_head(bwd):
    def build():
        raw, dout = rnd(44, 50, 2, scale=3.0), rnd(45, 50, 2)
        if bwd:
            return [dout, raw], lambda i: Fn.head_bwd(i[0], i[1], 3)
        return [raw], lambda i: Fn.head_fwd(i[0], 3)
    return build


def _a_dropout():
    x = rnd(46, 1001)
    return [x], lambda i: Fn.dropout(i[0], 0.2, 99)


def _a_relu_bwd():
    dy, y, acc = rnd(47, 101, 30), torch.relu(rnd(48, 101, 30)), rnd(49, 101, 30)

    def fn(i):
        a = i[2].clone()
        return [Fn.relu_bwd(i[0], i[1], -1.5, acc=a), a]
    return [dy, y, acc], fn


def _a_axpby():
    a, b = rnd(50, 1001), rnd(51, 1001)
    return [a, b], lambda i: Fn.axpby(2.0, i[0], -1.0, i[1])


def _a_weighted_colsum():
    x, w = rnd(52, 300, H), rnd(53, 300, positive=True)
    return [x, w], lambda i: Fn.weighted_colsum(i[0], i[1], H, torch.empty(H, device=DEV), accumulate=False)


def _a_amax():
    t = rnd(54, 257, 36)
    return [t], lambda i: Fn.amax(i[0], 33)


FFN_WIDTHS, FFN_M = [36, 32, 32, 1], 20


def _ffn_tensors():
    ws = [rnd(60 + j, n, k, scale=k ** -0.5) for j, (k, n) in enumerate(zip(FFN_WIDTHS[:-1], FFN_WIDTHS[1:]))]
    bs = [rnd(70 + j, n, scale=0.3) for j, n in enumerate(FFN_WIDTHS[1:])]
    return ws, bs


def _a_ffn_chain(bwd):
    from tests.test_gpu_ffn import _chain_backward, _chain_forward

    def build():
        ws, bs = _ffn_tensors()
        x, d = rnd(80, FFN_M, FFN_WIDTHS[0]), rnd(81, FFN_M, FFN_WIDTHS[-1])
        nl = len(ws)

        def fn(i):
            layers = [Fn.LinW(i[2 + j], i[2 + nl + j], big=False) for j in range(nl)]
            if not bwd:
                st, hs = _chain_forward(i[0], FFN_WIDTHS[0], layers, 0.1, 91)
                check(st, "rr_ffn_chain_f32")
                return hs
            _, (hs, raw) = Fn.ffn_forward(i[0], layers, 0.1, 17, 0)
            st, outs = _chain_backward(i[1], layers, hs, 0.1, FFN_WIDTHS[1])     # the readout columns (36 = 32 + 4 features)
            check(st, "rr_ffn_chain_f32")
            return outs
        return [x, d] + ws + bs, fn
    return build


def _a_pack_then_gemm(transpose):
    def build():
        M, N, Kk = 100, 32, 36
        w, a, dy = rnd(82, N, Kk, scale=0.2), rnd(83, M, Kk), rnd(84, M, N)

        def fn(i):
            W = Fn.LinW(i[0], None, big=False)
            if transpose:
                return Fn.linear(M, Kk, W.pk_t(0, Kk), w_packed=True, a1=i[2], k1=N)
            return Fn.linear(M, N, W.pk(Kk), w_packed=True, a1=i[1], k1=Kk)
        return [w, a, dy], fn
    return build


def _a_build_fbonds():
    small_graph()
    h = _GRAPH["pb"]._host
    fb = np.zeros((h["nB"], 24), np.float32)
    fb[:, :22] = h["f_bonds"][:, 61:83]
    t = {k: torch.from_numpy(h[k]).to(DEV) for k in featurization._GRAPH_KEYS}
    t["fbond"] = torch.from_numpy(fb).to(DEV)
    g = featurization.DeviceGraph.from_device(t, h["nA"], h["nB"], h["K"], h["M"], DEV)

    def fn(i):
        g._f_bonds = None                                          # rebuilt by rr_build_fbonds_f32 on the next read
        return g.f_bonds
    return [g.f_atoms, g.fbond], fn


def _a_adam():
    sizes = [1, 1025, 4096]
    ps = [torch.nn.Parameter(rnd(90 + j, n)) for j, n in enumerate(sizes)]
    gs = [rnd(93 + j, n) for j, n in enumerate(sizes)]
    ms = [rnd(96 + j, n, scale=0.1) for j, n in enumerate(sizes)]
    vs = [rnd(99 + j, n, positive=True, scale=0.01) for j, n in enumerate(sizes)]
    opt = HipAdam(ps, lr=1e-2)

    def fn(i):
        for j, p in enumerate(ps):
            p.grad = gs[j]
            opt.state[p] = dict(step=torch.tensor(3.0), exp_avg=ms[j], exp_avg_sq=vs[j])
        opt.step()
        return [[p.detach() for p in ps], ms, vs]
    return [p.data for p in ps] + gs + ms + vs, fn


A_CASES = [
    Case("linear f32 M=65", _a_linear_f32),
    Case("linear three-bf16-term M=8256 (LinW.pk + GEMM)", _a_linear_split),
    *[Case(f"wgrad side M={M} k2={k2} + SideStream.join", _a_wgrad(M, k2)) for M in (100, 5000) for k2 in (0, 83)],
    *[Case(f"gather_sum {k}", _a_gather(k)) for k in ("plain", "masked", "adds", "row0_partial", "multi", "dropmask")],
    Case("gather_diff", _a_gather_diff),
    Case("segment_mean_fwd", _a_segment_mean_fwd),
    Case("segment_mean_bwd", _a_segment_mean_bwd(False)),
    Case("segment_mean_bwd masked", _a_segment_mean_bwd(True)),
    Case("head_fwd", _a_head(False)),
    Case("head_bwd", _a_head(True)),
    Case("dropout", _a_dropout),
    Case("relu_bwd", _a_relu_bwd),
    Case("axpby", _a_axpby),
    Case("weighted_colsum", _a_weighted_colsum),
    Case("rr_amax_f32", _a_amax),
    Case("rr_ffn_chain_f32 forward", _a_ffn_chain(False)),
    Case("rr_ffn_chain_f32 backward", _a_ffn_chain(True)),
    Case("LinW.pk (f32 layout) + GEMM", _a_pack_then_gemm(False)),
    Case("LinW.pk_t + GEMM", _a_pack_then_gemm(True)),
    Case("rr_build_fbonds_f32", _a_build_fbonds),
    Case("HipAdam.step 1/1025/4096", _a_adam),
]


@pytest.mark.parametrize("case", A_CASES, ids=lambda c: c.name)
def test_a_per_op_entry_points(case, parity_log):
    with gemm(f16=False):
        assert run(case, parity_log).status == "armed"


# ============================================================================================== B. losses
B_SCOPE = [1, 2, 3, 32, 64, 65, 129]


def _b_loss(kind):
    def build():
        scope = [5, 5, 5, 5] if kind == "betanet" else B_SCOPE
        M = sum(scope)
        cols = 2 if kind in ("evidential_ranking", "task mle_gaussian") else 1
        x = rnd(110, M, cols, positive=True) if cols == 2 else rnd(110, M, positive=True)
        t = rnd(111, M)

        def fn(i):
            s = i[0].detach().requires_grad_(True)
            if kind == "mle":
                l = RL.MLEloss()(s, scope, i[1], 0)
            elif kind == "listnet":
                l = RL.ListnetLoss()(s, scope, i[1], 0)
            elif kind == "evidential_ranking":
                l = RL.evidential_ranking()(s, scope, i[1], None, None, None, 0)
            elif kind == "ranknet":
                l = RL.ranknet_loss(s, scope, i[1], 1.0, 0)[0]
            elif kind == "lambdarank":
                l = RL.lambdarank_loss(s, scope, i[1], 1.0, 10, 0, pairs=RL.sq_pairs(scope))[0]
            elif kind == "approx_ndcg":
                l = RL.approx_ndcg_loss(s, scope, i[1], 0.5, 10, 0, queries=len(scope))[0]
            elif kind == "task mle_gaussian":
                l = RL.task_step_loss("mle_gaussian", s, scope, i[1], 0, coef=0.25)
                assert l is not None
            else:
                l = RL.betanet_loss(s, scope, i[1], 100.0, 0)[0]
            RL.backward(l)
            return [l, s.grad]
        return [x, t], fn
    return build


B_CASES = [Case(k, _b_loss(k)) for k in ("mle", "listnet", "evidential_ranking", "ranknet", "lambdarank", "approx_ndcg",
                                         "task mle_gaussian", "betanet")]


@pytest.mark.parametrize("case", B_CASES, ids=lambda c: c.name)
def test_b_losses(case, parity_log):
    assert run(case, parity_log).status == "armed"


def test_b_fused_listmle_on_two_streams_at_once_uses_two_ticket_words(parity_log):
    """The step kernels finish through a ticket word that must be zero on entry: one word per (device, stream), because two
    streams' launches are not ordered.  One stream is delayed, the other is not; both must give the default stream's bits."""
    M = sum(B_SCOPE)
    xs, ts = [rnd(120 + j, M) for j in range(2)], [rnd(122 + j, M) for j in range(2)]

    def step(j):
        s = xs[j].detach().requires_grad_(True)
        l = RL.MLEloss()(s, B_SCOPE, ts[j], 0)
        RL.backward(l)
        return l.detach(), s.grad

    want = [step(0), step(1)]
    torch.cuda.synchronize()
    a, b = S.concurrent_pair(lambda: step(1), log=parity_log)
    S.spin(a, S.MIN_DELAY_MS)
    with torch.cuda.stream(a):
        behind = torch.cuda.Event()
        behind.record(a)
        ga = step(0)
    with torch.cuda.stream(b):
        gb = step(1)
    armed = not behind.query()
    torch.cuda.synchronize()
    parity_log(f"two-stream ListMLE: delayed stream {'armed' if armed else 'not armed'}")
    assert armed
    words = [RL.FusedStep._counter[(str(xs[0].device), q.cuda_stream)] for q in (a, b)]
    assert words[0].data_ptr() != words[1].data_ptr()
    for got, ref in ((ga, want[0]), (gb, want[1])):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert int(words[0]) == 0 and int(words[1]) == 0


# ============================================================================================== C. evaluation kernels
C_SCOPE = [1, 2, 7, 33, 64]


def _c_scored(fn_of):
    def build():
        M = sum(C_SCOPE)
        s, t = rnd(130, M), rnd(131, M)
        return [s, t], lambda i: fn_of(i[0], i[1])
    return build


def _c_sample_stats():
    M = sum(C_SCOPE)
    x, t = rnd(132, 7, M), rnd(133, M)
    return [x, t], lambda i: UQ.sample_stats(i[0], C_SCOPE, i[1], 0)


def _c_analytic(kind):
    """rr_analytic_rank_stats_f32 through the C entry point: the wrapper (uncertainty.analytic_stats) reads its result back to
    validate it, which blocks the host, so the launch itself is what can be held behind a delay"""
    def build():
        M, Q = sum(C_SCOPE), len(C_SCOPE)
        cols = 4 if kind == "nig" else 2
        x = rnd(134, M, cols, positive=True)
        if kind == "nig":
            x[:, 2] += 1.0                                        # alpha > 1
        t = rnd(135, M)
        _, seg, total, max_len, _ = RL._prep(x[:, 0], C_SCOPE, t, 0)
        nodes, weights = UQ._device_quadrature(32, x.device)
        nig = kind == "nig"

        def fn(i):
            outs = [torch.empty(M, dtype=torch.float32, device=DEV) for _ in range(6 if nig else 4)]
            qstats = torch.empty(Q, UQ.NQSTATS, dtype=torch.float64, device=DEV)
            mass = torch.empty(Q, dtype=torch.float64, device=DEV)
            check(lib().rr_analytic_rank_stats_f32(ptr(i[0]), i[0].stride(0), UQ.MOMENT_KINDS[kind], ptr(i[1]), ptr(seg), Q,
                                                   max_len, ptr(nodes), ptr(weights), 32, *[ptr(o) for o in outs],
                                                   *([] if nig else [None, None]), ptr(qstats), ptr(mass), stream()),
                  "rr_analytic_rank_stats_f32")
            return [outs, qstats, mass]
        return [x, t], fn
    return build


def _c_top1_sets():
    """rr_top1_sets_f32 through the C entry point (uncertainty.top1_sets validates its inputs on the host first)"""
    M, Q = sum(C_SCOPE), len(C_SCOPE)
    p, t = rnd(136, M, positive=True, scale=0.05), rnd(137, M)
    _, seg, total, max_len, _ = RL._prep(p, C_SCOPE, t, 0)

    def fn(i):
        rank = torch.empty(M, dtype=torch.int32, device=DEV)
        before = torch.empty(M, dtype=torch.float64, device=DEV)
        in_set = torch.empty(M, dtype=torch.uint8, device=DEV)
        stats = torch.empty(Q, UQ.TOP1_NSTATS, dtype=torch.float64, device=DEV)
        check(lib().rr_top1_sets_f32(ptr(i[0]), 1, ptr(i[1]), ptr(seg), Q, max_len, 0.4, ptr(rank), ptr(before), ptr(in_set),
                                     ptr(stats), stream()), "rr_top1_sets_f32")
        return [rank, before, in_set, stats]
    return [p, t], fn


def _c_calibration():
    n = 3000
    pred, tgt, std = rnd(138, n), rnd(139, n), rnd(140, n, positive=True)

    def fn(i):
        r = UQ.probabilistic_calibration(i[0], i[1], i[2], n_bins=20)
        return [torch.tensor([r["nll"], r["crps"], r["z_mean"], r["z2_mean"], r["sharpness"], r["rmse"]], dtype=torch.float64),
                torch.from_numpy(r["pit_hist"])]
    return [pred, tgt, std], fn


MODEL = {}


def model_case(Hd=32, p=0.1, train=True, dedup="auto", scope=(7, 3, 9, 5), seed=17, wseed=5):
    """a model and a batch as tests/test_gpu_plan.py builds them, with add_features and targets on the device"""
    key = (Hd, p, train, dedup, tuple(scope), seed, wseed)
    if key not in MODEL:
        from tests.test_gpu_model import make_model
        cfg = dict(hidden_size=Hd, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, task_num=1,
                   ffn_last_layer="with_softplus", task_type=None, add_features_dim=1)
        w = synth.seeded_weights(O.model_shapes(Hd, 3, 3, 3, 1, 1, True), wseed)
        model = make_model(cfg, w, dropout=p)
        model = model.train() if train else model.eval()
        model.dedup_reactants = dedup
        qb = synth.make_queries(seed, len(scope), list(scope), atoms_lo=5, atoms_hi=14)
        rb, pb = featurization.BatchMolGraph(qb.r_specs, K=4), featurization.BatchMolGraph(qb.p_specs, K=4)
        add = torch.tensor(np.asarray(qb.add_features), dtype=torch.float32).to(DEV)
        tg = torch.tensor(np.asarray(qb.targets), dtype=torch.float32).to(DEV)
        MODEL[key] = dict(model=model, qb=qb, rb=rb, pb=pb, add=add, tg=tg, w=w, scope=list(scope), p=p)
    return MODEL[key]


def graphs_of(mc):
    gs = [mc["rb"].device_graph(0), mc["pb"].device_graph(0)]
    ub = mc["rb"].unique()[0]
    if ub.n_mols < mc["rb"].n_mols:
        gs.append(ub.device_graph(torch.device(DEV)))
    return gs


def model_floats(mc):
    """everything float a step reads: the parameters, the atom / bond features of every graph, add_features, the targets"""
    ins = [q.data for q in mc["model"].flat_params() if q is not None]
    for g in graphs_of(mc):
        ins += [g.f_atoms, g.f_bonds]
    return ins + [mc["add"], mc["tg"]]


def forget_derived(mc):
    for g in graphs_of(mc):
        g._fb_sum = None                                           # sum of f_bonds over an atom's bonds: cached per batch


def _c_input_gradients():
    mc = model_case(p=0.0, train=False)

    def fn(i):
        forget_derived(mc)
        return attribution.input_gradients(mc["model"], mc["rb"], mc["pb"], add_features=mc["add"], column=0, gpu=0)
    return model_floats(mc)[:-1], fn


C_CASES = [
    Case("rr_ranking_metrics_f32 (ranking_stats)", _c_scored(lambda s, t: list(EV.ranking_stats(s, C_SCOPE, t, 0)))),
    Case("rank_correlation_stats", _c_scored(lambda s, t: EV.rank_correlation_stats(s, C_SCOPE, t, 0))),
    Case("rr_mc_sample_stats_f32 T=7", _c_sample_stats),
    Case("rr_analytic_rank_stats_f32 gaussian", _c_analytic("gaussian")),
    Case("rr_analytic_rank_stats_f32 nig", _c_analytic("nig")),
    Case("rr_top1_sets_f32", _c_top1_sets),
    Case("attribution.input_gradients H=32", _c_input_gradients),
    Case("probabilistic_calibration", _c_calibration, True, "returns Python numbers: it reads the sums back before it returns"),
]


@pytest.mark.parametrize("case", C_CASES, ids=lambda c: c.name)
def test_c_evaluation_kernels(case, parity_log):
    with gemm(f16=False):
        assert run(case, parity_log).status == ("exempt" if case.host_sync else "armed")


# ============================================================================================== D. whole model
def train_step(mc, seed, plan=True):
    """forward, ListMLE, backward -> scores, loss, every gradient (the tensors themselves: the caller clones)"""
    model = mc["model"]
    old = Fn.StepPlan.enabled
    Fn.StepPlan.enabled = plan
    try:
        forget_derived(mc)
        model.zero_grad()
        model.dropout_seed = seed
        out = model(mc["rb"], mc["pb"], gpu=0, add_features=mc["add"])
        l = RL.MLEloss()(out, mc["scope"], mc["tg"], 0)
        RL.backward(l)
        return dict(scores=out.detach(), loss=l.detach(), grads={k: q.grad for k, q in model.named_parameters() if q.grad is not None})
    finally:
        Fn.StepPlan.enabled = old


def _d_model(plan, mode, Hd=32, scope=(7, 3, 9, 5)):
    def build():
        kw = dict(train=dict(p=0.1, train=True), eval=dict(p=0.0, train=False), nodedup=dict(p=0.1, train=True, dedup=False))[mode]
        mc = model_case(Hd=Hd, scope=scope, **kw)
        return model_floats(mc), lambda i: train_step(mc, 4242, plan)
    return build


D_MODES = ("train", "eval", "nodedup")
D_CASES = ([Case(f"{'plan' if plan else 'per-op'} {m} H=32", _d_model(plan, m)) for plan in (True, False) for m in D_MODES] +
           [Case(f"plan f16x2 {m} H=32", _d_model(True, m)) for m in D_MODES] +
           [Case("plan train H=300, 64 candidates", _d_model(True, "train", 300, (20, 12, 24, 8)))])


@pytest.mark.parametrize("case", D_CASES, ids=lambda c: c.name)
def test_d_whole_model(case, parity_log):
    with gemm(f16="f16x2" in case.name):
        r = run(case, parity_log)
    assert r.status == "armed"
    ref = dict(r.ref)
    assert any(k.startswith("out.grads.") for k in ref) and "out.scores" in ref and "out.loss" in ref
    if case.name == "plan train H=32":
        # the reference run is not the library against itself alone: tests/test_gpu_model.py's comparison with the oracle
        from tests.test_gpu_model import _masks_for, close
        mc = model_case(p=0.1, train=True)
        qb = mc["qb"]
        masks = _masks_for(mc["model"], 4242, mc["rb"], mc["pb"], len(qb.p_specs), 1, 0.1)
        want = O.reaction_forward(O.params_from_numpy(mc["w"]), dict(depth=3, diff_depth=3, ffn_depth=3, task_type="with_softplus",
                                                                      dropout=0.1),
                                  O.pack_batch(qb.r_specs, K=4), O.pack_batch(qb.p_specs, K=4), qb.add_features, masks=masks)
        close(ref["out.scores"], want.detach(), tol=1e-5, what="staged reference scores against the oracle")


# ============================================================================================== E. steps without host synchronisation
def _e_steps(sync, on, parity_log):
    """four training steps (plan, H = 32, p = 0.1, HipAdam) on stream `on` -> the parameters before and afterwards"""
    from tests.test_gpu_model import make_model
    mcs = [model_case(seed=17), model_case(seed=23)]
    cfg = dict(hidden_size=32, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, task_num=1,
               ffn_last_layer="with_softplus", task_type=None, add_features_dim=1)
    model = make_model(cfg, mcs[0]["w"], dropout=0.1).train()
    opt = HipAdam(model.parameters(), lr=1e-3)
    before = [q.detach().clone() for q in model.parameters()]
    torch.cuda.synchronize()

    def maybe_sync():
        if sync:
            torch.cuda.synchronize()
    behind = None
    if not sync:
        S.spin(on, S.MAX_DELAY_MS)
    with torch.cuda.stream(on):
        if not sync:
            behind = torch.cuda.Event()
            behind.record(on)
        for k in range(4):
            mc = mcs[k % 2]
            forget_derived(mc)
            model.zero_grad()
            model.dropout_seed = 500 + k
            out = model(mc["rb"], mc["pb"], gpu=0, add_features=mc["add"])
            maybe_sync()
            l = RL.MLEloss()(out, mc["scope"], mc["tg"], 0)
            maybe_sync()
            RL.backward(l)
            maybe_sync()
            opt.step()
            maybe_sync()
            if k == 0 and behind is not None:
                assert not behind.query(), "the delay ended before the first step was enqueued"
        if behind is not None:
            parity_log(f"four unsynchronised steps: delay {'still' if not behind.query() else 'no longer'} pending after the last enqueue")
        params = [q.detach().clone() for q in model.parameters()]
    torch.cuda.synchronize()
    return before, params


def test_e_four_steps_without_a_host_synchronisation_equal_the_synchronised_steps(parity_log, monkeypatch):
    monkeypatch.setattr(Fn.WgradOrder, "mode", "late")
    with gemm(f16=False):
        start, want = _e_steps(True, torch.cuda.current_stream(), parity_log)
        _, got = _e_steps(False, torch.cuda.Stream(), parity_log)
    assert len(want) == len(got) == len(start)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    moved = sum(not torch.equal(a, b) for a, b in zip(start, want))
    assert moved >= len(start) - 2                                 # the steps did move every trained parameter (two constants are not trained)


# ============================================================================================== F. two caller streams
def _cloned(step):
    return dict(scores=step["scores"].clone(), loss=step["loss"].clone(), grads={k: v.clone() for k, v in step["grads"].items()})


def _diff(a, b):
    """labels of what differs between two train_step results"""
    bad = [k for k in ("scores", "loss") if not torch.equal(a[k], b[k])]
    return bad + [k for k in a["grads"] if not torch.equal(a["grads"][k], b["grads"][k])]


@contextlib.contextmanager
def pool_spy():
    """records (bytes asked for, bytes of the buffer handed out, its address) of every _WorkspacePool.take for the duration"""
    P = Fn._WorkspacePool
    o_take = P.__dict__["take"]
    calls = []

    def take(cls, nbytes, device):
        t = o_take.__func__(cls, nbytes, device)
        calls.append((int(nbytes), t.numel(), t.data_ptr()))
        return t
    P.take = classmethod(take)
    try:
        yield calls
    finally:
        P.take = o_take


def pool_scenario(log=None):
    """F(i): step 1's backward is enqueued behind a delay on stream A - its workspace is back in the pool while nothing of it
    has run - and stream B, not delayed, runs forwards of another batch whose workspace fits into that buffer.  -> dict:
    bad (what differs in step 1's result), b_grad / b_nograd (whether B's scores differ, with grad and under no_grad), armed
    (the delay was still pending when everything was enqueued), fits (B's request would fit A's buffer: the scenario is the
    one described), reused (B was handed A's buffer)"""
    mA, mB = model_case(seed=17), model_case(seed=29)
    model = mA["model"]

    def forward(mc, seed):
        forget_derived(mc)
        model.dropout_seed = seed
        return model(mc["rb"], mc["pb"], gpu=0, add_features=mc["add"])

    with pool_spy() as calls:
        with torch.no_grad():
            forward(mA, 900)
            forward(mB, 901)
    if calls[0][0] < calls[1][0]:                                  # step 1 is the batch with the larger workspace: B's then fits
        mA, mB = mB, mA
    want = _cloned(train_step(mA, 900))
    want_b = forward(mB, 901).detach().clone()
    torch.cuda.synchronize()
    old_free = Fn._WorkspacePool.free
    try:
        def probe():
            with torch.no_grad():
                forward(mB, 901)
        A, B = S.concurrent_pair(probe, log=log)                   # B's forward, helper streams included, must not queue behind A
        Fn._WorkspacePool.free = []                                # the scenario starts from an empty pool
        with pool_spy() as calls:
            with torch.cuda.stream(A):
                model.zero_grad()
                out = forward(mA, 900)
                l = RL.MLEloss()(out, mA["scope"], mA["tg"], 0)
            torch.cuda.synchronize()
            S.spin(A, S.MAX_DELAY_MS)
            with torch.cuda.stream(A):
                behind = torch.cuda.Event()
                behind.record(A)
                RL.backward(l)                                     # enqueued; the pool has the workspace again
            with torch.cuda.stream(B):
                b1 = forward(mB, 901)
                with torch.no_grad():
                    b2 = forward(mB, 901)
            armed = not behind.query()
            torch.cuda.synchronize()
        got = dict(scores=out.detach(), loss=l.detach(), grads={k: q.grad for k, q in model.named_parameters() if q.grad is not None})
        res = dict(bad=_diff(want, got), b_grad=not torch.equal(b1.detach(), want_b), b_nograd=not torch.equal(b2, want_b),
                   armed=armed, fits=calls[1][0] <= calls[0][1], reused=calls[1][2] == calls[0][2])
    finally:
        Fn._WorkspacePool.free = old_free
    if log is not None:
        log(f"F(i) pool scenario: delay {'armed' if armed else 'not armed'}; A's buffer {calls[0][1]} bytes, B asks for {calls[1][0]}"
            f" and {'is' if res['reused'] else 'is not'} handed A's buffer; step 1 differs in {len(res['bad'])} tensors; "
            f"B's scores differ: with grad {res['b_grad']}, no_grad {res['b_nograd']}")
    return res


def test_f_a_workspace_given_back_on_one_stream_is_not_handed_to_another(parity_log):
    """Fails with a pool that keeps one free list for all streams: B's forward then takes the workspace of A's pending backward
    and overwrites the activations that backward has yet to read."""
    with gemm(f16=False):
        r = pool_scenario(parity_log)
    assert r["armed"] and r["fits"]
    assert not r["reused"]
    assert r["bad"] == [] and not r["b_grad"] and not r["b_nograd"]


def test_f_two_training_steps_interleaved_on_two_streams_equal_their_serial_runs(parity_log):
    """A forward, B forward, A backward, B backward with a delay in front of A: the two callers share the device's side and aux
    streams, which wait for each caller in turn."""
    ma, mb = model_case(seed=17), model_case(seed=31, wseed=6)
    assert ma["model"] is not mb["model"]
    with gemm(f16=False):
        want = [_cloned(train_step(ma, 910)), _cloned(train_step(mb, 911))]
        torch.cuda.synchronize()
        A, B = S.concurrent_pair(lambda: train_step(mb, 911), log=parity_log)
        S.spin(A, S.MAX_DELAY_MS)
        outs, losses = {}, {}
        with torch.cuda.stream(A):
            behind = torch.cuda.Event()
            behind.record(A)
        for tag, q, mc, seed in (("a", A, ma, 910), ("b", B, mb, 911)):
            with torch.cuda.stream(q):
                forget_derived(mc)
                mc["model"].zero_grad()
                mc["model"].dropout_seed = seed
                outs[tag] = mc["model"](mc["rb"], mc["pb"], gpu=0, add_features=mc["add"])
                losses[tag] = RL.MLEloss()(outs[tag], mc["scope"], mc["tg"], 0)
        for tag, q in (("a", A), ("b", B)):
            with torch.cuda.stream(q):
                RL.backward(losses[tag])
        armed = not behind.query()
        torch.cuda.synchronize()
    parity_log(f"F(ii) interleaved steps: delay {'armed' if armed else 'not armed'}")
    assert armed
    for tag, mc, ref in (("a", ma, want[0]), ("b", mb, want[1])):
        got = dict(scores=outs[tag].detach(), loss=losses[tag].detach(),
                   grads={k: q.grad for k, q in mc["model"].named_parameters() if q.grad is not None})
        assert _diff(ref, got) == [], tag


# ============================================================================================== G. shard prefetcher
def test_g_streamed_steps_consumed_off_the_default_stream_equal_the_in_memory_steps(tmp_path, parity_log):
    """four steps through two slots (every slot is reused), the consumer on its own stream with a delay in front of step 2: the
    slots are released with events on the consumer's stream, so the copy stream may not overwrite a slot that step still reads"""
    from tests.test_gpu_shards import _make_steps, _model, _run
    steps = _make_steps(4, [6, 3, 8, 2])
    path = str(tmp_path / "epoch.rrshard")
    with shards.ShardWriter(path) as w:
        for qb, rb, pb in steps:
            w.add_step(rb, pb, qb.scope, qb.targets, qb.add_features)
    reader = shards.ShardReader(path)
    with gemm(f16=False):
        model = _model(0.15, True)
        want = [_run(model, rb, pb, qb.scope, torch.tensor(qb.targets).to(DEV), torch.tensor(np.asarray(qb.add_features)).to(DEV), 1000 + i)
                for i, (qb, rb, pb) in enumerate(steps)]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        pf = shards.StepPrefetcher(reader, DEV, [0, 1, 2, 3], depth=2)
        got, behind = [], None
        with torch.cuda.stream(s):
            for n, st in enumerate(pf):
                if n == 1:
                    S.spin(s, S.MAX_DELAY_MS)
                    behind = torch.cuda.Event()
                    behind.record(s)
                got.append(_run(model, st["r"], st["p"], st["scope"], st["targets"], st["add"], 1000 + st["index"]))
        pending = not behind.query()
        torch.cuda.synchronize()
        pf.close()
    parity_log(f"G prefetcher: delay {'still' if pending else 'no longer'} pending after the last step was enqueued")
    assert len(got) == 4
    for a, b in zip(want, got):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].keys() == b[2].keys()
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), k


SECTIONS = {"A": A_CASES, "B": B_CASES, "C": C_CASES, "D": D_CASES}
