"""Timing of the attributions on the headline batch: 64 queries x 64 candidates, H = 300, depth 3.
  (a) the fused W_i call of rr_input_attribution_f32 (adjoint of W_i, product by f_bonds and the two segment sums in one
      launch) next to the two-step form it replaces: linear(nB, 83, Wi.pk_t(0, 83), a1=d_inp, k1=H), then a torch row-dot;
  (b) attribute(..., "grad_x_input") next to one per-op training step (forward + ListMLE + backward, no step plan) of the same
      batch in the same process - with the reactants de-duplicated as training does at p = 0 ("auto") and without;
  (c) attribute(..., "integrated_gradients", steps=16).
    python tools/attribution_bench.py [--out profiles/attribution_bench.txt] [--queries 64 --cands 64 --hidden 300]
Timed with device events around back-to-back calls, enough of them for a window of about 0.3 s, after a warm-up of the same
shape; each figure is the median of five such windows with the lowest and highest next to it; the two sides of (a) and of (b)
alternate window by window.  The achieved rates of (a) use the operations and bytes the algorithm needs, computed from the
shapes: 2 M N K flops over the 83 real columns, dz and x read once, w once.  No threshold: the numbers are recorded, not
asserted.  Needs a GPU: without one the first device call raises."""
import argparse, os, sys, statistics
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from oracle import ref_cpu as O
from reactranker_amd import attribution as A, featurization, functions as Fn, synth
from reactranker_amd import loss as RL
from reactranker_amd.base_model import build_model

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the printed lines to this file")
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--cands", type=int, default=64)
ap.add_argument("--hidden", type=int, default=300)
ARGS = ap.parse_args()
LINES = []
PEAK_TF, PEAK_TBS = 157.3, 6.29          # f32 matrix rate (spec), measured copy bandwidth


def say(line):
    print(line, flush=True)
    LINES.append(line)


def sync_time(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                              # microseconds per call


def t_alternating(fns, reps=5, window_us=3e5):
    """median, min, max (us per call) of every fn, their windows alternating"""
    ns = []
    for fn in fns:
        for _ in range(3):
            fn()
        ns.append(int(min(4000, max(3, window_us / max(sync_time(fn, 3), 1.0)))))
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            out[k].append(sync_time(fn, ns[k]))
    return [(statistics.median(o), min(o), max(o), n) for o, n in zip(out, ns)]


def fmt(t):
    return f"{t[0]:10.1f} us  (min {t[1]:.1f}, max {t[2]:.1f}; {t[3]} calls per window)"


def main():
    H = ARGS.hidden
    torch.cuda.set_device(0)
    qb = synth.make_queries(7, ARGS.queries, ARGS.cands)
    rb, pb = featurization.BatchMolGraph(qb.r_specs), featurization.BatchMolGraph(qb.p_specs)
    w = synth.seeded_weights(O.model_shapes(H, 3, 3, 3, 1, 1, True), 1)
    model = build_model(hidden_size=H, mpnn_depth=3, mpnn_diff_depth=3, ffn_depth=3, use_bias=True, dropout=0.0, task_num=1,
                        ffn_last_layer="with_softplus", add_features_dim=1)
    model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    model = model.cuda()
    pg = featurization.device_graph_of(pb, 0)
    nB, nA, M = pg.nB, pg.nA, pg.M
    say(f"torch {torch.__version__}; {ARGS.queries} queries x {ARGS.cands} candidates, H = {H}, depth 3 / 3: "
        f"{M} candidates, {nA} atom rows, {nB} directed-bond rows per graph")

    # ---- (a) the fused W_i call against the two-step form
    g = torch.Generator(device="cuda").manual_seed(0)
    d_inp = torch.randn(nB, H, device="cuda", generator=g)
    Wi = Fn.LinW(model.encoder.W_i.weight, model.encoder.W_i.bias)
    attr = torch.empty(nB, 2, device="cuda")
    x = pg.f_bonds

    def fused():
        A.input_attribution(d_inp, Wi.w, 83, x=x, segments=(61, 83), attr=attr)

    def two_step():
        dX = Fn.linear(nB, 83, Wi.pk_t(0, 83), w_packed=True, a1=d_inp, k1=H)
        pr = dX[:, :83] * x[:, :83]
        return torch.stack([pr[:, :61].sum(1), pr[:, 61:].sum(1)], 1)

    ta, tb = t_alternating([fused, two_step])
    flops, nbytes = 2.0 * nB * H * 83, 4.0 * (nB * H + nB * 83 + H * 83 + nB * 2)
    floor = max(flops / (PEAK_TF * 1e12), nbytes / (PEAK_TBS * 1e12)) * 1e6
    say(f"(a) W_i adjoint x f_bonds, M = {nB}, N = {H}, K = 83 (segments 61 | 83)")
    say(f"  {'rr_input_attribution_f32 (one launch)':52s} {fmt(ta)}")
    say(f"      {flops / ta[0] * 1e-6:.1f} TFLOP/s, {nbytes / ta[0] * 1e-6:.2f} TB/s of algorithmic traffic; the hardware floor "
        f"({'flops' if flops / (PEAK_TF * 1e12) > nbytes / (PEAK_TBS * 1e12) else 'bytes'} bound) is {floor:.1f} us: {100 * floor / ta[0]:.0f} % of it")
    say(f"  {'linear(pk_t) + torch row-dot (two-step form)':52s} {fmt(tb)}   {tb[0] / ta[0]:.2f}x the launch")
    fused()
    ref = two_step()
    say(f"  fused against two-step on this batch: max |difference| {float((ref - attr).abs().max()):.2e}, "
        f"largest value {float(ref.abs().max()):.2e}")

    # ---- (b) grad_x_input against one per-op training step
    targets = torch.tensor(qb.targets)
    lossf = RL.MLEloss()
    Fn.StepPlan.enabled = False

    def train_step():
        model.zero_grad(set_to_none=True)
        out = model(rb, pb, gpu=0, add_features=qb.add_features)
        lossf(out, qb.scope, targets, 0).sum().backward()

    def gxi():
        return A.attribute(model, rb, pb, qb.add_features, method="grad_x_input", gpu=0)

    model.train()
    model.dedup_reactants = "auto"
    t_gxi, t_auto = t_alternating([gxi, train_step])
    model.dedup_reactants = False
    _, t_plain = t_alternating([gxi, train_step])
    model.dedup_reactants = "auto"
    Fn.StepPlan.enabled = True
    say("(b) whole calls on the same batch, same process, no step plan on either side")
    say(f"  {'attribute(grad_x_input)':52s} {fmt(t_gxi)}")
    say(f"  {'per-op training step, reactants de-duplicated':52s} {fmt(t_auto)}   attribute is {t_gxi[0] / t_auto[0]:.2f}x of it")
    say(f"  {'per-op training step, one reactant per candidate':52s} {fmt(t_plain)}   attribute is {t_gxi[0] / t_plain[0]:.2f}x of it")

    # ---- (c) integrated gradients, 16 nodes
    def ig():
        return A.attribute(model, rb, pb, qb.add_features, method="integrated_gradients", steps=16, gpu=0)

    t_ig, = t_alternating([ig], reps=3)
    res = ig()
    say(f"(c) {'attribute(integrated_gradients, steps=16)':48s} {fmt(t_ig)}   {t_ig[0] / t_gxi[0]:.1f}x grad_x_input")
    say(f"  max |gap| {float(res['gap'].abs().max()):.2e} at max |score - baseline| "
        f"{float((res['score'] - res['baseline_score']).abs().max()):.2e}")
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


main()
