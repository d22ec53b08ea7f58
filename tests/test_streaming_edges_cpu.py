"""tests/streaming_edges.py itself, without a GPU: the grid constants are found in the sources and every size lands in the
class it is named for; the table is complete; the planted values are in the generated inputs; the numpy and the whole-tensor
restatements of the elementwise kernels give the same bits and stay within a float32 chain's distance of float64; the Adam
restatement is torch.optim.Adam; the float32 CPU evaluation of every loss case keeps tests/loss_range.py's rule at its
1e-5 bound."""
import numpy as np
import pytest
import torch

from tests import loss_range as L
from tests import streaming_edges as S


def test_the_grid_constants_are_in_the_sources():
    c = S.constants()
    assert c["num_cu"] == 256 and c["grid_cap"] == 8192 and c["pointwise_cap"] == 1024 and c["amax_cap"] == 1024
    assert c["max_adds"] == 15 and c["max_adam"] == 64 and c["adam_block"] == 1024
    assert (c["amax_lanes"], c["amax_stride"]) == (16, 32)
    assert S.ONE_PASS == 2_097_152 and S.POINT_PASS == 262_144
    assert S.WRAP_SCALAR == 2 * 2_097_152 + 77 and S.WRAP_VEC == 4 * (2_097_152 + 1000) + 3
    assert S.POINTWISE == (65_536, 262_144, 262_145, 600_003)


def test_every_size_lands_in_its_class():
    for vector in (False, True):                                           # everything below "wrap" is one pass
        for n in S.TINY + (S.TODAY,):
            assert S.stream_class(n, vector)["passes"] == 1
    assert {n % 4 for n in S.TINY} == {0, 1, 2, 3}
    assert S.stream_class(S.TODAY, True)["tail"] == 2
    assert S.stream_class(S.WRAP_SCALAR, False) == dict(passes=3, partial=True, tail=0)
    assert S.stream_class(S.WRAP_VEC, True) == dict(passes=2, partial=True, tail=3)
    assert S.stream_class(S.ONE_PASS, False)["passes"] == 1 and S.stream_class(4 * S.ONE_PASS, True)["passes"] == 1
    want = [dict(passes=1, partial=False, partials=256), dict(passes=1, partial=False, partials=1024),
            dict(passes=2, partial=True, partials=1024), dict(passes=3, partial=True, partials=1024)]
    assert [S.point_class(n) for n in S.POINTWISE] == want
    assert max(hi - lo for n in S.POINTWISE for lo, hi in S.slices(n)) == S.POINT_PASS
    for n in S.POINTWISE:                                                  # slices: a partition into powers of two, one pass each
        sl = S.slices(n)
        assert sl[0][0] == 0 and sl[-1][1] == n and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all((hi - lo) & (hi - lo - 1) == 0 and S.point_class(hi - lo)["passes"] == 1 for lo, hi in sl)
    for head in S.HEAD_GROUPS:
        M, N = S.head_shapes(head, "wrap")[0]
        assert N % S.HEAD_GROUPS[head] == 0 and S.stream_class(M * N, False)["passes"] == 3
        assert S.stream_class(M * N, False)["partial"]
    assert (S.HEAD_ROWS, 8) in S.head_shapes(6, "wrap") and (1, 8) in S.head_shapes(6, "wrap")
    assert (S.HEAD_ROWS, 2) in S.head_shapes(3, "wrap") and (1, 2) in S.head_shapes(3, "wrap")
    assert S.stream_class(S.HEAD_ROWS * 8, False) == dict(passes=2, partial=True, tail=0)
    # amax: one vector and two scalar shapes past four strides of the capped grid by a partial stride, one below three
    v = S.amax_plan(*S.AMAX_WRAP["aligned"], 0)
    assert v["vec"] and v["cls"] == "past_four_strides" and v["tail"] == 3 and v["stride"] == 262_144
    assert S.AMAX_WRAP["aligned"][2] > S.AMAX_WRAP["aligned"][1]           # the last chunk of a row holds a pad column
    for align, off in (("all_off_1", 1), ("ld_odd", 0)):
        s = S.amax_plan(*S.AMAX_WRAP[align], off)
        assert not s["vec"] and s["cls"] == "past_four_strides" and s["stride"] == 262_144
    for off, ld in ((0, 100), (1, 100), (0, 101)):
        assert S.amax_plan(S.AMAX_BELOW[0], S.AMAX_BELOW[1], ld, off)["cls"] == "below_three_strides"
    assert S.amax_plan(*S.AMAX_TODAY, 0)["vec"] and not S.amax_plan(*S.AMAX_TODAY, 2)["vec"]
    assert set(S.ADAM_SIZES) >= {S.constants()["adam_block"] + d for d in (-1, 0, 1)}
    assert {c > S.constants()["max_adam"] for c in S.ADAM_COUNTS} == {False, True} and S.constants()["max_adam"] + 1 in S.ADAM_COUNTS


def test_the_table_is_complete():
    cells = set(S.cells())
    wanted = {"rr_relu_bwd_f32", "rr_relu_bwd_sum_f32", "rr_axpby_f32", "rr_dropout_f32", "rr_head_fwd_f32", "rr_head_bwd_f32",
              "rr_amax_f32", "rr_digamma_f32", "rr_adam_step_f32"}
    wanted |= {f"rr_{k}_{d}_f32" for k in ("mse", "gauss_nll", "lognorm", "exp_mse", "nig") for d in ("fwd", "bwd")}
    assert set(S.ENTRY_POINTS) == wanted
    assert S.ENTRY_POINTS["rr_relu_bwd_f32"][0] == ("dz", "acc", "both")
    assert S.ENTRY_POINTS["rr_relu_bwd_sum_f32"][0] == (0, 1, 2, 15)
    assert {"b_null", "b_given"} <= set(S.ENTRY_POINTS["rr_axpby_f32"][0])
    assert S.ENTRY_POINTS["rr_head_fwd_f32"][0] == S.ENTRY_POINTS["rr_head_bwd_f32"][0] == tuple(range(7))
    two_forms = {"rr_relu_bwd_f32", "rr_relu_bwd_sum_f32", "rr_axpby_f32", "rr_amax_f32"}
    assert {e for e, (_, ops) in S.ENTRY_POINTS.items() if ops is not None} == two_forms
    missing, total = [], 0
    for entry, (forms, ops_of) in S.ENTRY_POINTS.items():
        for form in forms:
            classes = ("adam",) if entry == "rr_adam_step_f32" else ("zero", "tiny", "today", "wrap")
            for sc in classes:
                aligns = ["aligned"]
                if entry in two_forms and sc in ("tiny", "today"):
                    aligns += [f"off1:{op}" for op in ops_of(form)] + ["all_off_1", "all_off_2", "all_off_3"]
                if entry in two_forms and sc == "wrap":
                    aligns += ["all_off_1"]
                if entry == "rr_amax_f32" and sc != "zero":
                    aligns += ["ld_odd"]
                for al in aligns:
                    total += 1
                    if (entry, form, sc, al) not in cells:
                        missing.append((entry, form, sc, al))
                    else:
                        assert S.sizes(entry, form, sc, al), (entry, form, sc, al)
    assert sorted(map(str, missing)) == sorted(map(str, S.EXCLUDED)), missing
    assert all(isinstance(r, str) and r for r in S.EXCLUDED.values())
    assert 16 * len(S.EXCLUDED) <= total
    assert {c[0] for c in cells} == set(S.ENTRY_POINTS)                       # no entry point is excluded entirely
    # each operand in turn: acc, dz, out, b and one entry of adds are among the misaligned ones
    singles = {(c[0], c[3]) for c in cells if c[3].startswith("off1:")}
    for entry, op in (("rr_relu_bwd_f32", "acc"), ("rr_relu_bwd_f32", "dz"), ("rr_relu_bwd_f32", "dy"), ("rr_relu_bwd_f32", "y"),
                      ("rr_relu_bwd_sum_f32", "out"), ("rr_relu_bwd_sum_f32", "adds[7]"), ("rr_relu_bwd_sum_f32", "adds[0]"),
                      ("rr_axpby_f32", "b"), ("rr_axpby_f32", "a"), ("rr_axpby_f32", "out"), ("rr_amax_f32", "x")):
        assert (entry, "off1:" + op) in singles, (entry, op)
    for entry, form, sc, al in cells:
        if S.ENTRY_POINTS[entry][1] is not None:
            off = S.offsets(entry, form, al)
            assert set(off.values()) <= {0, 1, 2, 3}
            if al.startswith("off1:"):
                assert sorted(off.values()) == [0] * (len(off) - 1) + [1]
    # the elementwise wrap sizes: the vector form at WRAP_VEC, the scalar form at WRAP_SCALAR
    assert S.sizes("rr_axpby_f32", "b_null", "wrap", "aligned") == [S.WRAP_VEC]
    assert S.sizes("rr_axpby_f32", "b_null", "wrap", "all_off_1") == [S.WRAP_SCALAR]
    assert S.sizes("rr_dropout_f32", 0.5, "wrap", "aligned") == [S.WRAP_SCALAR]
    assert S.sizes("rr_mse_bwd_f32", "stride2", "wrap", "aligned") == list(S.POINTWISE)
    assert S.sizes("rr_digamma_f32", "values", "wrap", "aligned") == list(S.POINTWISE)


def test_every_cell_fits_the_time_budget_of_a_gpu_test():
    """one dry enumeration of the table: the launches, device words and host reference work of every cell, and the seconds
    budget_seconds() allows for them - a few seconds at the most, the whole file within two minutes"""
    table = S.dry_enumeration()
    assert set(table) == set(S.cells())
    per_entry, total = {}, 0.0
    for (entry, form, sc, al), work in table.items():
        sec = S.budget_seconds(*work)
        assert sec <= 3.0, (entry, form, sc, al, work, sec)
        per_entry[entry] = max(per_entry.get(entry, 0.0), sec)
        total += sec
    for entry, sec in sorted(per_entry.items()):
        print(f"[streaming edges] {entry}: the largest cell may take {sec:.2f} s")
    print(f"[streaming edges] {len(table)} cells, {sum(w[0] for w in table.values())} launches, {total:.0f} s in all")
    assert total <= 120.0


def test_the_planted_values_are_in_the_inputs():
    for n in S.TINY + (S.TODAY,):
        d = S.stream_inputs(n)
        plus, minus = S.plant_positions(n)
        assert plus and (minus or n <= 2)
        zero = S.bits_np(d["dy"])
        assert all(zero[i] == 0 and d["y"][i] > 0 for i in plus)
        assert all(zero[i] == np.int32(-2 ** 31) and d["y"][i] > 0 and S.bits_np(d["adds"][0])[i] == np.int32(-2 ** 31) for i in minus)
        # a negative alpha / scale makes -0 of the +0 entries: in the vector body (index 0) and in its tail (index n - 1)
        out = S.axpby_np(S.ALPHA, d["dy"], 0.0, None)
        assert all(S.bits_np(out)[i] == np.int32(-2 ** 31) for i in plus)
        assert all(S.bits_np(S.relu_bwd_np(d["dy"], d["y"], S.SCALE)[0])[i] == np.int32(-2 ** 31) for i in plus)
    d = S.stream_inputs(S.TODAY)
    assert 0.4 < float((d["y"] == 0).mean()) < 0.6
    assert S.TODAY % 4 != 0 and S.WRAP_VEC % 4 == 3                          # n - 1 lies in the tail of the vector form
    t = S.stream_inputs_t(S.TODAY, "cpu")
    assert 0.4 < float((t["y"] == 0).float().mean()) < 0.6 and len(t["adds"]) == 15
    assert int(t["dy"][:1].view(torch.int32)) == 0 and int(t["dy"][S.TODAY // 2:S.TODAY // 2 + 1].view(torch.int32)) == -2 ** 31
    assert S.ALPHA < 0 and S.SCALE < 0
    for v in (S.ALPHA, S.BETA, S.SCALE):
        assert float(np.float32(v)) == v
    # heads: both neighbours of 20, in every column
    twenty = np.float32(20.0)
    assert np.nextafter(twenty, np.float32(np.inf)) in S.HEAD_PLANTED and np.nextafter(twenty, np.float32(-np.inf)) in S.HEAD_PLANTED
    for head in S.HEAD_GROUPS:
        for sc in ("today", "wrap"):
            M, N = S.head_shapes(head, sc)[0]
            if sc == "wrap" and head not in (3, 6):
                continue                                                     # (the same generator; two wrap blocks are enough here)
            raw, _ = S.head_inputs(M, N)
            for v in S.HEAD_PLANTED:
                hit = (raw.view(np.int32) == np.float32(v).view(np.int32))
                assert hit.any(axis=0).all(), (head, sc, v)
    raw, _ = S.head_inputs(5, 4)                                             # fewer rows than values: as many as fit
    assert [int(b) for b in raw[:, 0].view(np.int32)] == [int(np.float32(v).view(np.int32)) for v in S.HEAD_PLANTED[:5]]
    # digamma: the root's neighbours, the specials, the integers and half-integers
    pts = S.digamma_points()
    root = np.float32(S.DIGAMMA_ROOT)
    ref = S.digamma_reference(np.array([np.nextafter(root, np.float32(0)), root, np.nextafter(root, np.float32(2))], np.float32))
    assert ref[0] < 0 < ref[2] and abs(ref[1]) < 1e-7                        # the float32 neighbours straddle the root
    for v in (np.nextafter(root, np.float32(0)), root, np.nextafter(root, np.float32(2)), np.finfo(np.float32).tiny, np.float32(1e-40),
              np.float32(0), np.float32(-1), np.float32(0.5), np.float32(60.0), np.float32(59.5), np.float32(1e-6), np.float32(1e6)):
        assert (pts.view(np.int32) == np.float32(v).view(np.int32)).any(), v
    assert 0 < np.float32(1e-40) < np.finfo(np.float32).tiny and len(pts) > 4000
    sp = S.digamma_reference(np.asarray(S.DIGAMMA_SPECIAL, np.float32))
    assert np.isneginf(sp[2]) and np.isnan(sp[3]) and np.isfinite(sp[:2]).all()
    for n in (5, S.TODAY):
        assert np.array_equal(S.digamma_input(n)[:4].view(np.int32), np.asarray(S.DIGAMMA_SPECIAL, np.float32)[:min(4, n)].view(np.int32))
    # amax: the planted positions lie in the valid region, one of them beside the pad columns
    rows, cols, ld = S.AMAX_WRAP["aligned"]
    pos = S.amax_positions(rows, cols)
    assert len(pos) == 33 and pos[0] == (0, 0) and pos[1] == (rows - 1, cols - 1) and pos[2][1] == cols - 1
    assert all(0 <= r < rows and 0 <= c < cols for r, c in pos)
    x = S.amax_block(7, 99, 101)
    assert (x[:, 99:] == S.AMAX_PAD).all() and S.amax_np(x, 99) < 10 and np.isfinite(S.amax_np(x, 99))


@pytest.mark.parametrize("n_adds", (0, 1, 2, 15))
def test_both_restatements_give_the_same_bits_and_stay_close_to_float64(n_adds):
    d = S.stream_inputs(S.TODAY)
    t = {k: (torch.from_numpy(np.array(v)) if k != "adds" else [torch.from_numpy(np.array(a)) for a in v]) for k, v in d.items()}
    got = S.relu_bwd_sum_np(d["dy"], d["y"], S.SCALE, d["adds"][:n_adds])
    dev = S.relu_bwd_sum_t(t["dy"], t["y"], S.SCALE, t["adds"][:n_adds]).numpy()
    assert np.array_equal(S.bits_np(got), S.bits_np(dev))
    exact, bound = S.relu_bwd_sum_f64(d["dy"], d["y"], S.SCALE, d["adds"][:n_adds])
    for a in (got, dev):
        assert (np.abs(a.astype(np.float64) - exact) <= bound).all()
    if n_adds == 0:
        dz, acc = S.relu_bwd_np(d["dy"], d["y"], S.SCALE, d["acc"])
        dz_t, acc_t = S.relu_bwd_t(t["dy"], t["y"], S.SCALE, t["acc"])
        assert np.array_equal(S.bits_np(dz), S.bits_np(dz_t.numpy())) and np.array_equal(S.bits_np(acc), S.bits_np(acc_t.numpy()))
        assert np.array_equal(S.bits_np(got), S.bits_np(np.float32(0) + dz))      # 0.f + the gated term: a gated -0 is +0 here
        for b_np, b_t in ((None, None), (d["b"], t["b"])):
            a = S.axpby_np(S.ALPHA, d["dy"], S.BETA, b_np)
            assert np.array_equal(S.bits_np(a), S.bits_np(S.axpby_t(S.ALPHA, t["dy"], S.BETA, b_t).numpy()))
            pa, pb = S.ALPHA * d["dy"].astype(np.float64), (0 if b_np is None else S.BETA * b_np.astype(np.float64))
            # two products and one sum, each rounded once: at most 2^-24 (|pa| + |pb| + |pa + pb|) (1 + 2^-24)
            assert (np.abs(a - (pa + pb)) <= 2.0 ** -23 * (1 + 2.0 ** -20) * (np.abs(pa) + np.abs(pb))).all()


def test_the_dropout_restatement():
    x = S.stream_inputs(S.TODAY)["dy"]
    assert np.array_equal(S.bits_np(S.dropout_np(x, 0.0, S.DROP_SEEDS[0])), S.bits_np(x))     # p = 0: x bit for bit, -0 included
    assert sum(s >= 2 ** 32 for s in S.DROP_SEEDS) >= 2
    for p in S.DROP_P[1:]:
        out = S.dropout_np(x, p, S.DROP_SEEDS[1])
        kept = float((out != 0).mean())
        assert abs(kept - (1 - p)) < 0.01, (p, kept)
        live = out != 0
        assert np.array_equal(out[live], x[live] * (np.float32(1) / (np.float32(1) - np.float32(p))))
    assert S.keep_scale(0.5) == 2 and S.keep_scale(0.0) == 1


@pytest.mark.parametrize("wd", S.ADAM_DECAYS)
def test_the_adam_restatement_is_torch_adam(wd):
    """adam_np over five steps against torch.optim.Adam on CPU float64 parameters, to the tolerance
    tests/test_gpu_ops.py::test_hip_adam_is_torch_adam_in_one_launch holds HipAdam to: 1e-6 of the largest entry"""
    rng = np.random.default_rng(3)
    ps = [rng.standard_normal(n).astype(np.float32) for n in S.ADAM_SIZES]
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    P = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p in ps]
    opt = torch.optim.Adam([{"params": P, "lr": 1e-4, "weight_decay": wd}])
    for step in range(1, 6):
        lr = 1e-4 * step
        opt.param_groups[0]["lr"] = lr
        for i, p in enumerate(P):
            g = (rng.standard_normal(p.shape) * 10.0 ** (step - 4)).astype(np.float32)
            if i == 2 and step == 3:
                g[:] = 0                                                     # an all-zero gradient
            p.grad = torch.from_numpy(g.astype(np.float64))
            ps[i], ms[i], vs[i] = S.adam_np(ps[i], g, ms[i], vs[i], step, lr, 0.9, 0.999, 1e-8, wd)
        opt.step()
        for i, p in enumerate(P):
            ref = p.detach().numpy()
            assert np.abs(ps[i] - ref).max() <= 1e-6 * np.abs(ref).max(), (step, i)
            for mine, key in ((ms[i], "exp_avg"), (vs[i], "exp_avg_sq")):
                r = opt.state[p][key].numpy()
                assert np.abs(mine - r).max() <= 1e-6 * np.abs(r).max() + 1e-30, (key, step, i)
    assert int(S.ulps(np.float32([1.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0])).max()) == 1


@pytest.mark.parametrize("kind", S.LOSSES)
def test_every_loss_case_keeps_the_1e5_bound_of_the_rule(kind):
    """tests/loss_range.py derives a bound from the float32 CPU evaluation of the same restatement: at or below 1.25e-6 the
    bound is L.BOUND.  Held here at every size the GPU test runs, so that test compares with L.BOUND itself."""
    worst = 0.0
    for n in S.TINY + (S.TODAY,) + S.POINTWISE:
        ref = S.loss_reference(kind, n)
        assert L.is_finite(ref), (kind, n)
        e = max(L.errors(kind, S.loss_evaluate(kind, n, torch.float32), ref))
        worst = max(worst, e)
        assert L.rule(e) == L.BOUND, (kind, n, e)
    print(f"[streaming edges] {kind}: float32 CPU evaluation within {worst:.3e} of float64 at every size")
