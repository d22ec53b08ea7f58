"""Atom / bond attributions of a reaction score: input gradients, gradient x input and integrated gradients.

Which atoms and bonds of a reaction moved the score.  The model is a set of explicit autograd.Functions whose gradients stop
at the first layer's pre-activation, so this module carries its own input-gradient backward: the forward of the per-op
primitives in `functions` (no step plan, dropout 0, reactants NOT de-duplicated - attributions are per candidate), then the
data flow of `ReactionModelFn.backward` without any weight gradient, side stream or parameter `.grad`, ending in
rr_input_attribution_f32 (csrc/attribution.hip): the adjoint of W_i / W_o fused with the product by the layer's input and the
per-row segment sums.  rr_attribution_reduce_f32 turns the per-row terms into atom, bond and per-molecule numbers.

    input_gradients(model, r_batch, p_batch, add_features=None, column=0, gpu=None)
    attribute(model, r_batch, p_batch, add_features=None, column=0, method="grad_x_input", steps=16, gpu=None)

An atom's number is its own f_atoms row's term (the W_o path) plus the terms of the copies of its features that sit in the
first 61 columns of the f_bonds rows of its OUTGOING bonds (the W_i path, and through fb_sum the difference encoder's W_h).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import functions as Fn
from ._lib import check, lib, ptr, stream
from .featurization import device_graph_of
from .functions import ATOM_FDIM, FBOND, LinW

METHODS = ("grad_x_input", "integrated_gradients")
MAX_K = 128                                    # = RR_ATTR_MAX_K (checked against the library at the first launch)


# =========================================================================== the two native entries
def input_attribution(dz, w, K: int, *, N: Optional[int] = None, ld_w: Optional[int] = None, w_offset: int = 0, x=None,
                      add=None, add_idx=None, segments=None, alpha: float = 1.0, accumulate: bool = False, attr=None, dx=None,
                      M: Optional[int] = None):
    """rr_input_attribution_f32 on torch tensors.  `w` is a Linear.weight ([N, >= w_offset + K]); w_offset selects a column
    window.  attr [M, len(segments)] and / or dx [M, >= K] are written (or accumulated into) in place."""
    M = dz.shape[0] if M is None else M
    N = dz.shape[1] if N is None else N
    seg = None
    if attr is not None:
        seg = (C.c_int32 * len(segments))(*[int(s) for s in segments])
    wp = None if w is None else C.c_void_p(w.data_ptr() + 4 * int(w_offset))
    check(lib().rr_input_attribution_f32(
        ptr(dz), Fn._ld(dz), wp, (w.stride(0) if ld_w is None else ld_w), ptr(x), Fn._ld(x), ptr(add), Fn._ld(add), ptr(add_idx),
        M, N, K, seg, 0 if seg is None else len(segments), float(alpha), int(bool(accumulate)),
        ptr(attr), (0 if attr is None else attr.stride(0)), ptr(dx), Fn._ld(dx), stream()), "rr_input_attribution_f32")


def attribution_reduce(g, attr_fa, attr_fb):
    """rr_attribution_reduce_f32 -> (atom [nA], bond [nB], bond_sym [nB], mol_total [M] float64) of graph g."""
    dev = attr_fa.device
    atom = torch.empty(g.nA, dtype=torch.float32, device=dev)
    bond = torch.empty(g.nB, dtype=torch.float32, device=dev)
    bond_sym = torch.empty(g.nB, dtype=torch.float32, device=dev)
    total = torch.empty(g.M, dtype=torch.float64, device=dev)
    check(lib().rr_attribution_reduce_f32(ptr(attr_fa), attr_fa.stride(0), ptr(attr_fb), attr_fb.stride(0), ptr(g.a2b),
                                          ptr(g.b2revb), ptr(g.a_scope), g.nA, g.nB, g.M, g.K, ptr(atom), ptr(bond),
                                          ptr(bond_sym), ptr(total), stream()), "rr_attribution_reduce_f32")
    return atom, bond, bond_sym, total


# =========================================================================== arguments (no GPU needed)
def _count(batch, name: str, key: str):
    v = getattr(batch, name, None)
    if v is None:
        v = getattr(batch, key, None)
    return None if v is None else int(v)


def _check_args(model, r_batch, p_batch, add_features, column, method=None, steps=None):
    """Everything that can be wrong with a call, before the first byte reaches the GPU.  -> (F, features as [M,F] float32 or None)"""
    if method is not None and method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if steps is not None and (not isinstance(steps, (int, np.integer)) or isinstance(steps, bool) or steps < 1):
        raise ValueError(f"steps must be an integer >= 1, got {steps!r}")
    n_out = int(model.ffn.task_num)
    if not isinstance(column, (int, np.integer)) or isinstance(column, bool) or not 0 <= column < n_out:
        raise ValueError(f"column must be one of 0..{n_out - 1} (the model has {n_out} output column(s)), got {column!r}")
    ra, pa = _count(r_batch, "n_atoms", "nA"), _count(p_batch, "n_atoms", "nA")
    rm, pm = _count(r_batch, "n_mols", "M"), _count(p_batch, "n_mols", "M")
    if ra != pa or rm != pm:
        raise ValueError(f"reactant and product batches must hold the same molecules and atoms in the same order "
                         f"(allowed: equal counts; got {rm} / {pm} molecules, {ra} / {pa} atoms)")
    want = int(model.ffn.hidden_size) - int(model.diff_encoder.hidden_size)
    feat, F = None, 0
    if add_features is not None:
        if torch.is_tensor(add_features):
            feat = add_features.detach().to(dtype=torch.float32)
        else:
            feat = torch.as_tensor(np.asarray(add_features), dtype=torch.float32)
        if pm is not None and pm > 0 and feat.numel() % pm == 0:
            feat = feat.reshape(pm, -1)
        F = int(feat.shape[1]) if feat.dim() == 2 and feat.shape[0] == pm else -1
    if F != want:
        raise ValueError(f"add_features must have width {want} (the FFN reads {model.ffn.hidden_size} columns, "
                         f"{model.diff_encoder.hidden_size} of them the readout), got {F}")
    if max(ATOM_FDIM, FBOND) > MAX_K:
        raise ValueError(f"feature rows wider than {MAX_K} columns are not supported")
    return F, feat


# =========================================================================== forward / input-gradient backward
class _Scaled:
    """A DeviceGraph whose f_atoms, f_bonds and fb_sum are scaled copies (an integrated-gradients node); every table is the
    underlying graph's.  The batch's cached graph and its fb_sum stay as they are."""

    def __init__(self, g, alpha: float, need_fb_sum: bool):
        self._g = g
        def scaled(t):
            return Fn.axpby(alpha, t) if t.is_contiguous() else (t * alpha).contiguous()
        self.f_atoms = scaled(g.f_atoms)
        self.f_bonds = scaled(g.f_bonds)
        self._fbs = scaled(g.fb_sum()) if need_fb_sum else None

    def fb_sum(self):
        return self._fbs

    def __getattr__(self, k):
        return getattr(self._g, k)


def _mods(model):
    q = model.flat_params()
    enc = [LinW(q[0], q[1]), LinW(q[2], q[3]) if q[2] is not None else None, LinW(q[4], q[5])]
    dif = [LinW(q[6], q[7]), LinW(q[8], q[9]) if q[8] is not None else None, LinW(q[10], q[11]) if q[10] is not None else None]
    ffn = [LinW(q[i], q[i + 1], big=False) for i in range(12, len(q), 2)]
    return enc, dif, ffn


def _forward(cfg, mods, rg, pg, feat):
    """The per-op forward with dropout 0 and one reactant graph per candidate -> (out [M, n_out], saved)."""
    enc, dif, ffn = mods
    H = cfg["H"]
    r_h, r_saved = Fn.mpn_forward(rg, H, cfg["depth"], enc[0], enc[1], enc[2], 0.0, 0)
    p_h, p_saved = Fn.mpn_forward(pg, H, cfg["depth"], enc[0], enc[1], enc[2], 0.0, 0)
    vecs, d_saved = Fn.mpndiff_forward(pg, H, cfg["diff_depth"], dif[0], dif[1], dif[2], 0.0, 0, p_h, r_h, feat, cfg["F"])
    out, f_saved = Fn.ffn_forward(vecs, ffn, 0.0, 0, cfg["head"])
    return out, (r_saved, p_saved, d_saved, f_saved, r_h, p_h)


def _mp_input_backward(R, depth: int, Wh, msgs, d_a, want_dz_sum: bool = False):
    """functions._mp_backward_unfused without its weight gradients: d a_last -> (d input, sum over iterations of dZ_it or None)."""
    H = R.H
    d_msg = Fn.gather_sum(d_a, R.fwd_t, H)
    Fn.weighted_colsum(d_a, R.npad_a, H, d_msg[0], accumulate=True)
    d_inp = None
    for it in reversed(range(depth - 1)):
        if d_inp is None:
            d_inp = torch.zeros_like(d_msg)
        dz = Fn.relu_bwd(d_msg, msgs[it + 1], 1.0, dz=torch.empty_like(d_msg), acc=d_inp)
        d_min = Fn.linear(R.rows, H, Wh.pk_t(0, H), w_packed=True, a1=dz, k1=H)
        d_msg = Fn.gather_sum(d_min, R.back, H)
        Fn.weighted_colsum(d_min, R.npad, H, d_msg[0], accumulate=True)
    if d_inp is None:
        return Fn.relu_bwd(d_msg, msgs[0], 1.0), None
    dz_sum = d_inp.clone() if want_dz_sum else None
    Fn.relu_bwd(d_msg, msgs[0], 1.0, acc=d_inp, want_dz=False)
    return d_inp, dz_sum


def _mp_input_backward_fused(R, depth: int, Wh, msgs, d_a, part):
    """functions._mp_backward without its weight gradients (H % 4 == 0): every gradient is produced already masked by the
    epilogue of the gather that forms it, the padding row's adjoint rides on the GEMM's column-sum partials, and the last
    gather adds every iteration's dZ.  -> (d input, [dZ_it])."""
    H, top = R.H, depth - 1
    cur = Fn.gather_sum(d_a, R.fwd_t, H, row0_partial=part, mask=msgs[top], mask_scale=1.0)
    dzs = []
    for it in reversed(range(depth - 1)):
        dz = cur
        d_min, part = Fn.linear(R.rows, H, Wh.pk_t(0, H), w_packed=True, a1=dz, k1=H, colsum_w=R.npad)
        dzs.append(dz)
        cur = Fn.gather_sum(d_min, R.back, H, row0_partial=part, mask=msgs[it], mask_scale=1.0, adds=(dzs if it == 0 else ()))
    return cur, dzs


def _ffn_input_backward(layers, head: int, saved, dout):
    """functions.ffn_backward without its weight gradients, every input column -> d vecs [M, H + F]."""
    hs, raw = saved
    M = raw.shape[0]
    d = dout if head == 0 else Fn.head_bwd(dout, raw, head)
    L = layers[-1]
    dx = Fn.linear(M, L.w.shape[1], L.pk_t(0, L.w.shape[1]), w_packed=True, a1=d, k1=L.w.shape[0])
    for li in reversed(range(len(layers) - 1)):
        L = layers[li]
        dx = Fn.linear(M, L.w.shape[1], L.pk_t(0, L.w.shape[1]), w_packed=True, a1=dx, k1=L.w.shape[0], a_mask=hs[li + 1],
                       mask_scale=1.0)
    return dx


def _diff_input_backward(cfg, dif, pg, saved, p_h, dvecs):
    """Adjoint of mpndiff_forward in its inputs -> (d_diff [nA,H], d fb_sum [nA + 1, 84] or None).  Row nA of d fb_sum is the
    padding bond's share: bond 0 fills the npad[a] empty slots of every a2b row."""
    Wi, Wh, Wo = dif
    msgs, amsgs, a_last, hid = saved
    H, depth, F, nA = cfg["H"], cfg["diff_depth"], cfg["F"], pg.nA
    d_fbs = None

    def fbs_of(dzs):
        # d fb_sum = (sum_it dZ_it) . W_h[:, H:H+83]: the dense form of the new entry (x = NULL), one call per addend
        out = torch.empty(nA + 1, FBOND + 1, dtype=torch.float32, device=dvecs.device)
        for i, dz in enumerate(dzs):
            input_attribution(dz, Wh.w, FBOND, w_offset=H, dx=out, accumulate=i > 0, M=nA)
        Fn.weighted_colsum(out[:nA], pg.npad, FBOND, out[nA], accumulate=False)
        return out
    if depth > 0 and H % 4 == 0:
        # the readout's adjoint applies hid's ReLU pattern as it writes (dZ of W_o); the iterations follow the fused form
        R = Fn._Rel(pg, H, bonds=False, depth=depth)
        dz_o = Fn.segment_mean_bwd(dvecs, pg, H, F, 0.0, 0, mask=hid, mask_scale=1.0)
        d_x = Fn.linear(nA, H, Wo.pk_t(0, H), w_packed=True, a1=dz_o, k1=H)
        d_a, part = Fn.linear(nA, H, Wo.pk_t(H, 2 * H), w_packed=True, a1=dz_o, k1=H, colsum_w=pg.npad)
        d_inp, dzs = _mp_input_backward_fused(R, depth, Wh, msgs, d_a, part)
        if depth > 1:
            d_fbs = fbs_of(dzs)
        Fn.linear(nA, H, Wi.pk_t(0, H), w_packed=True, a1=d_inp, k1=H, residual=d_x, out=d_x)
    elif depth > 0:
        d_hid = Fn.segment_mean_bwd(dvecs, pg, H, F, 0.0, 0)
        R = Fn._Rel(pg, H, bonds=False, depth=depth)
        d_x = Fn.linear(nA, H, Wo.pk_t(0, H), w_packed=True, a1=d_hid, k1=H, a_mask=hid, mask_scale=1.0)
        d_a = Fn.linear(nA, H, Wo.pk_t(H, 2 * H), w_packed=True, a1=d_hid, k1=H, a_mask=hid, mask_scale=1.0)
        d_inp, dz_sum = _mp_input_backward(R, depth, Wh, msgs, d_a, want_dz_sum=depth > 1)
        if depth > 1:
            d_fbs = fbs_of([dz_sum])
        Fn.linear(nA, H, Wi.pk_t(0, H), w_packed=True, a1=d_inp, k1=H, residual=d_x, out=d_x)
    else:
        d_hid = Fn.segment_mean_bwd(dvecs, pg, H, F, 0.0, 0)
        d_inp = Fn.relu_bwd(d_hid, msgs[0], 1.0)
        d_x = Fn.linear(nA, H, Wi.pk_t(0, H), w_packed=True, a1=d_inp, k1=H)
    return d_x, d_fbs


def _fbs_route(pg):
    """add_idx of the product graph's W_i call: bond b receives d fb_sum of its TARGET atom; bond 0 (the padding bond) the
    extra row nA (see _diff_input_backward).  Cached on nothing: a [nB] int32 copy per call."""
    idx = pg.b2t.reshape(-1).clone()
    idx[:1].fill_(pg.nA)                           # (idx[0] = ... copies a host scalar and blocks the host on the caller's stream)
    return idx


def _encoder_input_backward(cfg, enc, g, saved, d_diff, sign: float):
    """Adjoint of mpn_forward down to the two pre-activation gradients the attribution entry reads:
    -> (d_inp [nB,H] of W_i, dz_o [nA,H] of W_o, both already masked by their ReLU)."""
    Wi, Wh, Wo = enc
    msgs, amsgs, a_last, h = saved
    H = cfg["H"]
    R = Fn._Rel(g, H, bonds=True)
    if H % 4 == 0:
        # the W_o input-gradient GEMM applies h's ReLU pattern in its operand loader and writes the masked dZ as a side output
        dz_o = torch.empty_like(d_diff)
        d_a, part = Fn.linear(g.nA, H, Wo.pk_t(ATOM_FDIM, ATOM_FDIM + H), w_packed=True, a1=d_diff, k1=H, a_mask=h,
                              mask_scale=sign, dz_out=dz_o, colsum_w=g.npad)
        d_inp, _ = _mp_input_backward_fused(R, cfg["depth"], Wh, msgs, d_a, part)
        return d_inp, dz_o
    dz_o = Fn.relu_bwd(d_diff, h, sign)
    d_a = Fn.linear(g.nA, H, Wo.pk_t(ATOM_FDIM, ATOM_FDIM + H), w_packed=True, a1=dz_o, k1=H)
    d_inp, _ = _mp_input_backward(R, cfg["depth"], Wh, msgs, d_a)
    return d_inp, dz_o


def _backward(cfg, mods, rg, pg, saved, column: int):
    """One-hot cotangent on output column `column` -> per graph (d_inp, dz_o), the fb_sum route, d vecs."""
    enc, dif, ffn = mods
    r_saved, p_saved, d_saved, f_saved, r_h, p_h = saved
    raw = f_saved[1]
    dout = torch.zeros_like(raw)
    dout[:, column] = 1.0
    dvecs = _ffn_input_backward(ffn, cfg["head"], f_saved, dout)
    d_diff, d_fbs = _diff_input_backward(cfg, dif, pg, d_saved, p_h, dvecs)
    p_pre = _encoder_input_backward(cfg, enc, pg, p_saved, d_diff, 1.0)
    r_pre = _encoder_input_backward(cfg, enc, rg, r_saved, d_diff, -1.0)
    route = None if d_fbs is None else (d_fbs, _fbs_route(pg))
    return r_pre, p_pre, route, dvecs


def _first_layer(enc, g, x_graph, pre, route, alpha, accumulate, attr=None, dx=None):
    """The two calls of the fused entry for one graph.  attr = (attr_fa [nA,1], attr_fb [nB,2]) and / or dx = (d f_atoms
    [nA,61], d f_bonds [nB,83]).  x_graph holds the (unscaled) inputs the products are taken with."""
    Wi, _, Wo = enc
    d_inp, dz_o = pre
    add, add_idx = route if route is not None else (None, None)
    input_attribution(d_inp, Wi.w, FBOND, x=None if attr is None else x_graph.f_bonds, add=add, add_idx=add_idx,
                      segments=(ATOM_FDIM, FBOND), alpha=alpha, accumulate=accumulate, attr=None if attr is None else attr[1],
                      dx=None if dx is None else dx[1])
    input_attribution(dz_o, Wo.w, ATOM_FDIM, x=None if attr is None else x_graph.f_atoms, segments=(ATOM_FDIM,), alpha=alpha,
                      accumulate=accumulate, attr=None if attr is None else attr[0], dx=None if dx is None else dx[0])


def _setup(model, r_batch, p_batch, add_features, column, gpu, method=None, steps=None):
    F, feat = _check_args(model, r_batch, p_batch, add_features, column, method, steps)
    if int(lib().rr_input_attribution_max_k()) != MAX_K:
        raise RuntimeError("reactranker_amd: RR_ATTR_MAX_K of the library differs from attribution.MAX_K; rebuild")
    rg, pg = device_graph_of(r_batch, gpu), device_graph_of(p_batch, gpu)
    if feat is not None:
        feat = feat.to(pg.device).contiguous()
    cfg = dict(H=model.encoder.hidden_size, depth=model.encoder.depth, diff_depth=model.diff_encoder.depth, F=F,
               head=model.ffn.head())
    for q in model.parameters():
        if q.device != pg.device:
            raise RuntimeError(f"the model lives on {q.device}, the batch on {pg.device}")
    return cfg, _mods(model), rg, pg, feat


def _score(out, column: int):
    return out[:, column].clone()


# =========================================================================== public interface
def input_gradients(model, r_batch, p_batch, add_features=None, column: int = 0, gpu=None):
    """d out[:, column] / d (f_atoms, f_bonds, add_features) of both graphs, head included, in eval arithmetic (dropout 0).
    Candidates do not interact, so the rows of a candidate's molecules hold that candidate's gradient.  d_f_atoms_* is the
    W_o path alone; d_f_bonds_* carries the copies of the source atom's features in its first 61 columns.
    -> {"d_f_atoms_r" [nA,61], "d_f_bonds_r" [nB_r,83], "d_f_atoms_p", "d_f_bonds_p", "d_add_features" [M,F] or None, "score" [M]}"""
    cfg, mods, rg, pg, feat = _setup(model, r_batch, p_batch, add_features, column, gpu)
    with torch.no_grad():
        out, saved = _forward(cfg, mods, rg, pg, feat)
        r_pre, p_pre, route, dvecs = _backward(cfg, mods, rg, pg, saved, column)
        res = {}
        for tag, g, pre, rt in (("r", rg, r_pre, None), ("p", pg, p_pre, route)):
            d_fa = torch.empty(g.nA, ATOM_FDIM, dtype=torch.float32, device=g.device)
            d_fb = torch.empty(g.nB, FBOND, dtype=torch.float32, device=g.device)
            _first_layer(mods[0], g, g, pre, rt, 1.0, False, dx=(d_fa, d_fb))
            res["d_f_atoms_" + tag], res["d_f_bonds_" + tag] = d_fa, d_fb
        H, F = cfg["H"], cfg["F"]
        res["d_add_features"] = dvecs[:, H:H + F].clone() if F else None
        res["score"] = _score(out, column)
    return res


def attribute(model, r_batch, p_batch, add_features=None, column: int = 0, method: str = "grad_x_input", steps: int = 16,
              gpu=None):
    """Attributions of out[:, column] to atoms, directed bonds and appended features.
    grad_x_input: input times gradient, one forward and one backward.  Complete (total == score) only for a bias-free model
    with a raw head.  integrated_gradients: zero baseline, midpoint rule with `steps` nodes alpha_s = (s + 0.5) / steps;
    total approaches score - baseline_score as steps grows ("gap" is what is left).
    -> {"atom_r", "atom_p" [nA], "bond_r", "bond_p" [nB] (directed), "bond_sym_r", "bond_sym_p" [nB], "feature" [M,F] or None,
        "total" [M] float64, "score" [M]; integrated gradients also "baseline_score" [M] and "gap" [M] float64}"""
    cfg, mods, rg, pg, feat = _setup(model, r_batch, p_batch, add_features, column, gpu, method, steps)
    H, F = cfg["H"], cfg["F"]
    dev = pg.device
    with torch.no_grad():
        attrs = {t: (torch.empty(g.nA, 1, dtype=torch.float32, device=dev), torch.empty(g.nB, 2, dtype=torch.float32, device=dev))
                 for t, g in (("r", rg), ("p", pg))}
        res = {}
        if method == "grad_x_input":
            out, saved = _forward(cfg, mods, rg, pg, feat)
            r_pre, p_pre, route, dvecs = _backward(cfg, mods, rg, pg, saved, column)
            _first_layer(mods[0], rg, rg, r_pre, None, 1.0, False, attr=attrs["r"])
            _first_layer(mods[0], pg, pg, p_pre, route, 1.0, False, attr=attrs["p"])
            feature = feat * dvecs[:, H:H + F] if F else None
            score = _score(out, column)
        else:
            need_fbs = cfg["diff_depth"] > 1
            d_feat = None
            for s in range(steps):
                a = (s + 0.5) / steps
                rs, ps = _Scaled(rg, a, False), _Scaled(pg, a, need_fbs)
                fs = None if feat is None else feat * a
                out, saved = _forward(cfg, mods, rs, ps, fs)
                r_pre, p_pre, route, dvecs = _backward(cfg, mods, rs, ps, saved, column)
                _first_layer(mods[0], rg, rg, r_pre, None, 1.0 / steps, s > 0, attr=attrs["r"])
                _first_layer(mods[0], pg, pg, p_pre, route, 1.0 / steps, s > 0, attr=attrs["p"])
                if F:
                    d_feat = dvecs[:, H:H + F].clone() if d_feat is None else d_feat + dvecs[:, H:H + F]
                del saved
            feature = feat * (d_feat / steps) if F else None
            out, _ = _forward(cfg, mods, rg, pg, feat)
            score = _score(out, column)
            out0, _ = _forward(cfg, mods, _Scaled(rg, 0.0, False), _Scaled(pg, 0.0, need_fbs), None if feat is None else feat * 0.0)
            res["baseline_score"] = _score(out0, column)
        total = torch.zeros(pg.M, dtype=torch.float64, device=dev)
        for t, g in (("r", rg), ("p", pg)):
            atom, bond, bond_sym, mol = attribution_reduce(g, attrs[t][0], attrs[t][1])
            res["atom_" + t], res["bond_" + t], res["bond_sym_" + t] = atom, bond, bond_sym
            total = total + mol
        if F:
            total = total + feature.to(torch.float64).sum(dim=1)
        res["feature"], res["total"], res["score"] = feature, total, score
        if method == "integrated_gradients":
            res["gap"] = total - (score.to(torch.float64) - res["baseline_score"].to(torch.float64))
    return res
