"""The baseline pair model - mirror of reference `reactranker/models/ranknet_baseline.py`: one MPN encoder applied to the
reactant graph and to the two product graphs of a pair, the difference encoder on  (p1_h - r_h) + (p2_h - r_h)  over the
REACTANT graph's topology (:52-63), then the FFN.  `ReactionModel(r_inputs, p1_inputs, p2_inputs, gpu)` and `build_model`
keep the reference's arguments, its head-string logic (:79-86) and the state-dict keys of base_model.ReactionModel, so a
checkpoint of either model loads into the other.

It is composed from the existing MPN / MPNDiff / FFN modules (each one autograd node on the HIP kernels), not a step plan of
its own.  In train mode with dropout it makes three encoder passes as the reference does.  With dropout inactive (eval, or
p = 0) and a pair batch that carries molecule indices (reactranker_amd.pairs.pair_batch), every distinct molecule of the
batch is encoded ONCE and rr_pair_combine_f32 gathers the pair rows: a query with C candidates has up to C (C - 1) ordered
pairs but only C + 1 molecules."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, lib, ptr, stream
from .base_model import FFN
from .featurization import ATOM_FDIM, BOND_FDIM, device_graph_of
from .mpn import MPN, MPNDiff


def _i32(a, device):
    return None if a is None else torch.as_tensor(a, dtype=torch.int32).to(device).contiguous()


class PairCombineFn(torch.autograd.Function):
    """out[row] = (h1[i1[row]] - hr[ir[row]]) + (h2[i2[row]] - hr[ir[row]]) (rr_pair_combine_f32).  Differentiable in its
    identity form (no index arrays: the three-pass path, d h1 = d h2 = g, d hr = -2 g); the gathering form is forward only."""

    @staticmethod
    def forward(ctx, hr, h1, h2, ir, i1, i2, n_rows):
        for t, name in ((hr, "hr"), (h1, "h1"), (h2, "h2")):
            _lib.require_cuda(t, name)
            if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
                raise RuntimeError(f"pair combine: {name} must be a row-major float32 matrix")
        H, ld = hr.shape[1], hr.stride(0)
        if h1.shape[1] != H or h2.shape[1] != H or h1.stride(0) != ld or h2.stride(0) != ld:
            raise RuntimeError("pair combine: the three sources must share width and row pitch")
        if ir is None and not (hr.shape[0] == h1.shape[0] == h2.shape[0] == n_rows):
            raise RuntimeError("reactant and product batches must hold the same atoms in the same order "
                               "(diff = p_h - r_h, reference models/ranknet_baseline.py:57-58)")
        out = torch.empty(n_rows, H, dtype=torch.float32, device=hr.device)
        check(lib().rr_pair_combine_f32(ptr(hr), ptr(h1), ptr(h2), ld, ptr(ir), ptr(i1), ptr(i2), n_rows, H, ptr(out),
                                        out.stride(0), stream()), "rr_pair_combine_f32")
        ctx.identity = ir is None
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.identity:
            raise RuntimeError("the de-duplicated pair path is forward only (dropout inactive, no gradient)")
        from .functions import axpby
        g = g.contiguous()
        return axpby(-2.0, g), g, g, None, None, None, None


class ReactionModel(nn.Module):
    """Reference models/ranknet_baseline.py:9-63."""

    def __init__(self, mpnn_hidden_size: int = 300, mpnn_bias: bool = True, mpnn_depth: int = 3, mpnn_dropout=0.2,
                 mpnn_diff_hidden_size: int = 300, mpnn_diff_bias: bool = True, mpnn_diff_depth: int = 3,
                 mpnn_diff_dropout=0.2, ffn_hidden_size: int = 300, ffn_bias: bool = True, ffn_dropout=0.2,
                 ffn_depth: int = 3, task_num: int = 2, task_type: str = 'no_softplus'):
        super().__init__()
        self.encoder = MPN(bond_fdim=ATOM_FDIM + BOND_FDIM, atom_fdim=ATOM_FDIM, MPN_hidden_size=mpnn_hidden_size,
                           MPN_bias=mpnn_bias, MPN_depth=mpnn_depth, MPN_dropout=mpnn_dropout, return_atom_hiddens=True)
        self.diff_encoder = MPNDiff(atom_fdim=mpnn_hidden_size, bond_fdim=ATOM_FDIM + BOND_FDIM,
                                    MPNDiff_hidden_size=mpnn_diff_hidden_size, MPNDiff_bias=mpnn_diff_bias,
                                    MPNDiff_depth=mpnn_diff_depth, MPNDiff_dropout=mpnn_diff_dropout)
        self.ffn = FFN(reacvec_fdim=mpnn_diff_hidden_size, ffn_hidden_size=ffn_hidden_size, ffn_dropout=ffn_dropout,
                       ffn_num_layers=ffn_depth, task_num=task_num, ffn_bias=ffn_bias, task_type=task_type)
        if mpnn_hidden_size % 4:
            raise NotImplementedError("the pair model needs a hidden size divisible by 4 (16-byte lanes of the row combine)")
        self.dedup_molecules = "auto"        # False: always three encoder passes

    def forward(self, r_inputs, p1_inputs, p2_inputs, gpu: int = None, pair_index=None):
        """pair_index: (u, ir, i1, i2) of reactranker_amd.pairs.pair_batch - used when dropout is inactive."""
        rg = device_graph_of(r_inputs, gpu)
        p_active = float(self.encoder.dropout) if self.training else 0.0
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if pair_index is not None and self.dedup_molecules in ("auto", True) and p_active == 0.0 and not grad:
            u, ir, i1, i2 = pair_index
            for ix in (ir, i1, i2):
                if len(ix) != rg.nA or (len(ix) and (int(ix.min()) < 0 or int(ix.max()) >= u.n_atoms)):
                    raise RuntimeError("pair_index does not describe this pair batch")
            cache = getattr(r_inputs, "_rr_pair_index_dev", None)
            if cache is None or cache[0] != str(rg.device):
                cache = (str(rg.device), *[_i32(ix, rg.device) for ix in (ir, i1, i2)])
                r_inputs._rr_pair_index_dev = cache
            h = self.encoder(u, gpu=gpu)
            feats = PairCombineFn.apply(h, h, h, cache[1], cache[2], cache[3], rg.nA)
        else:
            p1g, p2g = device_graph_of(p1_inputs, gpu), device_graph_of(p2_inputs, gpu)
            if not (rg.nA == p1g.nA == p2g.nA):
                raise RuntimeError("reactant and product batches must hold the same atoms in the same order "
                                   "(diff = p_h - r_h, reference models/ranknet_baseline.py:57-58)")
            r_h = self.encoder(r_inputs, gpu=gpu)
            p1_h = self.encoder(p1_inputs, gpu=gpu)
            p2_h = self.encoder(p2_inputs, gpu=gpu)
            feats = PairCombineFn.apply(r_h, p1_h, p2_h, None, None, None, rg.nA)
        return self.ffn(self.diff_encoder(feats, r_inputs, gpu=gpu))


def build_model(hidden_size: int = 300, mpnn_depth: int = 3, mpnn_diff_depth: int = 3, ffn_depth: int = 3,
                use_bias: bool = True, dropout=0.2, task_num: int = 2, ffn_last_layer: str = 'no_softplus'):
    """Reference models/ranknet_baseline.py:66-103 (same head-string logic :79-86)."""
    if task_num == 2 and ffn_last_layer != 'evidential':
        task_type = 'gaussian_' + ffn_last_layer
    elif task_num == 4:
        task_type = 'evidential_' + ffn_last_layer
    else:
        task_type = ffn_last_layer
    return ReactionModel(mpnn_hidden_size=hidden_size, mpnn_bias=use_bias, mpnn_depth=mpnn_depth, mpnn_dropout=dropout,
                         mpnn_diff_hidden_size=hidden_size, mpnn_diff_bias=use_bias, mpnn_diff_depth=mpnn_diff_depth,
                         mpnn_diff_dropout=dropout, ffn_hidden_size=hidden_size, ffn_bias=use_bias, ffn_dropout=dropout,
                         ffn_depth=ffn_depth, task_num=task_num, task_type=task_type)
