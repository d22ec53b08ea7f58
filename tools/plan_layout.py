"""CPU-only: workspace size and saved-tensor offsets of the step plans over a grid of models (fake pointers; layout passes
never dereference them).  Usage: python plan_layout.py REPO_ROOT > out.txt"""
import ctypes as C
import itertools
import sys

sys.path.insert(0, sys.argv[1])
from reactranker_amd import _lib  # noqa: E402

L = _lib.lib()
FAKE = 1 << 20
BASE = 1 << 32


def fp(i=0):
    return C.cast(C.c_void_p(FAKE + 4096 * i), _lib.c_f32p)


def ip(i=0):
    return C.cast(C.c_void_p(FAKE + 4096 * i), _lib.c_i32p)


def graph(nA, nB, M, K=4, Kb=3):
    G = _lib.Graph()
    G.nA, G.nB, G.M, G.K, G.Kb = nA, nB, M, K, Kb
    G.f_atoms, G.ld_fa, G.f_bonds, G.ld_fb = fp(1), 64, fp(2), 84
    for j, k in enumerate(("a2b", "b2a", "b2revb", "a2a", "a_scope", "b2t", "a2a_t", "atom2mol", "b2b_t")):
        setattr(G, k, ip(3 + j))
    G.npad, G.npad_b, G.fb_sum, G.ld_fbs = fp(20), fp(21), fp(22), 84
    return G


def lw(out, in_):
    W = _lib.LinearW()
    W.w, W.b, W.out, W.in_, W.ldw = fp(30), fp(31), out, in_, in_
    return W


n = 0
for H, d, dd, nf, F, mode, big in itertools.product((32, 300, 600), (1, 2, 3, 6, 16), (0, 1, 3, 16), (1, 3), (0, 1), (0, 1, 2), (0, 1)):
    if mode == 2 and d < 2:
        continue
    M = _lib.Model()
    M.H, M.depth, M.diff_depth, M.n_ffn, M.head, M.atom_fdim, M.bond_fdim = H, d, dd, nf, 0, 61, 83
    M.enc_wi, M.enc_wh, M.enc_wo = lw(H, 83), lw(H, H), lw(H, 61 + H)
    M.dif_wi, M.dif_wh, M.dif_wo = lw(H, H), lw(H, H + 83), lw(H, 2 * H)
    for i in range(nf):
        M.ffn[i] = lw(1 if i == nf - 1 else H, (H + F) if i == 0 else H)
    S = _lib.Step()
    nA, nB, nm = (60000, 130000, 4096) if big else (700, 1500, 48)
    S.p = graph(nA, nB, nm)
    S.r = graph(nA if mode != 1 else nA // 8, nB if mode != 1 else nB // 8, nm if mode != 1 else nm // 8)
    S.u = graph(nA // 8, nB // 8, nm // 8)
    S.mode = mode
    S.amap, S.amap_t, S.amap_t_cols = ip(40), ip(41), 9
    S.bmap, S.bmap_t, S.bmap_t_cols = ip(42), ip(43), 9
    S.feat, S.F, S.drop_p, S.seed, S.out = fp(44), F, 0.0 if mode == 1 else 0.1, 7, fp(45)
    need = int(L.rr_reaction_workspace_bytes(C.byref(M), C.byref(S)))
    S.workspace, S.workspace_bytes = C.c_void_p(BASE), need
    row = [H, d, dd, nf, F, mode, big, need]
    for flags in (0, _lib.RR_PLAN_TRAIN, _lib.RR_PLAN_F32_GEMM, _lib.RR_PLAN_F16X2_GEMM | _lib.RR_PLAN_TRAIN):
        for which in range(10):
            for idx in (0, 1, max(d, dd, nf) - 1):
                p, r, ld = C.c_void_p(), C.c_int64(), C.c_int64()
                st = L.rr_reaction_saved_f32(C.byref(M), C.byref(S), flags, which, idx, C.byref(p), C.byref(r), C.byref(ld))
                row.append((st, (p.value - BASE) if p.value else -1, r.value, ld.value))
    print(row)
    n += 1
print("cases", n, file=sys.stderr)
