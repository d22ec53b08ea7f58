"""The hidden sizes at which a dispatcher of the library changes its mind, as data, next to a pure-Python restatement of the
rules that decide (no GPU, no library needed: tests/test_hidden_sizes_cpu.py holds the rules against the sources and the table
against the rules, tests/test_gpu_hidden_sizes.py runs the assembled model and the FFN chain at every rung).

Rules restated, for a model of hidden size H with F appended features and an FFN head of widths [H + F, H, ..., H, task_num]:
  split GEMM (linear_split.hip launch_split_geometry, at the M <= 8192 rows of the test batches): every encoder GEMM has N = H
      N <= 64 -> <4,4,8>;  N <= 160 -> <10,10,8>;  N <= 304 -> <19,5,8>;  N <= 608 -> <38,19,12>
  f32 layout (functions.LinW._pack, plan.hip pack): N > 608 or N % 4 != 0 - the weight is packed for the f32 MFMA kernels
  step plan (functions.StepPlan.eligible, rr_reaction_forward's argument check): H % 4 == 0; otherwise the per-op path, no
      shared reactant prefix, no 16-byte gather path
  FFN chain (ffn.hip rr_ffn_chain_f32): T = ceil(H / 16) column tiles per hidden layer; T <= 8 -> <8,1>, T <= 24 -> <8,3>,
      T <= 40 -> <8,5>, above (or kmax > 1024, or H % 4 != 0) RR_ERR_UNSUPPORTED = -4: the layers are issued one by one
  per-wave tile counts: wave w of the 8 owns tiles w, w + 8, ... below T, so T // 8 + 1 tiles on the first T % 8 waves and
      T // 8 on the others; gemm() is compiled per count NTW, NTW - 1, ... and the "deficit" NTW - count picks the copy
  dynamic LDS: two buffers of 16 rows of pitch r32(r16(kmax)) + 4 floats = 128 * (r32(r16(kmax)) + 4) bytes, where kmax is the
      widest stage input or 16-padded MFMA-stage output: max(H + F, r16(H)) forward, r16(H) for the input-gradient chain
  row pitches of the saved activations and gradients: r4(n) = (n + 3) // 4 * 4 floats"""
from tests import gemm_dispatch_table as G

SPLIT_MAX_N = 608            # LinW._pack / plan.hip pack: rows <= 608 && rows % 4 == 0
CHAIN_WAVES = 8              # NW of every ffn_chain_kernel instantiation
CHAIN_NTW = (1, 3, 5)        # <8,1>, <8,3>, <8,5>: tile limits 8, 24, 40
CHAIN_KMAX = 1024            # FFN_KMAX
CHAIN_ROWS = 16              # FROWS
LDS_OPT_IN = 65536           # launches above it need hipFuncAttributeMaxDynamicSharedMemorySize
RR_ERR_UNSUPPORTED = -4

F32 = "f32 layout"
PER_LAYER = "per-layer"

# The ladder: every rung sits on, or one step of 4 past, a boundary of the rules above (200 and 256: the sizes people pick).
# H: (split geometry at M <= 8192 or F32, plan taken, chain <NW,NTW> or PER_LAYER, per-wave tile counts, forward LDS bytes at F = 1)
LADDER = {
    4:    ((4, 4, 8),     True,  (8, 1),    {0, 1}, 4608),       # the smallest H a plan takes: one tile, seven idle waves
    68:   ((10, 10, 8),   True,  (8, 1),    {0, 1}, 12800),      # first N past <4,4,8>
    128:  ((10, 10, 8),   True,  (8, 1),    {1},    20992),      # T = 8: last size of <8,1>, every wave one tile
    132:  ((10, 10, 8),   True,  (8, 3),    {1, 2}, 20992),      # T = 9: first of <8,3>, gemm<NTW-2> and gemm<NTW-1>
    160:  ((10, 10, 8),   True,  (8, 3),    {1, 2}, 25088),      # last N of <10,10,8>
    164:  ((19, 5, 8),    True,  (8, 3),    {1, 2}, 25088),      # first N of <19,5,8>
    200:  ((19, 5, 8),    True,  (8, 3),    {1, 2}, 29184),
    256:  ((19, 5, 8),    True,  (8, 3),    {2},    37376),      # T = 16: gemm<NTW-1> on every wave
    304:  ((19, 5, 8),    True,  (8, 3),    {2, 3}, 41472),      # last N of <19,5,8>
    308:  ((38, 19, 12),  True,  (8, 3),    {2, 3}, 41472),      # first N of <38,19,12>
    384:  ((38, 19, 12),  True,  (8, 3),    {3},    53760),      # T = 24: last size of <8,3>
    388:  ((38, 19, 12),  True,  (8, 5),    {3, 4}, 53760),      # T = 25: first of <8,5>, gemm<NTW-2>
    480:  ((38, 19, 12),  True,  (8, 5),    {3, 4}, 66048),      # first size above 64 KiB of LDS
    512:  ((38, 19, 12),  True,  (8, 5),    {4},    70144),      # T = 32: gemm<NTW-1> on every wave
    608:  ((38, 19, 12),  True,  (8, 5),    {4, 5}, 82432),      # the last split size
    612:  (F32,           True,  (8, 5),    {4, 5}, 82432),      # a plan with every encoder GEMM on the f32 layout
    640:  (F32,           True,  (8, 5),    {5},    86528),      # T = 40: the last size the chain takes
    644:  (F32,           True,  PER_LAYER, None,   None),       # T = 41: the chain refuses inside a plan
    1024: (F32,           True,  PER_LAYER, None,   None),       # and kmax = 1025 > 1024 as well
    150:  (F32,           False, PER_LAYER, None,   None),       # H % 4 != 0: no plan, no shared prefix, scalar gathers
    302:  (F32,           False, PER_LAYER, None,   None),
    610:  (F32,           False, PER_LAYER, None,   None),
}

RUNGS_MULT4 = [h for h in LADDER if h % 4 == 0]
RUNGS_ODD = [h for h in LADDER if h % 4 != 0]


def r4(n):
    return (n + 3) // 4 * 4


def r16(n):
    return (n + 15) & ~15


def r32(n):
    return (n + 31) & ~31


def split_geometry(H, M=4096):
    """<NTP, NT, WAVES> of the encoder's split GEMMs, or F32 where the weights are packed for the f32 MFMA kernels."""
    if H > SPLIT_MAX_N or H % 4 != 0:
        return F32
    return G.geometry(M, H)


def plan_taken(H):
    return H >= 4 and H % 4 == 0


def chain_lds(kmax):
    return 2 * CHAIN_ROWS * (r32(r16(kmax)) + 4) * 4


def chain_of(widths, rowdot=True):
    """rr_ffn_chain_f32's host decision for the stage widths [n_in0, n_out0 = n_in1, ..., n_out_last] of packed, 16-byte
    addressable operands: (status, <NW,NTW>, per-wave tile counts of the widest stage, LDS bytes).  rowdot: the last stage is
    the row-dot form (the forward chain); otherwise every stage is an MFMA stage (the input-gradient chain)."""
    kmax = tmax = 0
    n = len(widths) - 1
    for s in range(n):
        k, o = widths[s], widths[s + 1]
        kmax = max(kmax, k)
        if rowdot and s == n - 1:
            if o > 8 or k % 4 != 0:
                return RR_ERR_UNSUPPORTED, None, None, None
            continue
        if o % 4 != 0:
            return RR_ERR_UNSUPPORTED, None, None, None
        tmax = max(tmax, (o + 15) // 16)
        kmax = max(kmax, r16(o))
    if kmax > CHAIN_KMAX or tmax > CHAIN_WAVES * CHAIN_NTW[-1]:
        return RR_ERR_UNSUPPORTED, None, None, None
    ntw = next(v for v in CHAIN_NTW if tmax <= CHAIN_WAVES * v)
    counts = {sum(1 for g in range(ntw) if w + g * CHAIN_WAVES < tmax) for w in range(CHAIN_WAVES)}
    return 0, (CHAIN_WAVES, ntw), counts, chain_lds(kmax)


def forward_widths(H, F=1, ffn_depth=3, task_num=1):
    return [H + F] + [H] * (ffn_depth - 1) + [task_num]


def backward_widths(H, ffn_depth=3, task_num=1):
    """the input-gradient chain: d scores [M, task_num] back to the H readout columns (appended features have no gradient)"""
    return [task_num] + [H] * ffn_depth


def describe(H, F=1, ffn_depth=3, task_num=1):
    """What the library does with a model of this hidden size: a LADDER row, from the rules."""
    plan = plan_taken(H)
    st, inst, counts, lds = chain_of(forward_widths(H, F, ffn_depth, task_num))
    if not plan or st != 0:
        inst, counts, lds = PER_LAYER, None, None
    return split_geometry(H), plan, inst, counts, lds


def deficits(inst, counts):
    """which compiled copies of gemm() run: NTW - count per wave (a wave with no tile of its own runs none: deficit NTW)"""
    return {inst[1] - c for c in counts}
