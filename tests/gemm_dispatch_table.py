"""The kernel instantiations the split-GEMM dispatchers of reactranker_amd/csrc (linear_split.hip, wgrad.hip) can reach, by hand,
and a pure-Python restatement of the rules that pick one (no GPU, no library needed: tests/test_gemm_dispatch_table_cpu.py
holds the tables against the sources, tests/test_gpu_gemm_dispatch.py runs every entry against f64).

Rules restated (linear_split.hip; the last one wgrad.hip):
  launch_split_geometry (rr_linear_f32 with w_packed = 2 / 3): the geometry <NTP, NT, WAVES> by N and M
      N <= 64 -> <4,4,8>;  N <= 160 -> <10,10,8>;  N <= 304 and M <= 8192 -> <19,5,8>;  N <= 304 -> <19,19,12>;  else <38,19,12>
  launch_split: MODE 3 (a_mask_bits) before 2 (a_mask) before 1 (a1_sub) before 0
  launch_split_one: the 12-wave geometry, MODE 0 / 1 only - EPI 1 / 3 with a residual (RR_EPI_MODE 1), EPI 2 / 3 when a
      segment does not fit the lean loader (k1 + SK > RR_ZERO_ROW or k2 + SK > RR_ZERO_ROW, i.e. K > 992); EPI 0 otherwise
  launch_split_epi: the persistent form of <NT,NT,0,12,0> when the row blocks of 16 * WAVES rows outnumber the CUs, the
      number of k-steps r32(k1) / SK + r32(k2) / SK is even and >= 2, and both segments fit the lean loader
  rr_linear_wgrad_f32, split = 1: wgrad_split_kernel<MASK, SUB, WTK, false>, WTK from the narrowest k-block (96 / 128 / 160
      columns) that covers kext = r4(k1) + k2 + 1 with ceil(kext / 160) blocks; any operand that is not 16-byte
      addressable (leading dimension % 4, base pointer) or N % 4 != 0 sends the request to the scalar wgrad_kernel"""

SK = 32                  # k per step of the split kernels
RR_ZERO_ROW = 1024       # floats of rr_zero_row: the lean loader's reach

# <NTP, NT, WAVES> of rr_linear_f32's split blocks, in dispatch order
GEOMETRIES = [(4, 4, 8), (10, 10, 8), (19, 5, 8), (19, 19, 12), (38, 19, 12)]

# every linear_split_kernel launch the w_packed = 2 dispatcher can make: (NTP, NT, MODE, WAVES, EPI, persistent)
LINEAR_LEAVES = sorted(
    [(ntp, nt, mode, w, 0, False) for ntp, nt, w in GEOMETRIES if w == 8 for mode in range(4)]
    + [(ntp, nt, mode, 12, epi, False) for ntp, nt, w in GEOMETRIES if w == 12 for mode in (0, 1) for epi in range(4)]
    + [(ntp, nt, mode, 12, 0, False) for ntp, nt, w in GEOMETRIES if w == 12 for mode in (2, 3)]
    + [(19, 19, 0, 12, 0, True)])

# wgrad_split_kernel<MASK, SUB, WTK, F16 = false> (rr_wgrad_args.split = 1)
WGRAD_SPLIT = sorted((mask, sub, wtk) for mask in (False, True) for sub in (False, True) for wtk in (3, 4, 5))


def r32(k):
    return (k + 31) & ~31


def geometry(M, N):
    if N <= 64:
        return (4, 4, 8)
    if N <= 160:
        return (10, 10, 8)
    if N <= 304 and M <= 8192:
        return (19, 5, 8)
    if N <= 304:
        return (19, 19, 12)
    return (38, 19, 12)


def lean(k1, k2):
    return k1 + SK <= RR_ZERO_ROW and k2 + SK <= RR_ZERO_ROW


def leaf_of(M, N, k1, k2, mode, residual, n_cu):
    """The (NTP, NT, MODE, WAVES, EPI, persistent) that rr_linear_f32 launches for a w_packed = 2 call (N <= 608, every
    operand 16-byte addressable): rr_linear_f32's w_packed == 2 block, launch_split_one and launch_split_epi."""
    ntp, nt, waves = geometry(M, N)
    epi = 0
    if waves == 12 and mode in (0, 1):
        epi = (0 if lean(k1, k2) else 2) + (1 if residual else 0)
    persistent = False
    if mode == 0 and waves == 12 and nt == ntp and epi == 0:
        nblk = (M + 16 * waves - 1) // (16 * waves)
        nk = r32(k1) // SK + r32(k2) // SK
        persistent = nblk > n_cu and nk >= 2 and nk % 2 == 0 and lean(k1, k2)
    return (ntp, nt, mode, waves, epi, persistent)


def wgrad_wtk(k1, k2):
    """rr_linear_wgrad_f32's k-block width (3, 4, 5 MFMA tiles of 32 columns: 96 / 128 / 160) for a [k1 | k2] operand."""
    kext = ((k1 + 3) & ~3) + k2 + 1
    nblk = (kext + 159) // 160
    per = (kext + nblk - 1) // nblk
    return 3 if per <= 96 else (4 if per <= 128 else 5)


def leaf_name(leaf):
    ntp, nt, mode, w, epi, persistent = leaf
    return f"<{ntp},{nt},{mode},{w},{epi}>" + (" persistent" if persistent else "")
