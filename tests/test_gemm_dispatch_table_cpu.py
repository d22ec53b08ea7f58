"""Drift guard: the split-GEMM instantiations that tests/gemm_dispatch_table.py lists (and tests/test_gpu_gemm_dispatch.py
runs against f64) are the ones reactranker_amd/csrc/linear_split.hip and wgrad.hip launch.  A new geometry, mode or
epilogue variant in the dispatchers fails here until the table - and with it the GPU sweep - covers it."""
import os
import re

from tests import gemm_dispatch_table as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reactranker_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _block(text, start):
    """The brace-balanced body that follows the first occurrence of `start`."""
    i = text.index(start)
    j = text.index("{", i)
    depth = 0
    for k in range(j, len(text)):
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        if depth == 0:
            return text[j:k + 1]
    raise AssertionError(f"unbalanced block after {start!r}")


def test_split_geometries_are_the_table_s():
    # one ladder, a template over the arithmetic form; both forms (w_packed = 2: three bf16 terms, 3: two f16 terms) take it
    text = _source("linear_split.hip")
    ladder = _block(text, "int launch_split_geometry(")
    assert re.search(r"template <bool F16>\s*int launch_split_geometry\(", text)
    found = re.findall(r"launch_split<(\d+),\s*(\d+),\s*(\d+),\s*F16>\(P,\s*s\)", ladder)
    assert [tuple(int(v) for v in g) for g in found] == T.GEOMETRIES, found
    assert len(re.findall(r"launch_split<", ladder)) == len(T.GEOMETRIES)
    assert len(re.findall(r"launch_split<\d", text)) == len(T.GEOMETRIES)          # no second ladder anywhere
    entry = _block(text, "int rr_linear_split_launch(")
    assert "return two_f16 ? launch_split_geometry<true>(P, s) : launch_split_geometry<false>(P, s);" in entry
    fn = _block(_source("linear.hip"), "int rr_linear_f32(")
    blk = _block(fn, "if (a.w_packed >= 2)")
    assert "return rr_linear_split_launch(args, a.w_packed == 3, stream);" in blk
    assert "launch_split" not in fn.replace("rr_linear_split_launch", "")


def test_split_modes_epilogues_and_persistence_are_the_table_s():
    text = _source("linear_split.hip")
    # launch_split: one launch_split_one per operand MODE
    ls = _block(text, "int launch_split(")
    modes = sorted(int(m) for m in re.findall(r"launch_split_one<NTP,\s*NT,\s*(\d),", ls))
    assert modes == [0, 1, 2, 3]
    assert {leaf[2] for leaf in T.LINEAR_LEAVES} == set(modes)
    # launch_split_one: the epilogue / loader twins EPI 0 .. 3 exist for MODE 0 / 1 of the 12-wave geometry only
    one = _block(text, "int launch_split_one(")
    assert "WAVES == 12 && (MODE == 0 || MODE == 1)" in one
    assert re.search(r"E1\s*=\s*\(WAVES == 12 && \(MODE == 0 \|\| MODE == 1\)\) \? 1 : 0", one)
    assert re.search(r"G\s*=\s*\(WAVES == 12 && \(MODE == 0 \|\| MODE == 1\)\) \? 2 : 0", one)
    # the lean condition: one predicate, used by launch_split_one, launch_split_epi and the kernel
    assert ("constexpr bool split_lean(int k1, int k2) { return k1 + SK <= RR_ZERO_ROW && k2 + SK <= RR_ZERO_ROW; }") in text
    assert text.count("RR_ZERO_ROW && ") == 1                 # written nowhere else
    assert "const bool lean = split_lean(P.a.k1, P.a.k2);" in one
    kernel = _block(text, "linear_split_kernel(const LinearParams P)")
    assert "(LEAN_ONLY || split_lean(a.k1, a.k2))" in kernel
    for leaf in T.LINEAR_LEAVES:
        ntp, nt, mode, waves, epi, persistent = leaf
        assert (ntp, nt, waves) in T.GEOMETRIES
        assert epi == 0 or (waves == 12 and mode in (0, 1))
    assert sorted({l[4] for l in T.LINEAR_LEAVES if l[3] == 12 and l[2] in (0, 1)}) == [0, 1, 2, 3]
    # launch_split_epi: the persistent form's condition
    epi = _block(text, "int launch_split_epi(")
    assert re.search(r"constexpr bool split_can_persist\(int NTP, int NT, int MODE, int WAVES, int EPI\) \{\s*"
                     r"return MODE == 0 && WAVES == 12 && NT == NTP && EPI == 0;\s*\}", text)
    assert "constexpr bool can_persist = split_can_persist(NTP, NT, MODE, WAVES, EPI);" in epi
    assert "constexpr bool CAN_PERSIST = split_can_persist(NTP, NT, MODE, WAVES, EPI);" in kernel
    assert "if (can_persist) {" in epi
    assert "nblk > cus && nk >= 2 && nk % 2 == 0 && split_lean(P.a.k1, P.a.k2)" in epi
    assert "(P.a.M + 16 * WAVES - 1) / (16 * WAVES)" in epi
    assert [l for l in T.LINEAR_LEAVES if l[5]] == [(19, 19, 0, 12, 0, True)]
    # the constants leaf_of uses
    common = _source("linear_common.h")
    assert re.search(r"constexpr int SK = (\d+);", common).group(1) == str(T.SK)
    assert re.search(r"constexpr int RR_ZERO_ROW = (\d+);", common).group(1) == str(T.RR_ZERO_ROW)


def test_wgrad_split_instantiations_are_the_table_s():
    text = _source("wgrad.hip")
    # the kernel launches: written once, for both kernel families and both arithmetic forms (FORM = rr_wgrad_args.split)
    one = _block(text, "void wgrad_launch_one(")
    assert re.search(r"if constexpr \(FORM == 0\) wgrad_fast_kernel<MASK,\s*SUB,\s*WTK><<<", one)
    assert re.search(r"else wgrad_split_kernel<MASK,\s*SUB,\s*WTK,\s*FORM == 2><<<", one)
    assert len(re.findall(r"wgrad_(?:fast|split)_kernel<[^>]*><<<", text)) == 2      # no launch beside these two
    # the wtk ladder and the (mask, sub) ladder, each once
    ladder = _block(text, "void wgrad_launch_wtk(")
    wtks = [int(w) for w in re.findall(r"wgrad_launch_one<FORM,\s*MASK,\s*SUB,\s*(\d)>\(", ladder)]
    assert wtks == [3, 4, 5] and re.findall(r"wtk == (\d)", ladder) == ["3", "4"]
    pick = _block(text, "void wgrad_launch(")
    uses = re.findall(r"wgrad_launch_wtk<FORM,\s*(true|false),\s*(true|false)>\(", pick)
    assert uses == [("true", "true"), ("true", "false"), ("false", "true"), ("false", "false")]
    assert re.findall(r"(?:else )?if \((.*?)\) wgrad_launch_wtk", pick) == ["P.a.mask && P.a.x1_sub", "P.a.mask", "P.a.x1_sub"]
    assert len(re.findall(r"wgrad_launch_one<", text)) == 3 and len(re.findall(r"wgrad_launch_wtk<", text)) == 4
    got = sorted((m == "true", s == "true", w) for m, s in uses for w in wtks)
    assert got == T.WGRAD_SPLIT
    fn = _block(text, "int rr_linear_wgrad_f32(")
    forms = re.findall(r"(?:if \(a\.split == (\d)\) |else )wgrad_launch<(\d)>\(P, grid, s, wtk\);", fn)
    assert forms == [("2", "2"), ("1", "1"), ("", "0")]                            # split = 1: the table's F16 = false form
    assert "wgrad_split_kernel" not in fn and "wgrad_fast_kernel" not in fn      # no second ladder beside the helper
    # the k-block choice leaf_of's companion restates
    assert "const int wtk = per_blk <= 96 ? 3 : (per_blk <= 128 ? 4 : 5);" in fn
    assert "P->kext = P->k1p + k2 + 1;" in text and "P->k1p = (k1 + 3) & ~3;" in text


def test_leaf_of_reaches_every_leaf_and_nothing_else():
    """the restated rules, over a grid of arguments, produce exactly the table (no leaf unreachable, none missing)"""
    seen = set()
    for N in (4, 64, 68, 160, 164, 304, 308, 608):
        for M in (1, 8192, 8193, 60000):
            for k1, k2 in ((300, 0), (1025, 0), (300, 993), (289, 0)):
                for mode in range(4):
                    for res in (False, True):
                        seen.add(T.leaf_of(M, N, k1, k2, mode, res, 256))
    assert seen == set(T.LINEAR_LEAVES)
    assert len(T.LINEAR_LEAVES) == 33 and len(T.WGRAD_SPLIT) == 12
    assert T.leaf_of(60000, 300, 300, 0, 0, False, 256)[5] and not T.leaf_of(60000, 300, 257, 0, 0, False, 256)[5]
    # kext = r4(k1) + k2 + 1 = 93, 97, 129, 161, 193, 257, 321: one block of <= 96 / 128 / 160 columns, two of <= 96 / 128 /
    # 160, three of 107
    assert [T.wgrad_wtk(k, 0) for k in (91, 95, 127, 159, 191, 255, 319)] == [3, 4, 5, 3, 4, 5, 4]
