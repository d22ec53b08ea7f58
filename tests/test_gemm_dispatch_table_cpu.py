"""Drift guard: the split-GEMM instantiations that tests/gemm_dispatch_table.py lists (and tests/test_gpu_gemm_dispatch.py
runs against f64) are the ones reactranker_amd/csrc/linear.hip launches.  A new geometry, mode or epilogue variant in the
dispatcher fails here until the table - and with it the GPU sweep - covers it."""
import os
import re

from tests import gemm_dispatch_table as T

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reactranker_amd", "csrc", "linear.hip")


def _source():
    with open(SRC) as f:
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


def _geometries(block, f16):
    suffix = r",\s*true" if f16 else ""
    found = re.findall(r"launch_split<(\d+),\s*(\d+),\s*(\d+)" + suffix + r">\(P,\s*s\)", block)
    assert found, "no launch_split<...> call found"
    return [tuple(int(v) for v in g) for g in found]


def test_split_geometries_are_the_table_s():
    text = _source()
    fn = _block(text, "int rr_linear_f32(")
    for wp, f16 in ((2, False), (3, True)):
        blk = _block(fn, f"if (a.w_packed == {wp})")
        assert _geometries(blk, f16) == T.GEOMETRIES, (wp, _geometries(blk, f16))


def test_split_modes_epilogues_and_persistence_are_the_table_s():
    text = _source()
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
    assert "P.a.k1 + SK <= RR_ZERO_ROW && P.a.k2 + SK <= RR_ZERO_ROW" in one
    for leaf in T.LINEAR_LEAVES:
        ntp, nt, mode, waves, epi, persistent = leaf
        assert (ntp, nt, waves) in T.GEOMETRIES
        assert epi == 0 or (waves == 12 and mode in (0, 1))
    assert sorted({l[4] for l in T.LINEAR_LEAVES if l[3] == 12 and l[2] in (0, 1)}) == [0, 1, 2, 3]
    # launch_split_epi: the persistent form's condition
    epi = _block(text, "int launch_split_epi(")
    assert "can_persist = MODE == 0 && WAVES == 12 && NT == NTP && EPI == 0" in epi
    assert "nblk > cus && nk >= 2 && nk % 2 == 0 && lean" in epi
    assert "(P.a.M + 16 * WAVES - 1) / (16 * WAVES)" in epi
    assert [l for l in T.LINEAR_LEAVES if l[5]] == [(19, 19, 0, 12, 0, True)]
    # the constants leaf_of uses
    assert re.search(r"constexpr int SK = (\d+);", text).group(1) == str(T.SK)
    assert re.search(r"constexpr int RR_ZERO_ROW = (\d+);", text).group(1) == str(T.RR_ZERO_ROW)


def test_wgrad_split_instantiations_are_the_table_s():
    text = _source()
    fn = _block(text, "int rr_linear_wgrad_f32(")
    macro = re.search(r"#define RR_WSPLIT_LAUNCH\(MASK, SUB, F16\)(.*?)while \(0\)", fn, re.S).group(1)
    wtks = sorted(int(w) for w in re.findall(r"wgrad_split_kernel<MASK,\s*SUB,\s*(\d),\s*F16>", macro))
    assert wtks == [3, 4, 5]
    body = fn[fn.index("} else {", fn.index("if (a.split == 2)")):]
    uses = re.findall(r"RR_WSPLIT_LAUNCH\((true|false),\s*(true|false),\s*false\)", body)
    got = sorted((m == "true", s == "true", w) for m, s in uses for w in wtks)
    assert got == T.WGRAD_SPLIT
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
