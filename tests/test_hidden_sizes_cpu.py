"""Drift guard of tests/hidden_sizes.py: the ladder of hidden sizes reaches every branch of the restated dispatch rules, the
table's rows are what the rules give, and the rules' constants are the ones in the sources (reactranker_amd/csrc/ffn.hip,
linear_split.hip, plan.hip and functions.py).  A rung taken off the ladder, or a boundary moved in the sources without the
ladder following, fails here - before tests/test_gpu_hidden_sizes.py would silently stop covering that boundary."""
import os
import re

from tests import gemm_dispatch_table as G
from tests import hidden_sizes as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "reactranker_amd")


def _source(*parts):
    with open(os.path.join(PKG, *parts)) as f:
        return f.read()


def test_the_ladder_is_the_agreed_one():
    assert sorted(L.RUNGS_MULT4) == [4, 68, 128, 132, 160, 164, 200, 256, 304, 308, 384, 388, 480, 512, 608, 612, 640, 644, 1024]
    assert sorted(L.RUNGS_ODD) == [150, 302, 610]
    assert len(L.LADDER) == 22
    # every rung on, or one step of 4 past, a boundary of the rules - except the two sizes people actually pick
    edges = {4, 64, 160, 304, 608} | {16 * L.CHAIN_WAVES * v for v in L.CHAIN_NTW} | {16 * 8 * c for c in (2, 4)} | {L.CHAIN_KMAX}
    first_above_64k = min(h for h in range(4, 1024, 4) if L.chain_lds(max(h + 1, L.r16(h))) > L.LDS_OPT_IN)
    assert first_above_64k == 480
    edges.add(first_above_64k)
    for h in L.RUNGS_MULT4:
        assert h in edges or h - 4 in edges or h in (200, 256), h          # (256 is T = 16 as well)


def test_every_row_of_the_table_is_what_the_rules_give():
    for h, row in L.LADDER.items():
        assert L.describe(h) == row, (h, L.describe(h), row)
        st, inst, counts, lds = L.chain_of(L.forward_widths(h))
        bst, binst, bcounts, blds = L.chain_of(L.backward_widths(h), rowdot=False)
        if h % 4 == 0:                                   # both chains of a size take the same instantiation, or neither
            assert st == bst and inst == binst and counts == bcounts, h
            assert st == (L.RR_ERR_UNSUPPORTED if h in (644, 1024) else 0), h
            if st == 0:
                assert blds == L.chain_lds(L.r16(h)) <= lds
        else:
            assert st == L.RR_ERR_UNSUPPORTED


def test_the_ladder_reaches_every_branch_of_the_rules():
    rows = {h: L.describe(h) for h in L.LADDER}
    # each split geometry of the small-M ladder, and the f32 layout for both of its reasons
    small_m = [g for g in G.GEOMETRIES if g != (19, 19, 12)]               # (<19,19,12>: M > 8192, tests/test_gpu_headline_kernels.py)
    assert {r[0] for r in rows.values() if r[0] != L.F32} == set(small_m)
    assert any(r[0] == L.F32 and h % 4 == 0 for h, r in rows.items()) and any(r[0] == L.F32 and h % 4 for h, r in rows.items())
    for lo in (64, 160, 304, 608):                       # both sides of every N boundary
        assert lo + 4 in rows and (lo in rows or lo == 64), lo             # (64 itself: tests/test_gpu_model.py, test_gpu_plan.py)
        assert L.split_geometry(lo) != L.split_geometry(lo + 4)
    # plan and no plan; chain and per-layer, the latter inside a plan and without one
    assert {r[1] for r in rows.values()} == {True, False}
    assert any(r[1] and r[2] == L.PER_LAYER for r in rows.values()) and any(not r[1] for r in rows.values())
    # each chain instantiation with each tile-count deficit it can produce: the counts of T = 1 .. 40 tiles
    can = {}
    for T in range(1, L.CHAIN_WAVES * L.CHAIN_NTW[-1] + 1):
        st, inst, counts, _ = L.chain_of([16 * T + 1, 16 * T, 16 * T, 1])
        assert st == 0
        can.setdefault(inst, set()).update(L.deficits(inst, counts))
    assert can == {(8, 1): {0, 1}, (8, 3): {0, 1, 2}, (8, 5): {0, 1, 2}}    # (gemm<NTW-3>, <NTW-4>: narrower stages of a mixed chain only)
    got = {}
    for r in rows.values():
        if r[2] != L.PER_LAYER:
            got.setdefault(r[2], set()).update(L.deficits(r[2], r[3]))
    assert got == can
    # ... and each instantiation with all waves on one count as well as split between two
    for inst in can:
        kinds = {len(r[3]) for r in rows.values() if r[2] == inst}
        assert kinds == {1, 2}, (inst, kinds)
    # both sides of the 64 KiB opt-in, inside ONE instantiation (what launch_chain's per-instantiation record has to survive)
    big = sorted(r[4] for r in rows.values() if r[2] == (8, 5))
    assert big[0] <= L.LDS_OPT_IN < big[1] and len({b for b in big if b > L.LDS_OPT_IN}) >= 3
    assert all(r[4] <= L.LDS_OPT_IN for r in rows.values() if r[2] in ((8, 1), (8, 3)))
    # the chain's own limits from both sides
    assert rows[640][2] == (8, 5) and rows[644][2] == L.PER_LAYER
    assert L.chain_of([1024, 640, 1])[0] == 0 and L.chain_of([1028, 640, 1])[0] == L.RR_ERR_UNSUPPORTED
    assert L.chain_of([1024, 640, 1])[3] == 131584


def test_restated_constants_are_the_sources():
    ffn = _source("csrc", "ffn.hip")
    assert re.search(r"constexpr int FROWS = (\d+);", ffn).group(1) == str(L.CHAIN_ROWS)
    assert "constexpr int f_r16(int k) { return (k + 15) & ~15; }" in ffn
    assert "constexpr int f_pitch(int kmax) { return ((kmax + 31) & ~31) + 4; }" in ffn
    assert re.search(r"constexpr int FFN_KMAX = (\d+);", ffn).group(1) == str(L.CHAIN_KMAX)
    tmax = int(re.search(r"constexpr int FFN_TMAX = (\d+);", ffn).group(1))
    assert "if (kmax > FFN_KMAX || tmax > FFN_TMAX) return RR_ERR_UNSUPPORTED;" in ffn
    ladder = re.findall(r"(?:if \(tmax <= (\d+)\) )?return launch_chain<(\d+), (\d+)>\(P, lds, s\);", ffn)
    assert [(int(w), int(n)) for _, w, n in ladder] == [(L.CHAIN_WAVES, v) for v in L.CHAIN_NTW], ladder
    limits = [int(t) for t, _, _ in ladder[:-1]] + [tmax]
    assert limits == [L.CHAIN_WAVES * v for v in L.CHAIN_NTW] == [8, 24, 40]
    assert "return static_cast<size_t>(2) * FROWS * f_pitch(f_r16(kmax)) * sizeof(float);" in ffn
    assert "P.pitch = f_pitch(f_r16(kmax));" in ffn and "const size_t lds = f_lds_bytes(kmax);" in ffn
    assert L.chain_lds(1024) == 128 * 1028 == 131584
    # gemm() is compiled for NTW, NTW - 1, ... NTW - 4
    assert [int(d) for d in re.findall(r"ntw == NTW - (\d)\) gemm\(", ffn)] == [1, 2, 3, 4] and "if (ntw == NTW) gemm(" in ffn
    # the opt-in is asked for at the largest admissible size, once per device, under an atomic
    chain = ffn[ffn.index("int launch_chain("):ffn.index("inline bool f_vec_ok")]
    assert "static std::atomic<uint64_t> configured{0};" in chain and "static bool configured" not in ffn
    assert "static_cast<int>(f_lds_bytes(FFN_KMAX))" in chain and "static_cast<int>(lds)" not in chain
    assert f"lds > {L.LDS_OPT_IN} &&" in chain
    # the split ladder's N boundaries (the tuples themselves: tests/test_gemm_dispatch_table_cpu.py)
    split = _source("csrc", "linear_split.hip")
    geo = split[split.index("int launch_split_geometry("):]
    assert [int(n) for n in re.findall(r"a\.N <= (\d+)", geo[:geo.index("}  // namespace")])] == [64, 160, 304, 304]
    assert [L.split_geometry(n) for n in (64, 68, 160, 164, 304, 308, 608)] == \
        [(4, 4, 8), (10, 10, 8), (10, 10, 8), (19, 5, 8), (19, 5, 8), (38, 19, 12), (38, 19, 12)]
    # the last split size, in the plan and in the per-op mirror
    plan = _source("csrc", "plan.hip")
    assert f"const bool split = c.split && big && rows <= {L.SPLIT_MAX_N} && rows % 4 == 0;" in plan
    assert f"split = SplitGemm.enabled and self.big and rows <= {L.SPLIT_MAX_N} and rows % 4 == 0" in _source("functions.py")
    assert L.split_geometry(612) == L.split_geometry(606) == L.F32
    # who takes a plan, and the pitch of everything the plans and the tests allocate
    assert "RR_CHECK_ARG(m->H >= 4 && m->H % 4 == 0 &&" in plan
    assert 'st["H"] % 4 != 0' in _source("functions.py")
    assert "inline int64_t r4(int64_t n) { return (n + 3) / 4 * 4; }" in plan
    assert [L.r4(n) for n in (1, 4, 5, 301, 611)] == [4, 4, 8, 304, 612]
    assert not L.plan_taken(610) and L.plan_taken(4) and not L.plan_taken(0)
