"""Per-kernel comparison of two sets of gfx950 device assembly (hipcc <Makefile's CXXFLAGS> --cuda-device-only -S FILE.hip):
which kernels exist on each side, whose instruction streams differ once comments, whitespace and label numbers are
normalised, and every kernel's registers / accumulator offset / scratch / LDS / spill counts side by side.
Usage: python tools/isa_diff.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...] [-v]     (exit status 1 on any difference)"""
import re, subprocess, sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(paths):
    """{symbol: (normalised instruction lines, resources)}; a symbol defined twice is an error"""
    out = {}
    for path in paths:
        text = open(path).read()
        for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
            name, desc = m.group(1), m.group(2)
            assert name not in out, f"{name} defined twice"
            start = text.index(f"\n{name}:") + 1
            raw = text[start:text.index("\n.Lfunc_end", start)]
            body = []
            for line in raw.split("\n")[1:]:
                line = " ".join(line.split(";")[0].split())
                line = re.sub(r"(\.L)?BB\d+_", r"\1BB_", line)
                if line:
                    body.append(line)
            res = {f: int(re.search(rf"\.amdhsa_{f} (\d+)", desc).group(1)) for f in FIELDS}
            res["vgpr_spill"] = raw.count("Folded Spill")
            res["vgpr_reload"] = raw.count("Folded Reload")
            res["sgpr_spill"] = raw.count("SGPR spill to VGPR lane")
            out[name] = (body, res)
    return out


def main(argv):
    verbose = "-v" in argv
    argv = [a for a in argv if a != "-v"]
    cut = argv.index("--")
    old, new = kernels(argv[:cut]), kernels(argv[cut + 1:])
    names = sorted(set(old) | set(new))
    pretty = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    pretty = {n: p.replace("(anonymous namespace)::", "").split("(")[0] for n, p in zip(names, pretty)}
    same = differ = 0
    for n in names:
        if n not in old or n not in new:
            print(f"{'ADDED  ' if n in new else 'MISSING'} {pretty[n]}")
            differ += 1
            continue
        (bo, ro), (bn, rn) = old[n], new[n]
        isa_same, res_same = bo == bn, ro == rn
        same += isa_same and res_same
        differ += not (isa_same and res_same)
        if verbose or not (isa_same and res_same):
            cols = " ".join(f"{k} {ro[k]}|{rn[k]}" for k in ro)
            print(f"{'same   ' if isa_same else 'ISA    '} {'' if res_same else 'RESOURCES '}{pretty[n]}: {len(bo)}|{len(bn)} instructions, {cols}")
    spilling = sum(1 for n in new if new[n][1]["vgpr_spill"])
    print(f"{len(old)} old kernels, {len(new)} new kernels, {same} identical, {differ} different / added / missing; "
          f"{spilling} new kernels with VGPR spills")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
