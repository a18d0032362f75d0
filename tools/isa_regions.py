"""Static VALU instructions per region of a kernel in an amdgcn .s file (tooling, not product code): the kernel's
text is split at its workgroup barriers, and the vector-ALU instructions of each region are counted by class (FP64,
FP32, integer, compare / select, moves, other). For the pencil kernels (gls_brick_pencil.hip) the largest region holds
the sweeps and the pointwise algebra; what precedes it is the set-up and the gather (PRO: and the prolongation stages),
what follows it the reduction / scatter / restriction. The text order of the .s file stands in for the execution
order (loops count once).

Usage: python tools/isa_regions.py file.s [kernel-substring] [--all]
  --all: one line per barrier-delimited region instead of the before / sweeps / after summary"""
import collections
import re
import sys

CLASSES = ("fp64", "fp32", "int", "cmp_sel", "mov", "other")


def valu_class(op):
    if not op.startswith("v_"):
        return None
    if op.startswith(("v_cmp", "v_cndmask")):
        return "cmp_sel"
    if op.startswith(("v_mov", "v_readfirstlane", "v_readlane", "v_writelane", "v_accvgpr", "v_swap")):
        return "mov"
    if op.startswith("v_cvt"):
        return "other"
    if re.search(r"_f64($|_)", op):
        return "fp64"
    if re.search(r"_f32($|_)", op):
        return "fp32"
    if re.search(r"_(u|i|b)(16|24|32|64)($|_)", op) or op.startswith(("v_bfe", "v_bfi", "v_bfm", "v_bcnt", "v_mbcnt",
                                                                       "v_lshl", "v_lshr", "v_ashr", "v_and", "v_or",
                                                                       "v_xor", "v_not", "v_perm", "v_alignbit")):
        return "int"
    return "other"


def regions(body):
    """[Counter per barrier-delimited region]"""
    out = [collections.Counter()]
    for line in body:
        t = line.strip().split()
        if not t or t[0].startswith((".", ";")) or t[0].endswith(":"):
            continue
        if t[0] == "s_barrier":
            out.append(collections.Counter())
            continue
        c = valu_class(t[0])
        if c:
            out[-1][c] += 1
    return out


def fmt(c):
    return "%5d VALU (" % sum(c.values()) + ", ".join("%s %d" % (k, c[k]) for k in CLASSES if c[k]) + ")"


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lines = open(args[0]).read().split("\n")
    sub = args[1] if len(args) > 1 else ""
    for s in [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and sub in l]:
        e = s
        while "s_endpgm" not in lines[e]:
            e += 1
        reg = regions(lines[s:e])
        print(lines[s].split(":")[0])
        if "--all" in sys.argv:
            for i, c in enumerate(reg):
                print("   region %d: %s" % (i, fmt(c)))
            continue
        big = max(range(len(reg)), key=lambda i: sum(reg[i].values()))
        tot = lambda rs: sum(rs, collections.Counter())
        print("   before the sweeps (%d regions): %s" % (big, fmt(tot(reg[:big]))))
        print("   sweeps + pointwise            : %s" % fmt(reg[big]))
        print("   after the sweeps (%d regions) : %s" % (len(reg) - big - 1, fmt(tot(reg[big + 1:]))))
        print("   kernel                        : %s" % fmt(tot(reg)))


if __name__ == "__main__":
    main()
