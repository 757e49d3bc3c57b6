#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of p3d_kernels.hip (tool, CPU only).

usage: tools/isa_compare.py OLD.s NEW.s
The .s files come from the compile of tools/isa_stats.sh (`--cuda-device-only -S`), once per tree.  A kernel counts as
identical when its instruction stream -- comments and directives dropped, block labels renumbered: they carry the
function's ordinal, which moves when kernels are added -- and its VGPR / SGPR / spill / scratch counts are the same.
Prints every kernel that is new, gone or different, then the totals and how many builds of each frame kernel were compared.
"""
import re
import subprocess
import sys


def kernels(path):
    txt = open(path).read()
    body = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        lines = [ln.split(";")[0].strip() for ln in m.group(2).split("\n")]
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", ln) for ln in lines if ln and not ln.startswith(".")]
        body[m.group(1)] = lines
    meta = {}
    for blk in txt.split("- .agpr_count")[1:]:
        def g(k):
            return (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
        meta[g("name")] = (g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"), g("private_segment_fixed_size"))
    return body, meta


def main(old, new):
    a, am = kernels(old)
    b, bm = kernels(new)
    names = sorted(set(a) | set(b))
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    dem = {n: p.replace("p3d::", "") for n, p in zip(names, plain)}
    same = diff = 0
    for n in names:
        if n not in a:
            print("NEW   %-90s insts %5d vgpr %s sgpr %s vspill %s sspill %s scratch %s" % ((dem[n][:90], len(b[n])) + bm.get(n, ("?",) * 5)))
        elif n not in b:
            print("GONE  %s" % dem[n])
        elif a[n] == b[n] and am.get(n) == bm.get(n):
            same += 1
        else:
            diff += 1
            print("DIFF  %-90s insts %d -> %d regs %s -> %s" % (dem[n][:90], len(a[n]), len(b[n]), am.get(n), bm.get(n)))
    print("identical: %d, different: %d" % (same, diff))
    for fam in ("wf_primary_kernel<", "wf_primary_kernel_tiles", "wf_secondary_kernel", "wf_tile_kernel", "whitted_tree_kernel"):
        print("%-28s %3d builds compared" % (fam, sum(1 for n in names if n in a and n in b and fam in dem[n])))
    return 1 if diff else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
