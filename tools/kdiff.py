#!/usr/bin/env python3
"""CPU only: compare the kernels of two sets of gfx950 code objects, a parent's against a candidate's.

usage: tools/kdiff.py PARENT.co[,MORE.co] CANDIDATE.co[,MORE.co]
(code objects: hipcc <the Makefile's KFLAGS> --cuda-device-only --no-gpu-bundle-output -c FILE.hip -o FILE.co)
Prints whether the kernel names are the same, how many kernels differ in bytes, and every kernel whose figures
(VGPR, SGPR, VGPR / SGPR spills, private segment, LDS, kernarg) differ, with its waves per SIMD before and after
(min(8, 512 // (VGPRs rounded up to 8))).  Exit status 1 if names differ or a kernel gained a spill, scratch or lost a wave.
"""
import re, subprocess, sys
LLVM = "/opt/rocm/lib/llvm/bin/"
KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size")
run = lambda *a: subprocess.run(a, capture_output=True, text=True, check=True).stdout

def load(paths):
    code, figs = {}, {}
    for co in paths.split(","):
        subprocess.check_call([LLVM + "llvm-objcopy", "-O", "binary", "--only-section=.text", co, co + ".text"])
        text = open(co + ".text", "rb").read()
        base = int(re.search(r"\.text\s+PROGBITS\s+([0-9a-f]+)", run(LLVM + "llvm-readelf", "-SW", co)).group(1), 16)
        for f in (l.split() for l in run(LLVM + "llvm-readelf", "-sW", co).splitlines()):
            if len(f) >= 8 and f[3] == "FUNC":
                code[f[7]] = text[int(f[1], 16) - base:int(f[1], 16) - base + int(f[2])]
        for blk in run(LLVM + "llvm-readelf", "--notes", co).split("- .agpr_count")[1:]:
            g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
            figs[re.search(r"\.name:\s+(\S+)", blk).group(1)] = tuple(g(k) for k in KEYS)
    return code, figs

waves = lambda vgprs: min(8, 512 // max(8, (vgprs + 7) // 8 * 8))
(a, fa), (b, fb) = load(sys.argv[1]), load(sys.argv[2])
bad = set(a) != set(b)
print("kernels: %d -> %d, same names: %s" % (len(a), len(b), not bad))
for n in sorted(set(a) ^ set(b)): print("  only in", "parent:" if n in a else "candidate:", n)
both = [n for n in a if n in b]
print("identical bytes: %d, different: %d (longer: %d, shorter: %d)" % (
    sum(a[n] == b[n] for n in both), sum(a[n] != b[n] for n in both),
    sum(len(b[n]) > len(a[n]) for n in both), sum(len(b[n]) < len(a[n]) for n in both)))
changed = [n for n in both if fa[n] != fb[n]]
print("figures (%s) differ in %d kernels" % (" ".join(KEYS), len(changed)))
demangle = dict(zip(changed, run("c++filt", *changed).splitlines())) if changed else {}
for n in changed:
    worse = any(fb[n][i] > fa[n][i] for i in (2, 3, 4)) or waves(fb[n][0]) < waves(fa[n][0])
    bad |= worse
    print("  %s %s\n      %s -> %s, waves/SIMD %d -> %d" % ("WORSE" if worse else "     ", demangle[n], fa[n], fb[n], waves(fa[n][0]), waves(fb[n][0])))
sys.exit(1 if bad else 0)
