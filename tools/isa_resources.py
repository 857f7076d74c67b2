#!/usr/bin/env python3
"""Per-kernel resources from `make isa` listings (csrc/_obj/<unit>.s): static VALU instructions, VGPRs, scratch,
waves per SIMD and LDS, one line per kernel; with two directories, the kernels whose figures differ side by side.

  tools/isa_resources.py <dir with *.s>                 table of every kernel of every unit
  tools/isa_resources.py <parent dir> <this dir>        differences, unit sums of VALU, and the conditions of a
                                                        change that must cost no scratch and no wave per SIMD
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = (("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
          ("occ", r"; Occupancy: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"))


def parse(path):
    """{mangled kernel name: dict(valu, vgpr, agpr, scratch, occ, lds)} of one listing."""
    out, sym, valu, info = {}, None, 0, None
    for line in open(path):
        m = re.match(r"\s+\.type\s+(\S+),@function", line)
        if m:
            sym, valu, info = m.group(1), 0, None
        elif re.match(r"\s+v_", line):
            valu += 1
        elif line.startswith("; Kernel info:") and sym:
            info = {"valu": valu}
            out[sym] = info
        elif info is not None:
            for key, pat in FIELDS:
                m = re.match(pat, line)
                if m:
                    info[key] = int(m.group(1))
    return out


def load(d):
    res = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        unit = os.path.basename(path)[:-2]
        for sym, info in parse(path).items():
            res[(unit, sym)] = info
    return res


def demangle(syms):
    txt = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    clean = lambda s: re.sub(r"\(.*", "", s.replace("void (anonymous namespace)::", "")).replace("dcts::", "")
    return dict(zip(syms, map(clean, txt)))


def row(i):
    return "valu=%5d vgpr=%3d agpr=%3d scratch=%3d occ=%d lds=%6d" % (i["valu"], i["vgpr"], i.get("agpr", 0), i["scratch"],
                                                                    i["occ"], i.get("lds", 0))


def main(argv):
    a = load(argv[1])
    names = demangle(sorted({s for _, s in a}))
    if len(argv) == 2:
        for (unit, sym), i in sorted(a.items()):
            print("%-8s %-60s %s" % (unit, names[sym], row(i)))
        return 0
    b = load(argv[2])
    units = {u for u, _ in a} & {u for u, _ in b}  # a directory may hold the listings of some units only
    a = {k: i for k, i in a.items() if k[0] in units}
    b = {k: i for k, i in b.items() if k[0] in units}
    assert set(a) == set(b), "the two trees hold different kernels"
    print("# static VALU per unit: parent -> this tree")
    for unit in sorted({u for u, _ in a}):
        sa = sum(i["valu"] for (u, _), i in a.items() if u == unit)
        sb = sum(i["valu"] for (u, _), i in b.items() if u == unit)
        print("%-10s %7d -> %7d  %+.1f %%" % (unit, sa, sb, 100.0 * (sb - sa) / max(sa, 1)))
    same = sum(a[k] == b[k] for k in a)
    print("# %d kernels, %d with identical figures; the others, parent then this tree:" % (len(a), same))
    for k in sorted(a):
        if a[k] == b[k]:
            continue
        flag = ""
        if b[k]["scratch"] > a[k]["scratch"]:
            flag += "  GAINS SCRATCH"
        if b[k]["occ"] < a[k]["occ"]:
            flag += "  LOSES A WAVE"
        if b[k]["occ"] > a[k]["occ"]:
            flag += "  gains a wave"
        print("%-8s %s%s\n    %s\n    %s" % (k[0], names[k[1]], flag, row(a[k]), row(b[k])))
    print("# kernels that gain scratch: %d; kernels that lose a wave per SIMD: %d" % (
        sum(b[k]["scratch"] > a[k]["scratch"] for k in a), sum(b[k]["occ"] < a[k]["occ"] for k in a)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
