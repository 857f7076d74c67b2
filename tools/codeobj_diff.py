#!/usr/bin/env python3
"""Device code of two builds of libdctscore.so, compared per kernel symbol ("Device code across the whole
change"): tools/codeobj_diff.py <before.so> <after.so> [--list].

The gfx950 code objects are the bundles of the .hip_fatbin section, split at the __CLANG_OFFLOAD_BUNDLE__ headers: one per
translation unit, in link order. Each goes through `llvm-objdump -d --no-show-raw-insn` and `llvm-readelf --notes`; per
kernel the instruction stream, the register / LDS / scratch / kernarg figures of the metadata and the 64 descriptor bytes
without the entry offset are compared. Prints identical / different / missing / new per code object and kernel template;
--list names every kernel that differs. Needs no GPU."""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".wavefront_size", ".max_flat_workgroup_size", ".vgpr_spill_count", ".sgpr_spill_count")


def code_objects(path):
    data = open(path, "rb").read()
    out = []
    for m in re.finditer(MAGIC, data):
        base = m.start()
        (n,) = struct.unpack_from("<Q", data, base + len(MAGIC))
        o = base + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, o)
            triple = data[o + 24:o + 24 + tlen]
            o += 24 + tlen
            if b"gfx950" in triple and size:
                out.append(data[base + off:base + off + size])
    return out


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def kernels(obj):
    """{symbol: (instruction stream, metadata figures, descriptor bytes)} of one code object"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(obj)
        f.flush()
        dis, notes, syms, secs = (tool("llvm-objdump", "-d", "--no-show-raw-insn", f.name), tool("llvm-readelf", "--notes", f.name),
                                  tool("llvm-readelf", "-sW", f.name), tool("llvm-readelf", "-SW", f.name))
    streams, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = streams.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())  # without the address comment; branch targets are symbol-relative
    meta = {}
    for block in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        block = ".agpr_count" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = tuple(re.search(re.escape(k) + r":\s+(\S+)", block).group(1) if k in block else None for k in META)
    rodata = next(l for l in secs.splitlines() if re.search(r"\]\s+\.rodata\s", l)).split("]")[1].split()
    addr, off = int(rodata[2], 16), int(rodata[3], 16)
    out = {}
    for line in syms.splitlines():
        p = line.split()
        if len(p) == 8 and p[7].endswith(".kd"):
            name = p[7][:-3]
            kd = obj[off + int(p[1], 16) - addr:][:64]
            out[name] = ("\n".join(streams[name]), meta[name], kd[:16] + kd[24:])  # bytes 16-23: the entry offset
    return out


def template(sym):
    name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    return re.sub(r"[<(].*", "", name)


def main():
    before, after = code_objects(sys.argv[1]), code_objects(sys.argv[2])
    print("code objects: %d before, %d after" % (len(before), len(after)))
    total = collections.Counter()
    for i, (a, b) in enumerate(zip(before, after)):
        if a == b:
            n = len(kernels(a))
            total["identical"] += n
            print("object %2d: %4d kernels, bytes identical" % (i, n))
            continue
        ka, kb = kernels(a), kernels(b)
        per = collections.defaultdict(collections.Counter)
        for s in sorted(set(ka) | set(kb)):
            what = "missing" if s not in kb else "new" if s not in ka else "identical" if ka[s] == kb[s] else "different"
            per[template(s)][what] += 1
            total[what] += 1
            if "--list" in sys.argv and what != "identical":
                why = "" if what != "different" else " (%s)" % ", ".join(
                    w for w, x, y in zip(("code", "metadata", "descriptor"), ka[s], kb[s]) if x != y)
                print("    %s %s%s" % (what, s, why))
        print("object %2d: %4d kernels before, %4d after" % (i, len(ka), len(kb)))
        for t, c in sorted(per.items()):
            print("    %-28s %s" % (t, ", ".join("%d %s" % (c[w], w) for w in ("identical", "different", "missing", "new") if c[w])))
    print("total: " + ", ".join("%d %s" % (total[w], w) for w in ("identical", "different", "missing", "new")))
    return 0 if len(before) == len(after) else 1


if __name__ == "__main__":
    sys.exit(main())
