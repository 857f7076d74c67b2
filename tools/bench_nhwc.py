"""Channels-last scoring against the copy route, per native edge and dtype.

    python tools/bench_nhwc.py [--out profiles/bench_nhwc_mi355x.jsonl] [--launches 16] [--edges 2,4,...]
    python tools/bench_nhwc.py --resources     # profiles/nhwc_kernel_resources.txt from the compiler's report

Every (edge, dtype) runs in a child process of its own under `timeout`. Four rotated tensors of about 100 M elements per
shape (together past the 256 MB Infinity Cache), one HIP-event pair per launch, the three routes alternating in blocks:
  (a) energy_nc(x_cl)               the channels-last kernel
  (b) energy_nc(x_cl.contiguous())  the transposing copy inside the timed region: the only route before dcts_energy_nhwc
  (c) energy_nc(x_nchw)             an NCHW tensor of the same shape
One JSON line per shape and dtype: median ms and spread = (max - min) / median of each route. An edge stays in
dcts_has_nhwc_kernel only if b - a exceeds the larger of the two spreads (in ms)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {2: (32768, 512), 4: (16384, 512), 7: (1024, 2048), 8: (4096, 384), 14: (512, 1024), 16: (2048, 192),
          28: (256, 512), 32: (1024, 96), 56: (128, 256)}
DTYPES = ("fp32", "fp16", "bf16")
ROTATE, BLOCK = 4, 4


def child(edge, dt, launches):
    import torch
    import dct_pruning_amd as dpa
    dtype = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[dt]
    N, C = SHAPES[edge]
    g = torch.Generator(device="cuda").manual_seed(edge)
    nchw = [torch.relu(torch.randn(N, C, edge, edge, device="cuda", generator=g)).to(dtype) for _ in range(ROTATE)]
    cl = [x.contiguous(memory_format=torch.channels_last) for x in nchw]
    out = torch.empty(N, C, device="cuda")
    routes = {"a": lambda i: dpa.energy_nc(cl[i], out=out),
              "b": lambda i: dpa.energy_nc(cl[i].contiguous(), out=out),
              "c": lambda i: dpa.energy_nc(nchw[i], out=out)}
    assert dpa.ops.energy_route(cl[0].shape, cl[0].stride()) == dpa.ops.ROUTE_NHWC
    for fn in routes.values():  # warm-up: kernels loaded, workspace and the copy's block allocated
        for i in range(ROTATE):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    k = 0
    for _ in range(launches // BLOCK):
        for name, fn in routes.items():
            for _ in range(BLOCK):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(k % ROTATE)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
                k += 1
    rec = {"edge": edge, "dtype": dt, "N": N, "C": C, "launches": len(times["a"]), "device": torch.cuda.get_device_name(0)}
    for name, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        rec[name + "_ms"] = round(med, 5)
        rec[name + "_spread"] = round((t[-1] - t[0]) / med, 4)
        rec[name + "_all_ms"] = [round(v, 5) for v in times[name]]
    rec["b_minus_a_ms"] = round(rec["b_ms"] - rec["a_ms"], 5)
    rec["larger_spread_ms"] = round(max(rec["a_spread"] * rec["a_ms"], rec["b_spread"] * rec["b_ms"]), 5)
    rec["keep"] = rec["b_minus_a_ms"] > rec["larger_spread_ms"]
    print(json.dumps(rec))


def resources(path):
    """-Rpass-analysis=kernel-resource-usage of nhwc.hip with the Makefile's flags, one line per kernel (no GPU needed)."""
    import re
    csrc = os.path.join(ROOT, "dct_pruning_amd", "csrc")
    flags = re.search(r"^CXXFLAGS = (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).replace("$(ARCH)", "gfx950")
    p = subprocess.run(["hipcc"] + flags.split() + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "nhwc.hip"],
                       cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"k_nhwc_(lane|block)ILi(\d+)ELi(\d)E|k_nhwc_(strip)ILi(\d)E", m.group(2))
            cur = ["k_nhwc_%s<%s, dtype %s>" % (k.group(1), k.group(2), k.group(3)) if k.group(1) else
                   "k_nhwc_strip<56, dtype %s>" % k.group(5)]
            rows.append(cur)
        elif cur is not None:
            cur.append("%s: %s" % (m.group(1), m.group(2)))
    with open(path, "w") as f:
        f.write("# python tools/bench_nhwc.py --resources: -Rpass-analysis=kernel-resource-usage of nhwc.hip (the Makefile's flags, "
                "gfx950); dtype 0 fp32, 1 fp16, 2 bf16\n")
        for r in rows:
            f.write(" | ".join(r) + "\n")
    print("%d kernels -> %s" % (len(rows), path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true", help="write profiles/nhwc_kernel_resources.txt (compiles; no GPU) and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_nhwc_mi355x.jsonl"))
    ap.add_argument("--launches", type=int, default=16)
    ap.add_argument("--edges", default=",".join(str(e) for e in SHAPES))
    ap.add_argument("--child", nargs=2, default=None)
    args = ap.parse_args()
    if args.resources:
        return resources(os.path.join(ROOT, "profiles", "nhwc_kernel_resources.txt"))
    if args.child:
        return child(int(args.child[0]), args.child[1], args.launches)
    with open(args.out, "w") as f:
        for edge in (int(e) for e in args.edges.split(",")):
            for dt in DTYPES:
                p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", str(edge), dt,
                                    "--launches", str(args.launches)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                if p.returncode != 0:  # a fault or a time limit: nothing more is started on the GPU
                    sys.stderr.write(p.stderr[-2000:])
                    sys.exit("bench_nhwc: %d x %d %s ended with status %d; stopping" % (edge, edge, dt, p.returncode))
                line = p.stdout.strip().splitlines()[-1]
                f.write(line + "\n")
                f.flush()
                r = json.loads(line)
                print("%2d %s a %.4f (%.2f) b %.4f (%.2f) c %.4f (%.2f) b-a %.4f / %.4f keep=%s" % (
                    edge, dt, r["a_ms"], r["a_spread"], r["b_ms"], r["b_spread"], r["c_ms"], r["c_spread"], r["b_minus_a_ms"],
                    r["larger_spread_ms"], r["keep"]), flush=True)


if __name__ == "__main__":
    main()
