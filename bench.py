#!/usr/bin/env python3
"""bench.py — DCT+score throughput of the hot path on synthetic ResNet-50 feature maps.

Workload (BASELINE.json configs[3], the one the metric's 1/2/4/8-GPU figures are quoted on):
the 49 hooked tensors of imp_score for resnet_50 (utils/common.py:557-607; shapes in
dct_pruning_amd/schedules.py) at batch 256, fp32, synthetic, resident in HBM
before the clock starts. One STEP = one batch pass of the hot path: one DCT+energy launch per tile
shape covering every hooked tensor of that shape (dcts_energy_multi_f32: [N,C,H,W] -> [N,C] each;
`--per-tensor` launches them one by one as the per-hook harness does), then one batch-sum /
running-mean launch covering all hooked tensors (utils/common.py:265-277). After the K timed steps (= `--limit K` batches) multi-GPU runs do
the path's single exchange: one RCCL all-gather of the flat score buffer; it is inside the
timed region.

N > 1: layer/channel-range units are LPT-sharded over the ranks (dct_pruning_amd/sharding.py);
total work is fixed, so scaling = "strong".

Prints ONE JSON line on rank 0: `value` (Mmaps/s over the K timed steps) and `ms_per_step`. A plain
run does nothing else: set-up, `--warmup` steps, the `--steps` timed steps, `--dump-outputs` if given,
the line. `--full` adds `roofline` for the dominant kernel (the 56x56 codelet kernel, measured with
HIP events on the launch stream inside the timed region), the Parseval and dead-channel checks of
the result, `all_gather_ms` (N > 1), the `headline` micro-benchmarks and `cpu_baseline` (the
oracle's per-map loop on a bounded sample).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak
CFG_ID = 4


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="default 20; 200 for workloads whose step is under 1 GB (the CIFAR nets: a step is ~50 us, "
                         "20 of them would be timed against the fixed cost of the final barrier)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="default 256 (u2netp: 12, README.md:222 of the reference)")
    ap.add_argument("--net", default="resnet_50")
    ap.add_argument("--input-size", type=int, default=None,
                    help="u2netp only: input crop edge (reference crop 288, BASELINE config 5 names 320)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: `roofline` (HIP events around "
                         "the dominant kernel inside the timed region), the Parseval and dead-channel checks of the result, "
                         "`all_gather_ms`, the `headline` micro-benchmarks and `cpu_baseline`")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out cpu_baseline")
    ap.add_argument("--no-headline", action="store_true", help="with --full: leave out the headline micro-benchmarks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed as DIR/<name>.npy (float32): "
                         "`scores` (the per-channel running means of every hook point, concatenated in hook order) and "
                         "`energy` (the last step's per-map energies [batch, channels] of rank 0's tensors); at most "
                         "64 MiB in all, beyond that a fixed seeded sample of the flattened array")
    ap.add_argument("--per-tensor", action="store_true",
                    help="one energy launch per hooked tensor (default: one dcts_energy_multi_f32 launch per tile shape)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--pmc-calib", action="store_true",
                    help="(tools/profile_bench_pmc.sh) run the known-size calibration read first, so a PMC pass of "
                         "this process can correct FETCH_SIZE")
    return ap.parse_args()


def synth(n, c, h, w, seed, device):
    """relu(randn) * exp(0.5 randn) per channel, channels c % 8 == 5 dead."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g, device=device)
    x.relu_()
    s = torch.exp(0.5 * torch.randn(c, generator=g, device=device))
    s[torch.arange(c, device=device) % 8 == 5] = 0
    x.mul_(s[None, :, None, None])
    return x


class BoundUnit:
    """One work unit with its launches pre-bound (ctypes argument tuples built once)."""

    def __init__(self, lib, x, pad, stream_ptr, ws):
        n, c, h, w = x.shape
        self.x = x
        self.h = h
        self.nmaps = n * c
        self.bytes = self.nmaps * (4 * h * w + 4)  # algorithmic bytes, SURVEY.md §8(d)
        self.energy = torch.empty((n, c), dtype=torch.float32, device=x.device)
        self.fr = torch.zeros(c, dtype=torch.float32, device=x.device)
        self.total = 0.0
        self.n = n
        self._lib = lib
        self._stream = stream_ptr
        self._eargs = (x.data_ptr(), n, c, h, w, x.stride(0), x.stride(1), x.stride(2), x.stride(3),
                       0, c, 1 if pad else 0, self.energy.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr)

    def launch_energy(self):
        rc = self._lib.dcts_energy_f32(*self._eargs)
        if rc:
            raise RuntimeError("dcts_energy_f32 -> %d" % rc)

    def launch_update(self):
        rc = self._lib.dcts_running_mean_update_f32(self.energy.data_ptr(), self.n, self.fr.numel(),
                                                    self.fr.data_ptr(), self.total, self._stream)
        if rc:
            raise RuntimeError("dcts_running_mean_update_f32 -> %d" % rc)
        self.total += self.n


def cpu_baseline(points, seconds):
    """The reference CPU path on this box's host cores, two legs:
    * value (kind "port"): the oracle's restatement of the reference loop (utils/common.py:265-277: one
      dct_2d + sum + .item() per map in a Python list comprehension) on whole samples of the same hooked
      tensors. One thread: the loop is serial Python around ~25 tiny torch ops per map, more threads do not
      make it faster (torch's intra-op pool has nothing to chew on at 56x56) - that IS the reference's CPU path;
    * batched: the best this host does with the same arithmetic when the Python loop is removed: one
      batched FFT-DCT over all maps of a tensor, every core torch can use, >= 64 samples per tensor, 3 reps."""
    from oracle import dct_oracle as orc
    from dct_pruning_amd import schedules

    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(99)
    tensors = []
    for pt in points:
        cb, cc, pad = schedules.scored_shape(pt)
        tensors.append((torch.relu(torch.randn(1, cc, pt.H, pt.W, generator=g)), pt.kind))
    maps = 0
    t0 = time.perf_counter()
    reps = 0
    while True:
        for x, kind in tensors:
            st = orc.HookState()
            if kind == "full":
                orc.get_feature_hook(st, x)
            elif kind == "last12":
                orc.get_feature_hook_densenet(st, x)
            else:
                orc.get_feature_hook_u2net_input(st, (x,))
            maps += x.shape[0] * x.shape[1]
        reps += 1
        if time.perf_counter() - t0 >= seconds or reps >= 8:
            break
    dt = time.perf_counter() - t0
    # the vectorised leg
    ncpu = os.cpu_count() or 1
    try:
        ncpu = len(os.sched_getaffinity(0))  # what this process may actually use
    except (AttributeError, OSError):
        pass
    # a one-GPU box of this pool shares a 256-CPU host: its share is 16 CPUs per GPU; torch's intra-op pool
    # on more threads than that share only contends (an unbounded pool made this leg take minutes)
    ncpu = max(1, min(ncpu, int(os.environ.get("DCTS_BENCH_CPU_THREADS", "32"))))
    torch.set_num_threads(ncpu)
    nsamp = 64
    per_sample = sum(x.shape[1] * x.shape[2] * x.shape[3] * 4 for x, _ in tensors)
    while nsamp > 8 and nsamp * per_sample > 6e9:  # bound the host memory of a pass (U2-Net-p: 165 MB per sample)
        nsamp //= 2
    best, bmaps, passes, tb0 = None, 0, 0, time.perf_counter()
    for _ in range(3):
        t1 = time.perf_counter()
        bmaps = 0
        for x, kind in tensors:
            orc.energy_nc_batched(x.expand(nsamp, -1, -1, -1).contiguous(), pad_front_if_odd=(kind != "full"))
            bmaps += nsamp * x.shape[1]
        dtb = time.perf_counter() - t1
        best = dtb if best is None else min(best, dtb)
        passes += 1
        if time.perf_counter() - tb0 > 20.0:  # keep the default bench run within minutes
            break
    return {
        "value": maps / dt / 1e6, "unit": "Mmaps/s", "cores": 1, "kind": "port",
        "sample": "%d x (1 sample of the %d hooked tensors = %d maps), per-map Python loop of oracle.get_feature_hook "
                  "(restates utils/common.py:265-277), torch CPU, 1 thread because the loop is serial Python, %.1f s"
                  % (reps, len(tensors), maps // reps, dt),
        "batched": {"value": bmaps / best / 1e6, "unit": "Mmaps/s", "cores": ncpu, "torch_threads": torch.get_num_threads(),
                    "sample": "%d samples per tensor (%d maps per pass), one batched FFT-DCT per tensor "
                              "(oracle.energy_nc_batched), best of %d passes, %.1f s per pass" % (nsamp, bmaps, passes, best)},
        "host_cpus": os.cpu_count(),
    }


def lib_sha256():
    """Content hash of the library this process runs (stamps profiles/pmc_traffic_bench.json)."""
    import hashlib
    from dct_pruning_amd import _lib
    h = hashlib.sha256()
    with open(_lib.LIB_PATH, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def kernel_name(edge, per_tensor):
    """The kernel dcts_energy_f32 / dcts_energy_multi_f32 (AUTO) runs for a square tile edge."""
    if edge in (7, 9):
        return "k_energy_lane_multi<%d>" % edge
    if edge <= 64:
        from dct_pruning_amd import ops
        if not ops.has_codelet(edge, edge):
            return "k_energy_rect (%dx%d)" % (edge, edge)  # no square kernel of its own: the run-time codelet pair
        return ("k_energy_codelet<%d,%d>" if per_tensor else "k_energy_codelet_multi<%d,%d>") % (edge, edge)
    if edge == 224:
        return "k_tile2d (224x224)"
    if edge == 128:
        return "k_split_pipe (%dx%d)" % (edge, edge)
    if edge in (288, 320):
        return "k_split_fused2 (%dx%d)" % (edge, edge)
    if edge in (72, 80, 144, 160):
        return "k_tile2g (%dx%d)" % (edge, edge)
    if edge in (96, 112, 192, 256):
        return "k_split_fused (%dx%d)" % (edge, edge)
    if (edge <= 256 and edge % 4 == 0 and ((edge // 4) % 2 == 0 or edge // 4 <= 32)) or (edge <= 512 and edge % 16 == 0):
        return "k_pass1d x2 (%dx%d, two launches)" % (edge, edge)
    return "k_energy_direct (%dx%d)" % (edge, edge)


def headline(lib, dev, stream_ptr, ws_fn):
    """SURVEY.md §8(d) headline micro-benchmarks: (N*C = 16384, 56x56) and (4096, 224x224);
    buffers rotated so the working set exceeds L2 + Infinity Cache."""
    out = {}
    for name, nmaps, h, nbuf in [("56x56", 16384, 56, 3), ("224x224", 4096, 224, 1), ("28x28", 65536, 28, 3),
                                 ("14x14", 262144, 14, 3), ("7x7", 1048576, 7, 3), ("32x32", 65536, 32, 3),
                                 ("288x288", 2048, 288, 1), ("320x320", 2048, 320, 1), ("144x144", 8192, 144, 1),
                                 ("72x72", 32768, 72, 1),
                                 # round 3: shapes that used to fall to the cosine-matrix kernel - a non-square map and an edge
                                 # without a square kernel (run-time codelet pair, rect.hip), an edge on the two-launch path only
                                 ("56x28", 32768, (56, 28), 3), ("13x13", 262144, 13, 3), ("384x384", 512, 384, 1)]:
        h, w = h if isinstance(h, tuple) else (h, h)
        bufs = [synth(1, nmaps, h, w, 777 + i, dev) for i in range(nbuf)]
        ws = ws_fn(1, nmaps, h, w)
        units = [BoundUnit(lib, b, False, stream_ptr, ws) for b in bufs]
        # >= 20 warm-up + >= 100 timed launches, median and min. The length matters for
        # the large tiles: under sustained load the clock management first drops, then raises the shader
        # clock (224x224, 4096 maps: 225 us -> 300 us after ~10 launches -> 215 us from launch ~90 on,
        # profiles/r02_rep_times_dvfs.txt); ten launches measured the dip
        for i in range(20):
            units[i % nbuf].launch_energy()
        torch.cuda.synchronize(dev)
        reps = 100
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for i in range(reps):
            ev[i][0].record()
            units[i % nbuf].launch_energy()
            ev[i][1].record()
        torch.cuda.synchronize(dev)
        ts = sorted(a.elapsed_time(b) for a, b in ev)
        med = ts[len(ts) // 2]
        by = units[0].bytes
        # the same 100 launches back to back between ONE pair of events: no event packets between the kernels (an event pair
        # around a 40 us kernel adds ~3.5 us to what it measures, profiles/r03_headline56_launch_series.txt), inter-kernel
        # gaps included. Reported beside the per-launch median, which stays the headline figure.
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            units[i % nbuf].launch_energy()
        e1.record()
        torch.cuda.synchronize(dev)
        ser = e0.elapsed_time(e1) / reps
        out[name] = {"maps": nmaps, "median_us": med * 1e3, "min_us": ts[0] * 1e3,
                     "Mmaps_s": nmaps / med / 1e3, "GB_s": by / med / 1e6, "frac": by / med / 1e6 / HBM_PEAK_GBS,
                     "series_us_per_launch": ser * 1e3, "series_frac": by / ser / 1e6 / HBM_PEAK_GBS}
        del units, bufs
        torch.cuda.empty_cache()
    return out


OUTPUT_BUDGET = 64 << 20  # bytes, all files of --dump-outputs together


def write_outputs(d, arrays, budget=OUTPUT_BUDGET):
    """--dump-outputs: each tensor of `arrays` (name -> tensor) as d/<name>.npy in float32. An array that does not fit
    its share of `budget` (smallest arrays first, each gets an equal share of what is left) is replaced by the
    elements of its flattened form at a fixed seeded choice of positions, in ascending order of position."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    left = budget - 128 * len(arrays)  # the .npy header of each file
    names = sorted(arrays, key=lambda k: arrays[k].numel())
    for i, name in enumerate(names):
        t = arrays[name].detach().float()
        k = left // (4 * (len(names) - i))
        if t.numel() > k:
            pick = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:k].sort().values
            t = t.reshape(-1)[pick.to(t.device)]
        a = t.cpu().numpy()
        np.save(os.path.join(d, name + ".npy"), a)
        left -= a.nbytes


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(n):
    """`python bench.py --gpus N` on its own: start the N ranks as a CHILD torch.distributed.run (this
    process has not touched the GPU and never execs), relay the child's output (rank 0 prints the one
    JSON line) and its exit code."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    # before the first HIP call: this pool's driver only supports dmabuf IPC, RCCL fails with hipIpcGetMemHandle otherwise
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    args = parse()
    if args.batch is None:
        args.batch = 12 if args.net == "u2netp" else 256
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        sys.exit("bench.py --gpus %d but WORLD_SIZE=%d: launch with --nproc-per-node %d (or without a launcher)"
                 % (args.gpus, world, args.gpus))
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (no CPU fallback in the product path)")
    # rehearsal mode for a one-GPU box: DCTS_BENCH_REHEARSE=1 puts every rank on cuda:0 and runs the
    # collective over gloo (through host memory); the driver's real runs use one GPU per rank + RCCL
    rehearse = os.environ.get("DCTS_BENCH_REHEARSE") == "1"
    dev = torch.device("cuda", 0 if rehearse else local_rank)
    torch.cuda.set_device(dev)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        from dct_pruning_amd import sharding as _sh
        # bounded bring-up: a rank that cannot reach the others prints {"error": ...} and exits 3 (sharding.py)
        _sh.init_process_group("gloo" if rehearse else "nccl", rank=rank, world_size=world, device=dev, what="bench.py")

    from dct_pruning_amd import _lib, schedules, sharding
    from dct_pruning_amd.ops import _workspace
    lib = _lib.load()
    stream_ptr = torch.cuda.current_stream(dev).cuda_stream

    def ws_fn(n, c, h, w):
        return _workspace(dev, stream_ptr, lib.dcts_workspace_bytes(n, c, h, w))

    if args.input_size is not None and args.net != "u2netp":
        sys.exit("--input-size applies to --net u2netp only")
    points = schedules.SCHEDULES[args.net](args.input_size) if args.input_size else schedules.SCHEDULES[args.net]()
    N = args.batch
    scored = [schedules.scored_shape(p) for p in points]
    chans = [s[1] for s in scored]
    cost_pc = [float(N * (4 * p.H * p.W + 4)) for p in points]
    total_cost = sum(c * k for c, k in zip(chans, cost_pc))
    # whole hook points (layers) are the units; wide layers are only cut into channel ranges when
    # there are too few layers per rank for LPT to balance (49 layers over 8 ranks: 2.3 % imbalance)
    split = (total_cost / (world * 8)) if world * 4 > len(points) else None  # as harness.imp_score's single-sweep modes
    units = sharding.make_units(chans, cost_pc, max_unit_cost=split)
    owner, load = sharding.assign(units, world)
    off, seg = sharding.layout(units, owner, world)

    mine = [i for i in range(len(units)) if owner[i] == rank]
    bound = []
    for i in mine:
        u = units[i]
        p = points[u.layer]
        x = synth(N, u.c_hi - u.c_lo, p.H, p.W, 20260104 + 1000 * CFG_ID + 64 * u.layer + (u.c_lo % 61), dev)
        bound.append((i, BoundUnit(lib, x, scored[u.layer][2], stream_ptr, ws_fn(N, u.c_hi - u.c_lo, p.H, p.W))))
    if args.steps is None:
        args.steps = 20 if total_cost >= 1e9 else 200
    if args.steps < 1 or args.warmup < 0:
        sys.exit("bench.py needs --steps >= 1 and --warmup >= 0")
    maps_per_step = N * sum(chans)
    per_edge = {}
    for p, ch in zip(points, chans):
        per_edge[p.H] = per_edge.get(p.H, 0) + ch
    shape_summary = ", ".join("%dx%d x%d" % (e, e, per_edge[e]) for e in sorted(per_edge, reverse=True))

    # dominant kernel: the one owning the most algorithmic bytes on this rank
    by_edge = {}
    for _, b in bound:
        by_edge[b.h] = by_edge.get(b.h, 0) + b.bytes
    dom_edge = max(by_edge, key=by_edge.get)
    dom = [b for _, b in bound if b.h == dom_edge]

    # launch order inside a step: all energy kernels grouped by tile edge (largest first), then ONE
    # fused running-mean launch for every hook point (dcts_running_mean_update_multi_f32)
    bound.sort(key=lambda ib: (-ib[1].h, ib[0]))
    # one descriptor array per step, built before the clock starts (total_before = samples seen so far): the
    # host side of a step is then two or more ctypes calls and nothing else - for the CIFAR nets a step is
    # ~40 us of GPU work, and a Python loop over the hook points per step made the bench host-bound
    def make_descs(total_before):
        d = (_lib.UpdateDesc * len(bound))()
        for k, (_, b) in enumerate(bound):
            d[k].energy_nc, d[k].feature_result = b.energy.data_ptr(), b.fr.data_ptr()
            d[k].N, d[k].C_count = b.n, b.fr.numel()
            d[k].total_before = float(total_before)
        return d

    descs_by_total = {}
    for s_ in range(max(args.steps, args.warmup)):
        descs_by_total[s_ * N] = make_descs(s_ * N)
    state = {"total": 0}

    # multi-launch plan: all units of one tile shape go into one dcts_energy_multi_f32 call
    by_shape = {}
    for _, b in bound:
        by_shape.setdefault(b.h, []).append(b)
    multi = []
    for h, bs in sorted(by_shape.items(), key=lambda kv: -kv[0]):
        arr = (_lib.TensorItem * len(bs))()
        for i, b in enumerate(bs):
            arr[i].x, arr[i].out_nc = b.x.data_ptr(), b.energy.data_ptr()
            arr[i].N, arr[i].C_total = b.x.shape[0], b.x.shape[1]
            arr[i].strideN, arr[i].strideC = b.x.stride(0), b.x.stride(1)
            arr[i].c_begin, arr[i].c_count = 0, b.x.shape[1]
        ws = ws_fn(max(b.x.shape[0] for b in bs), max(b.x.shape[1] for b in bs), h, h)
        multi.append((h, arr, len(bs), ws))

    # CIFAR-sized nets: every hooked tensor (tile edges 2..32, whatever the shape) in ONE launch per 48 tensors
    # (dcts_energy_mixed_f32) instead of one per tile shape
    mixed = None
    if not args.per_tensor and bound and all(b.h in (2, 4, 8, 16, 32) and b.x.shape[2] == b.x.shape[3] for _, b in bound):
        marr = (_lib.ShapedItem * len(bound))()
        for i, (_, b) in enumerate(bound):
            t = marr[i].t
            t.x, t.out_nc = b.x.data_ptr(), b.energy.data_ptr()
            t.N, t.C_total = b.x.shape[0], b.x.shape[1]
            t.strideN, t.strideC = b.x.stride(0), b.x.stride(1)
            t.c_begin, t.c_count = 0, b.x.shape[1]
            marr[i].H, marr[i].W, marr[i].pad_front_if_odd = b.h, b.h, 0
        mixed = (marr, len(bound))
        dom = [b for _, b in bound]  # one kernel covers every tensor: it is the dominant one

    # timing events (--full only) are created before the clock starts (creating one costs more host time than recording it)
    ev_pool = [torch.cuda.Event(enable_timing=True) for _ in range(2 * args.steps * (len(bound) + 2))] if args.full else []

    def new_event():
        return ev_pool.pop()

    def step(events=None):
        if mixed is not None:
            if events is not None:
                ev = new_event()
                ev.record()
                events.append(ev)
            rc = lib.dcts_energy_mixed_f32(mixed[0], mixed[1], None, 0, stream_ptr)
            if rc:
                raise RuntimeError("dcts_energy_mixed_f32 -> %d" % rc)
            if events is not None:
                ev = new_event()
                ev.record()
                events.append(ev)
        elif args.per_tensor:
            in_dom = False
            for _, b in bound:
                if events is not None and (b.h == dom_edge) != in_dom:
                    ev = new_event()
                    ev.record()
                    events.append(ev)
                    in_dom = not in_dom
                b.launch_energy()
            if events is not None and in_dom:
                ev = new_event()
                ev.record()
                events.append(ev)
        else:
            for h, arr, n, ws in multi:
                timed = events is not None and h == dom_edge
                if timed:
                    ev = new_event()
                    ev.record()
                    events.append(ev)
                rc = lib.dcts_energy_multi_f32(arr, n, h, h, 0, ws.data_ptr(), ws.numel(), stream_ptr)
                if rc:
                    raise RuntimeError("dcts_energy_multi_f32 -> %d" % rc)
                if timed:
                    ev = new_event()
                    ev.record()
                    events.append(ev)
        descs = descs_by_total[state["total"]]
        state["total"] += N
        rc = lib.dcts_running_mean_update_multi_f32(descs, len(bound), stream_ptr)
        if rc:
            raise RuntimeError("dcts_running_mean_update_multi_f32 -> %d" % rc)

    def gather():
        flat = torch.zeros(seg, dtype=torch.float32, device=dev)
        for i, b in bound:
            flat[off[i]:off[i] + b.fr.numel()] = b.fr
        if rehearse and world > 1:
            return sharding.all_gather_scores(flat.cpu(), world).to(dev)
        return sharding.all_gather_scores(flat, world)

    def barrier():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    if args.pmc_calib:
        cal = torch.ones(1 << 28, device=dev)
        sink = torch.zeros(4, device=dev)
        for _ in range(3):
            _lib.check(lib.dcts_debug_stream_read_f32(cal.data_ptr(), cal.numel(), sink.data_ptr(), stream_ptr))
        torch.cuda.synchronize(dev)
        del cal
    for _ in range(args.warmup):
        step()
    if world > 1:
        gather()
    for _, b in bound:
        b.fr.zero_()
    state["total"] = 0

    events = []
    barrier()
    t0 = time.perf_counter()
    # --full: the dominant kernel is timed with HIP events inside the timed region; when a step is tens of
    # microseconds the event packets themselves open gaps between the launches, so only every 8th step is timed
    ev_stride = 1 if total_cost >= 1e9 else 8
    for i_ in range(args.steps):
        step(events if args.full and i_ % ev_stride == 0 else None)
    t_enqueued = time.perf_counter() - t0  # host time to enqueue the K steps (a run is host-bound if this is ~ dt)
    gathered = gather()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if rehearse else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()

    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives: the score vector of every hook point (all ranks' shares,
        # gathered) and the per-map energies of the last step (this rank's tensors, in unit order)
        scores = torch.cat(sharding.unpack(gathered, units, owner, off, chans))
        energy = torch.cat([b.energy for _, b in sorted(bound, key=lambda ib: ib[0])], dim=1)
        write_outputs(args.dump_outputs, {"scores": scores, "energy": energy})

    full = {}
    if args.full:
        # sanity on the result the timed region produced: Parseval against the inputs (device-side),
        # and the dead channels of the synthetic tensors (c % 8 == 5) must come out as exactly +0.0
        i0, b0 = bound[0]
        ref = (b0.x.double() ** 2).sum(dim=(-2, -1)).mean(0)
        got = gathered[rank, off[i0]:off[i0] + b0.fr.numel()].double()
        rel = ((got - ref).abs() / ref.clamp_min(1e-30))[ref > 0].max().item()
        if not rel <= 1e-4:
            sys.exit("bench sanity check failed: rel err %g" % rel)
        dead_bad = 0
        for i, b in bound:
            fr = gathered[rank, off[i]:off[i] + b.fr.numel()]
            dead = (b.x[0].reshape(b.x.shape[1], -1).abs().amax(dim=1) == 0) & (b.x.abs().amax(dim=(0, 2, 3)) == 0)
            dead_bad += int(((fr[dead] != 0) | torch.signbit(fr[dead])).sum().item())
        if dead_bad:
            sys.exit("bench sanity check failed: %d dead channels are not exactly +0.0" % dead_bad)

        # the collective on its own (reported separately), outside the timed region
        if world > 1:
            barrier()
            tg = time.perf_counter()
            gather()
            barrier()
            full["all_gather_ms"] = (time.perf_counter() - tg) * 1e3  # flat buffer fill + one all_gather_into_tensor + barriers

        # events come in (start, stop) pairs around each contiguous group of dominant-kernel launches
        dom_ms = sum(events[i].elapsed_time(events[i + 1]) for i in range(0, len(events), 2))
        timed_steps = len(range(0, args.steps, ev_stride))
        dom_bytes = sum(b.bytes for b in dom) * timed_steps
        n_launch = max((len(dom) if args.per_tensor else -(-len(dom) // (48 if mixed is not None else 32))) * timed_steps, 1)

        achieved = dom_bytes / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
        # HBM bytes per launch of the dominant kernel from the committed PMC passes of THIS bench at THIS launch
        # size (tools/profile_bench_pmc.sh: FETCH_SIZE and WRITE_SIZE in separate rocprofv3 runs, the read side
        # corrected by the known-size calibration read of the same run); null when the record is for another
        # workload / launch size
        traffic = None
        traffic_note = "no PMC record (profiles/pmc_traffic_bench.json)"
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic_bench.json")
        alg_per_launch = dom_bytes / n_launch
        if rank == 0 and os.path.isfile(tpath):
            try:
                # the record is only valid for the binary it was measured on: it carries the SHA-256 of libdctscore.so
                # (the build is reproducible: the same sources give the same bytes on any box of this image)
                stamp = json.load(open(tpath)).get("libdctscore_sha256")
                mine = lib_sha256()
                if stamp != mine:
                    raise ValueError("PMC record is for another build of libdctscore.so (%s..., this one %s...)"
                                     % (str(stamp)[:12], mine[:12]))
                want = ("k_energy_codelet_mixed" if mixed is not None else kernel_name(dom_edge, args.per_tensor)).split(" ")[0].split("<")[0]
                for kname, rec in json.load(open(tpath)).get("kernels", {}).items():
                    if kname.split("<")[0] == want and rec.get("alg_bytes_per_launch") and \
                            abs(rec["alg_bytes_per_launch"] - alg_per_launch) <= 0.01 * alg_per_launch:
                        if mixed is not None or ("<%d, %d" % (dom_edge, dom_edge)) in kname or "tile2d" in kname or "split" in kname:
                            traffic = rec["hbm_bytes_per_launch"]
                            traffic_note = "PMC passes of this bench at this launch size on this binary (sha256 %s...)" % mine[:12]
                if traffic is None:
                    traffic_note = "PMC record is for another workload or launch size"
            except Exception as exc:
                traffic = None
                traffic_note = str(exc)
        full["roofline"] = {"bound": "hbm",
                            "kernel": "k_energy_codelet_mixed (edges 2..32)" if mixed is not None else kernel_name(dom_edge, args.per_tensor),
                            "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_note,
                            "launches": n_launch, "timed_steps": timed_steps, "avg_launch_us": dom_ms / n_launch * 1e3,
                            "alg_bytes_per_launch": dom_bytes / n_launch}
        full["parity_check_rel_err"], full["dead_channels_not_plus_zero"] = rel, dead_bad

    if rank == 0:
        res = {
            "metric": "feature-map DCT+score throughput", "value": maps_per_step * args.steps / dt / 1e6,
            "unit": "Mmaps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s hooked feature maps (%d tensors, %d maps/sample: %s), batch %d, limit=steps"
                                   % (args.net, len(points), sum(chans), shape_summary, N),
                       "global_batch": N, "sharding": "layer-sharded (LPT on bytes), 1 all-gather" if world > 1 else "none",
                       "launch_mode": "per-tensor" if args.per_tensor else ("one launch for all tile shapes" if mixed is not None
                                                                               else "one launch per tile shape"),
                       "units_rank0": len(bound), "load_imbalance": (max(load) / (sum(load) / world)) if world > 1 else 1.0},
            "GB_s_whole_step": total_cost * args.steps / dt / 1e9,
            "host_enqueue_ms_per_step": t_enqueued / args.steps * 1e3,
        }
        res.update(full)
        if args.full and not args.no_headline and world == 1:
            res["headline"] = headline(lib, dev, stream_ptr, ws_fn)
        if args.full and not args.no_cpu_baseline and world == 1:
            res["cpu_baseline"] = cpu_baseline(points, args.cpu_seconds)
        print(json.dumps(res))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
