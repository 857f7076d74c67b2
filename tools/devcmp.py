#!/usr/bin/env python3
"""Two builds of libdctscore.so on the same seeded inputs: are the outputs bit-identical? tools/devcmp.py <a.so> <b.so>

Every entry point whose kernels run the two-pass codelet schedule, at the smallest shapes at which its shared pieces can go
wrong: edges 2, 7, 14, 20, 28, 56, 64 (G = 32, 9, 4, 3, 2, 1, 1 maps per wave, both special LDS strides, idle lanes) with
3 * G + 1 maps (a ragged last group: tail lanes load the stand-in map); bands and entropy also at 13, 27, 55 with the odd
front pad; bands with K = 1, 3, 8; channels_last with N = 2 and channels 2 ... 38 of 41 at every native edge (ragged in the
64-lane run and in every channel block).

The single-launch role-wave kernels (fused, two-roles, pipelined; the phases they share are in split_common.hpp), by
explicit family: every path of FusedCfg and Fused2Cfg (LARGE below) with 1, 2 and 3 * CUs * B + 2 maps - a workgroup that
never reaches the next-map prefetch, and every workgroup with at least three maps (both buffer parities, the deferred sum
across two maps, the epilogue), B an upper bound on workgroups per CU; a base that is only 4-byte aligned; coefficients
through a workspace of two tiles (the leaf chunks and k_assemble loop); dcts_energy_multi_f32 over three tensors (the
tile_in / tile_out hints across tensors). Exit status 1 if any comparison differs."""
import ctypes
import itertools
import sys

import torch

I64, I32, VP, SZ = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t
F32, F16, BF16 = 0, 1, 2
TORCH_DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
EDGES = (2, 7, 14, 20, 28, 56, 64)
ODD_EDGES = (13, 27, 55)
NHWC_EDGES = (2, 4, 7, 8, 14, 16, 28, 32, 56)
NCHW = [VP] + [I64] * 8 + [I32] * 3  # x, N, C_total, H, W, four strides, c_begin, c_count, pad_front_if_odd
ALGO_AUTO, ALGO_FUSED, ALGO_PIPE = 0, 5, 6
# (family, edge, waves per workgroup): FusedCfg's unbalanced rounds at L = 3 and 4 (72, 160) and rounds of 3 + 3 + 2 roles (144),
# the balanced dump at L = 3 and 4 (96, 256), 224 (excluded from it); Fused2Cfg's deferred sum (288) and 48-column rounds
# with the immediate sum (320); the pipelined kernel's two edges
LARGE = [(ALGO_FUSED, 72, 8), (ALGO_FUSED, 160, 16), (ALGO_FUSED, 144, 8), (ALGO_FUSED, 96, 8), (ALGO_FUSED, 256, 16),
         (ALGO_FUSED, 224, 16), (ALGO_FUSED, 288, 8), (ALGO_FUSED, 320, 8), (ALGO_PIPE, 128, 8), (ALGO_PIPE, 224, 16)]
FUSED2_EDGES = (288, 320)  # their launcher states one workgroup per CU


class TensorItem(ctypes.Structure):  # dcts_tensor_item
    _fields_ = [("x", VP), ("out_nc", VP), ("N", I64), ("C_total", I64), ("strideN", I64), ("strideC", I64),
                ("c_begin", I32), ("c_count", I32)]


def load(path):
    lib = ctypes.CDLL(path)
    lib.dcts_energy_f32_ex.argtypes = NCHW + [VP, VP, SZ, VP, I32]
    lib.dcts_dct2d_f32_ex.argtypes = NCHW + [VP, VP, SZ, VP, I32]
    lib.dcts_energy_multi_f32.argtypes = [ctypes.POINTER(TensorItem), I32, I64, I64, I32, VP, SZ, VP]
    lib.dcts_band_energy_f32.argtypes = NCHW + [VP, I32, VP, VP, SZ, VP, I32]
    lib.dcts_spectral_entropy_f32.argtypes = NCHW + [VP, VP, SZ, VP, I32]
    lib.dcts_energy_typed.argtypes = [VP, I32] + NCHW[1:] + [VP, VP, SZ, VP]
    lib.dcts_energy_nhwc.argtypes = [VP, I32] + [I64] * 7 + [I32] * 2 + [VP, VP, SZ, VP]
    for name, args in (("dcts_workspace_bytes", [I64] * 4), ("dcts_band_workspace_bytes", [I64] * 4 + [I32]),
                       ("dcts_entropy_workspace_bytes", [I64] * 4), ("dcts_typed_workspace_bytes", [I32] + [I64] * 4),
                       ("dcts_nhwc_workspace_bytes", [I32] + [I64] * 4)):
        getattr(lib, name).restype = SZ
        getattr(lib, name).argtypes = args
    return lib


def maps(edge, nmaps, dt=F32):
    return torch.relu(torch.randn(1, nmaps, edge, edge, device="cuda")).to(TORCH_DT[dt])


def run(lib, need, out_shape, call):
    out = torch.full(out_shape, float("nan"), device="cuda")
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    rc = call(out.data_ptr(), ws.data_ptr(), ws.numel())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def energy(lib, x, pad, dt, algo=ALGO_AUTO):
    _, c, h, w = x.shape
    if dt == F32:
        return run(lib, lib.dcts_workspace_bytes(1, c, h, w), (1, c), lambda o, ws, n: lib.dcts_energy_f32_ex(
            x.data_ptr(), 1, c, h, w, *x.stride(), 0, c, pad, o, ws, n, None, algo))
    return run(lib, lib.dcts_typed_workspace_bytes(dt, 1, c, h, w), (1, c), lambda o, ws, n: lib.dcts_energy_typed(
        x.data_ptr(), dt, 1, c, h, w, *x.stride(), 0, c, pad, o, ws, n, None))


def coeff(lib, x, algo, ws_tiles):
    _, c, h, w = x.shape
    return run(lib, ws_tiles * h * w * 4, (1, c, h, w), lambda o, ws, n: lib.dcts_dct2d_f32_ex(
        x.data_ptr(), 1, c, h, w, *x.stride(), 0, c, 0, o, ws, n, None, algo))


def energy_multi(lib, xs):
    edge = xs[0].shape[-1]
    out = torch.full((sum(x.shape[1] for x in xs),), float("nan"), device="cuda")
    items, first = (TensorItem * len(xs))(), 0
    for it, x in zip(items, xs):
        c = x.shape[1]
        it.x, it.out_nc, it.N, it.C_total, it.strideN, it.strideC = x.data_ptr(), out[first:].data_ptr(), 1, c, x.stride(0), x.stride(1)
        it.c_begin, it.c_count = 0, c
        first += c
    need = max(lib.dcts_workspace_bytes(1, x.shape[1], edge, edge) for x in xs)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    rc = lib.dcts_energy_multi_f32(items, len(xs), edge, edge, 0, ws.data_ptr(), ws.numel(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def bands(lib, x, pad, weights):
    _, c, h, w = x.shape
    k = weights.shape[0]
    return run(lib, lib.dcts_band_workspace_bytes(1, c, h, w, k), (1, c, k), lambda o, ws, n: lib.dcts_band_energy_f32(
        x.data_ptr(), 1, c, h, w, *x.stride(), 0, c, pad, weights.data_ptr(), k, o, ws, n, None, 0))


def entropy(lib, x, pad):
    _, c, h, w = x.shape
    return run(lib, lib.dcts_entropy_workspace_bytes(1, c, h, w), (1, c), lambda o, ws, n: lib.dcts_spectral_entropy_f32(
        x.data_ptr(), 1, c, h, w, *x.stride(), 0, c, pad, o, ws, n, None, 0))


def nhwc(lib, x, dt, c_begin, c_count):
    n, c, h, w = x.shape  # channels_last memory: strides (H * W * C, 1, W * C, C)
    sn, _, sh, sw = x.stride()
    return run(lib, lib.dcts_nhwc_workspace_bytes(dt, n, c_count, h, w), (n, c_count), lambda o, ws, nb: lib.dcts_energy_nhwc(
        x.data_ptr(), dt, n, c, h, w, sn, sh, sw, c_begin, c_count, o, ws, nb, None))


def cases():
    for edge, pad in [(e, 0) for e in EDGES] + [(e, 1) for e in ODD_EDGES]:
        nmaps = 3 * (64 // (edge + pad)) + 1
        x = maps(edge, nmaps)
        yield "energy f32 %d x %d pad %d, %d maps" % (edge, edge, pad, nmaps), lambda lib: energy(lib, x, pad, F32)
        yield "entropy %d x %d pad %d, %d maps" % (edge, edge, pad, nmaps), lambda lib: entropy(lib, x, pad)
        for k in (1, 3, 8):
            wt = torch.rand(k, edge + pad, edge + pad, device="cuda")
            yield "bands K=%d %d x %d pad %d, %d maps" % (k, edge, edge, pad, nmaps), lambda lib: bands(lib, x, pad, wt)
    for dt, name in ((F16, "f16"), (BF16, "bf16")):
        for edge in EDGES:
            nmaps = 3 * (64 // edge) + 1
            xh = maps(edge, nmaps, dt)
            yield "energy %s %d x %d, %d maps" % (name, edge, edge, nmaps), lambda lib: energy(lib, xh, 0, dt)
    for dt, name in ((F32, "f32"), (F16, "f16"), (BF16, "bf16")):
        for edge in NHWC_EDGES:
            xc = torch.relu(torch.randn(2, 41, edge, edge, device="cuda")).to(TORCH_DT[dt]).contiguous(memory_format=torch.channels_last)
            yield "nhwc %s %d x %d, N=2, channels 2..38 of 41" % (name, edge, edge), lambda lib: nhwc(lib, xc, dt, 2, 37)


def large_cases():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for algo, edge, waves in LARGE:
        name = "pipe" if algo == ALGO_PIPE else "fused"
        per_cu = 1 if edge in FUSED2_EDGES else 32 // waves
        for nmaps in (1, 2, 3 * cus * per_cu + 2):
            x = maps(edge, nmaps)
            yield "%s %d x %d, %d maps" % (name, edge, edge, nmaps), lambda lib: energy(lib, x, 0, F32, algo)
    for edge in (96, 288):  # the fused families load dwords into registers: any 4-byte-aligned base (pipe: 16 bytes)
        flat = torch.relu(torch.randn(5 * edge * edge + 1, device="cuda"))
        xo = flat[1:].view(1, 5, edge, edge)
        yield "fused %d x %d, base + 4 bytes, 5 maps" % (edge, edge), lambda lib: energy(lib, xo, 0, F32, ALGO_FUSED)
    for edge in (72, 96, 288):
        x5 = maps(edge, 5)
        yield "fused coefficients %d x %d, 5 maps, 2 tiles" % (edge, edge), lambda lib: coeff(lib, x5, ALGO_FUSED, 2)
    for edge in (96, 288):
        xs = [maps(edge, n) for n in (1, 7, 40)]
        yield "multi %d x %d, tensors of 1, 7, 40 maps" % (edge, edge), lambda lib: energy_multi(lib, xs)


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    torch.manual_seed(0)
    differ = 0
    for what, f in itertools.chain(cases(), large_cases()):
        ra, rb = f(a), f(b)
        same = torch.equal(ra.view(torch.int32), rb.view(torch.int32)) and not torch.isnan(ra).any().item()
        differ += not same
        print("%-48s bit-identical %s" % (what, same), flush=True)
    print("%d comparisons differ" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
