#!/usr/bin/env python3
"""Two builds of libdctscore.so on the same seeded inputs: are the outputs bit-identical? tools/devcmp.py <a.so> <b.so>

Every entry point whose kernels run the two-pass codelet schedule, at the smallest shapes at which its shared pieces can go
wrong: edges 2, 7, 14, 20, 28, 56, 64 (G = 32, 9, 4, 3, 2, 1, 1 maps per wave, both special LDS strides, idle lanes) with
3 * G + 1 maps (a ragged last group: tail lanes load the stand-in map); bands and entropy also at 13, 27, 55 with the odd
front pad; bands with K = 1, 3, 8; channels_last with N = 2 and channels 2 ... 38 of 41 at every native edge (ragged in the
64-lane run and in every channel block). Exit status 1 if any comparison differs."""
import ctypes
import sys

import torch

I64, I32, VP, SZ = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t
F32, F16, BF16 = 0, 1, 2
TORCH_DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
EDGES = (2, 7, 14, 20, 28, 56, 64)
ODD_EDGES = (13, 27, 55)
NHWC_EDGES = (2, 4, 7, 8, 14, 16, 28, 32, 56)
NCHW = [VP] + [I64] * 8 + [I32] * 3  # x, N, C_total, H, W, four strides, c_begin, c_count, pad_front_if_odd


def load(path):
    lib = ctypes.CDLL(path)
    lib.dcts_energy_f32_ex.argtypes = NCHW + [VP, VP, SZ, VP, I32]
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


def energy(lib, x, pad, dt):
    _, c, h, w = x.shape
    if dt == F32:
        return run(lib, lib.dcts_workspace_bytes(1, c, h, w), (1, c), lambda o, ws, n: lib.dcts_energy_f32_ex(
            x.data_ptr(), 1, c, h, w, *x.stride(), 0, c, pad, o, ws, n, None, 0))
    return run(lib, lib.dcts_typed_workspace_bytes(dt, 1, c, h, w), (1, c), lambda o, ws, n: lib.dcts_energy_typed(
        x.data_ptr(), dt, 1, c, h, w, *x.stride(), 0, c, pad, o, ws, n, None))


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


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    torch.manual_seed(0)
    differ = 0
    for what, f in cases():
        ra, rb = f(a), f(b)
        same = torch.equal(ra.view(torch.int32), rb.view(torch.int32)) and not torch.isnan(ra).any().item()
        differ += not same
        print("%-48s bit-identical %s" % (what, same))
    print("%d comparisons differ" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
