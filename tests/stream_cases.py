"""The case table of tests/test_streams_gpu.py: one case per launch site of libdctscore, at the smallest shape that reaches it
(N = 2, five channels: a ragged count wherever a kernel works in groups), every call through ctypes with an explicit stream.

A Case names the entry point, the route inside it and the .hip units its launches live in; build() allocates every buffer of
the call on the device and returns a Run:

  xs      the input buffers the test's producer writes (device), fresh[v] what it writes into them for input variant v (three
          variants: the eager protocol uses the first, capture and replay the other two);
  outs    the output buffers (float32), ws the workspace (uint8) or None;
  call    call(stream) -> return code of the entry point, made on that hipStream_t;
  check   check(v, outs on the CPU): the float64 oracle the family's own GPU test uses, at that test's tolerance;
  inout   the outputs are read before they are written (the running means): reset() puts their start values back and the
          sentinel checks do not apply.

No case reads anything but this directory's oracles, and nothing here touches the GPU until build() is called."""

import numpy as np
import torch

import band_oracle as bo
import dct_probes as dp
import entropy_oracle as eo
import gm_metric_oracle as mo
import gm_oracle as go
import gm_pairs_oracle as po
import lowpass_oracle as lo
import rank_oracle as ro
from dct_pruning_amd import _lib, ops
from dct_pruning_amd.accumulate import HostAccumulator
from helpers import synth
from oracle import dct_oracle as orc

DEV = "cuda"
VARIANTS = 3
SENTINEL = -12345.0
N, C = 2, 5
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPE_CODE = {F32: 0, F16: 1, BF16: 2}  # DCTS_DTYPE_*


class Run:
    def __init__(self, xs, fresh, outs, ws, call, check, inout=False, reset=None, keep=()):
        self.xs, self.fresh, self.outs, self.ws, self.call, self.check = xs, fresh, outs, ws, call, check
        self.inout, self.reset, self.keep = inout, reset, keep

    def reset_outs(self):
        if self.reset is not None:
            self.reset()
        else:
            for o in self.outs:
                o.fill_(SENTINEL)


class Case:
    def __init__(self, name, entry, units, build, capture=False, reuse_tables=False):
        self.name, self.entry, self.units, self.build = name, entry, tuple(units.split()), build
        self.capture = capture            # one of the representatives of layer 3 (one per .hip unit)
        self.reuse_tables = reuse_tables  # direct family: the basis tables are built on the side stream BEFORE the case runs

    def __repr__(self):
        return self.name


def _maps(shape, seed, dtype=F32, dead=True):
    """[variants of a CPU tensor]: the suite's synthetic maps, rounded to dtype."""
    return [synth(*shape, seed=seed + 1000 * v, dead=dead).to(dtype) for v in range(VARIANTS)]


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16) + 256, dtype=torch.uint8, device=DEV)


def _dev(ts):
    return [t.to(DEV) for t in ts]


def _strides(x):
    return x.stride(0), x.stride(1), x.stride(2), x.stride(3)


# ---- oracles, each as its family's GPU test applies it ------------------------------------------------------------------
def _check_energy(x, got, pad=False):
    """test_gpu_probes.py / test_half_gpu.py / test_nhwc_gpu.py: sum(x^2) in float64, 8 x the fp32 reference's own error."""
    x = x.float()
    dp.check_energy(lambda _: got, x, dp.tolerance(dp.reference_error(x, pad_front_if_odd=pad)))


def _check_coeff(x, got):
    """test_gpu_coeff_large.py: 2e-6 of the coefficient scale."""
    ref = orc.dct_2d_f64(x.numpy())
    assert got.shape == ref.shape
    assert np.abs(got.numpy() - ref).max() <= 2e-6 * np.abs(ref).max()


def _rel(got, ref):
    got, ref = got.double(), ref.double()
    return ((got - ref).abs() / ref.abs().clamp_min(1e-30))[ref != 0].max().item()


# ---- builders ---------------------------------------------------------------------------------------------------------
def _single(entry, h, w, algo=None, pad=0, store=False, seed=1, shape_nc=(N, C)):
    """dcts_energy_f32[_ex] / dcts_dct2d_f32[_ex] on one dense tensor."""
    def build():
        lib = _lib.load()
        n, c = shape_nc
        cpu = _maps((n, c, h, w), seed)
        x = torch.empty_like(cpu[0], device=DEV)
        p = 1 if (pad and h % 2) else 0
        out = torch.empty((n, c, h + p, w + p) if store else (n, c), dtype=F32, device=DEV)
        ws = _ws(lib.dcts_workspace_bytes(n, c, h, w) + (n * c * (h + p) * (w + p) * 4 if store else 0))
        args = (x.data_ptr(), n, c, h, w) + _strides(x) + (0, c, pad, out.data_ptr(), ws.data_ptr(), ws.numel() - 256)
        fn = getattr(lib, entry)

        def call(stream):
            return fn(*args, stream) if algo is None else fn(*args, stream, algo)

        def check(v, outs):
            (_check_coeff if store else lambda a, b: _check_energy(a, b, bool(pad)))(cpu[v], outs[0])
        return Run([x], [_dev([t]) for t in cpu], [out], ws, call, check)
    return build


def _weighted(h):
    def build():
        lib = _lib.load()
        cpu = _maps((N, C, h, h), 40 + h, dead=False)
        wt = torch.rand(h, h, generator=torch.Generator().manual_seed(41 + h))
        x, wd = torch.empty_like(cpu[0], device=DEV), wt.to(DEV)
        out = torch.empty((N, C), dtype=F32, device=DEV)
        ws = _ws(lib.dcts_weighted_workspace_bytes(N, C, h, h))
        args = (x.data_ptr(), N, C, h, h) + _strides(x) + (0, C, 0, wd.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() - 256)

        def check(v, outs):  # test_gpu_parity.py: 2e-5 relative
            assert _rel(outs[0], torch.from_numpy(orc.weighted_energy_nc_f64(cpu[v], wt.numpy()))) <= 2e-5
        return Run([x], [_dev([t]) for t in cpu], [out], ws, lambda s: lib.dcts_weighted_energy_f32(*args, s), check, keep=(wd,))
    return build


def _band(h, K):
    def build():
        lib = _lib.load()
        cpu = _maps((N, C, h, h), 50 + h)
        wt = torch.rand(K, h, h, generator=torch.Generator().manual_seed(51 + h)) * 2.0
        x, wd = torch.empty_like(cpu[0], device=DEV), wt.to(DEV)
        out = torch.empty((N, C, K), dtype=F32, device=DEV)
        ws = _ws(lib.dcts_band_workspace_bytes(N, C, h, h, K))
        args = (x.data_ptr(), N, C, h, h) + _strides(x) + (0, C, 0, wd.data_ptr(), K, out.data_ptr(), ws.data_ptr(), ws.numel() - 256)

        def check(v, outs):  # test_bands_gpu.py: 8 x the fp32 restatement's own error, of the map's energy
            tol = dp.tolerance(bo.band_error(bo.band_energy_nc_f32(cpu[v], wt), cpu[v], wt))
            assert bo.band_error(outs[0], cpu[v], wt) <= tol
        return Run([x], [_dev([t]) for t in cpu], [out], ws, lambda s: lib.dcts_band_energy_f32(*args, s, ops.ALGO_AUTO), check, keep=(wd,))
    return build


def _entropy(h):
    def build():
        lib = _lib.load()
        cpu = _maps((N, C, h, h), 60 + h)
        x = torch.empty_like(cpu[0], device=DEV)
        out = torch.empty((N, C), dtype=F32, device=DEV)
        ws = _ws(lib.dcts_entropy_workspace_bytes(N, C, h, h))
        args = (x.data_ptr(), N, C, h, h) + _strides(x) + (0, C, 0, out.data_ptr(), ws.data_ptr(), ws.numel() - 256)

        def check(v, outs):  # test_entropy_gpu.py
            assert np.abs(outs[0].numpy().astype(np.float64) - eo.entropy_nc_f64(cpu[v])).max() <= eo.TOL
        return Run([x], [_dev([t]) for t in cpu], [out], ws, lambda s: lib.dcts_spectral_entropy_f32(*args, s, ops.ALGO_AUTO), check)
    return build


def _lowpass(h, w, K, drop_dc=False):
    def build():
        lib = _lib.load()
        cpu = _maps((N, C, h, w), 70 + h + w)
        x = torch.empty_like(cpu[0], device=DEV)
        out = torch.empty((N, C, min(K, h), min(K, w)), dtype=F32, device=DEV)
        ws = _ws(lib.dcts_dct2d_lowpass_workspace_bytes(N, C, h, w, K))
        args = (x.data_ptr(), N, C, h, w) + _strides(x) + (0, C, K, 1 if drop_dc else 0, out.data_ptr(), ws.data_ptr(), ws.numel() - 256)

        def check(v, outs):  # test_lowpass_gpu.py
            ref = lo.lowpass_f64(cpu[v], K, drop_dc=drop_dc)
            assert outs[0].shape == ref.shape
            assert np.abs(outs[0].numpy() - ref).max() / lo.coefficient_scale(cpu[v]) <= lo.SIG_TOL
        return Run([x], [_dev([t]) for t in cpu], [out], ws, lambda s: lib.dcts_dct2d_lowpass_f32(*args, s), check)
    return build


def _rank(h):
    def build():
        lib = _lib.load()
        cpu = _maps((N, C, h, h), 80 + h)
        x = torch.empty_like(cpu[0], device=DEV)
        out = torch.empty((N, C), dtype=F32, device=DEV)
        args = (x.data_ptr(), N, C, h, h) + _strides(x) + (0, C, out.data_ptr())

        def check(v, outs):  # test_rank_gpu.py: the oracle's integers wherever the threshold decides
            ok = ~ro.undecidable(cpu[v])
            assert ok.float().mean().item() > 0.99 and torch.equal(outs[0][ok], ro.rank_nc(cpu[v])[ok])
        return Run([x], [_dev([t]) for t in cpu], [out], None, lambda s: lib.dcts_rank_f32(*args, s), check)
    return build


def _gm(metric, pairs=False, via_metric=True, shape=(N, 12, 7, 7)):
    """dcts_gm_distance_f32 (via_metric False), dcts_gm_distance_metric_f32, dcts_gm_pairs_f32."""
    def build():
        lib = _lib.load()
        n, c = shape[:2]
        cpu = _maps(shape, 90 + shape[0], dead=True)
        x = torch.empty_like(cpu[0], device=DEV)
        out = torch.empty((c, c) if pairs else (n, c), dtype=F32, device=DEV)
        code = ops.GM_METRICS[metric]
        if pairs:
            assert lib.dcts_gm_pairs_slices(n, c) > 1  # the summing kernel runs
        ws = _ws(lib.dcts_gm_pairs_workspace_bytes(code, n, c, c) if pairs else lib.dcts_gm_workspace_bytes(code, n, c, c))
        args = (x.data_ptr(), n, c) + tuple(shape[2:]) + _strides(x) + (0, c, 0, c, out.data_ptr())
        if pairs:
            call = lambda s: lib.dcts_gm_pairs_f32(*args, s, code, ws.data_ptr(), ws.numel() - 256)  # noqa: E731
        elif via_metric:
            call = lambda s: lib.dcts_gm_distance_metric_f32(*args, s, code, ws.data_ptr(), ws.numel() - 256)  # noqa: E731
        else:
            call = lambda s: lib.dcts_gm_distance_f32(*args, s)  # noqa: E731

        def check(v, outs):
            g = outs[0].numpy()
            if pairs:  # test_gm_pairs_gpu.py
                zeros = po.exact_zeros(cpu[v], metric)
                assert po.error(g, po.pair_matrix_f64(cpu[v], metric), metric, n, zeros) <= po.TOL[metric]
                assert (g[zeros].view(np.int32) == 0).all()
            elif metric == "l2":  # test_gm_gpu.py
                ref = go.gm_nc_f64(cpu[v])
                assert go.relative_error(g, ref) <= go.TOL and (g[ref == 0].view(np.int32) == 0).all()
            else:  # test_gm_metric_gpu.py
                ref = mo.gm_metric_nc_f64(cpu[v], metric)
                assert mo.error_per_reference(g, ref, c) <= mo.TOL[metric] and (g[ref == 0].view(np.int32) == 0).all()
        return Run([x], [_dev([t]) for t in cpu], [out], ws, call, check)
    return build


def _typed(dtype, h):
    def build():
        lib = _lib.load()
        cpu = _maps((N, C, h, h), 110 + h, dtype)
        x = torch.empty_like(cpu[0], device=DEV)
        out = torch.empty((N, C), dtype=F32, device=DEV)
        ws = _ws(lib.dcts_typed_workspace_bytes(DTYPE_CODE[dtype], N, C, h, h))
        args = (x.data_ptr(), DTYPE_CODE[dtype], N, C, h, h) + _strides(x) + (0, C, 0, out.data_ptr(), ws.data_ptr(), ws.numel() - 256)
        return Run([x], [_dev([t]) for t in cpu], [out], ws, lambda s: lib.dcts_energy_typed(*args, s),
                   lambda v, outs: _check_energy(cpu[v], outs[0]))
    return build


def _nhwc(dtype, h):
    def build():
        lib = _lib.load()
        cpu = _maps((N, C, h, h), 120 + h, dtype)
        x = torch.empty((N, C, h, h), dtype=dtype, device=DEV).contiguous(memory_format=torch.channels_last)
        out = torch.empty((N, C), dtype=F32, device=DEV)
        args = (x.data_ptr(), DTYPE_CODE[dtype], N, C, h, h, x.stride(0), x.stride(2), x.stride(3), 0, C, out.data_ptr(), None, 0)
        assert x.stride(1) == 1
        return Run([x], [_dev([t]) for t in cpu], [out], None, lambda s: lib.dcts_energy_nhwc(*args, s),
                   lambda v, outs: _check_energy(cpu[v], outs[0]))
    return build


def _items(shapes_pads, seed):
    """Several dense tensors, each (n, c, h, w, pad): the device inputs, their variants, their [n, c] outputs."""
    cpus = [_maps(sp[:4], seed + 7 * i) for i, sp in enumerate(shapes_pads)]
    xs = [torch.empty_like(c[0], device=DEV) for c in cpus]
    outs = [torch.empty(sp[:2], dtype=F32, device=DEV) for sp in shapes_pads]
    fresh = [_dev([c[v] for c in cpus]) for v in range(VARIANTS)]

    def check(v, got):
        for c, g, sp in zip(cpus, got, shapes_pads):
            _check_energy(c[v], g, bool(sp[4]))
    return cpus, xs, outs, fresh, check


def _fill_item(t, x, out):
    t.x, t.out_nc, t.N, t.C_total, t.strideN, t.strideC, t.c_begin, t.c_count = (
        x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], x.stride(0), x.stride(1), 0, x.shape[1])


def _multi(h, w, count, pad=0):
    def build():
        lib = _lib.load()
        sp = [(N, C + i, h, w, pad) for i in range(count)]
        _, xs, outs, fresh, check = _items(sp, 130 + h)
        arr = (_lib.TensorItem * count)()
        for t, x, o in zip(arr, xs, outs):
            _fill_item(t, x, o)
        ws = _ws(lib.dcts_workspace_bytes(N, C + count, h, w))
        return Run(xs, fresh, outs, ws, lambda s: lib.dcts_energy_multi_f32(arr, count, h, w, pad, ws.data_ptr(), ws.numel() - 256, s),
                   check, keep=(arr,))
    return build


def _mixed():
    def build():
        lib = _lib.load()
        sp = [(N, C, 32, 32, 0), (N, C + 1, 16, 16, 0), (N, C, 8, 8, 0), (N, C + 2, 4, 4, 0), (N, C, 2, 2, 0), (N, C, 7, 7, 1)]
        _, xs, outs, fresh, check = _items(sp, 140)
        arr = (_lib.ShapedItem * len(sp))()
        for t, x, o, s_ in zip(arr, xs, outs, sp):
            _fill_item(t.t, x, o)
            t.H, t.W, t.pad_front_if_odd = s_[2], s_[3], s_[4]
        ws = _ws(max(lib.dcts_workspace_bytes(*s_[:4]) for s_ in sp))
        return Run(xs, fresh, outs, ws, lambda s: lib.dcts_energy_mixed_f32(arr, len(sp), ws.data_ptr(), ws.numel() - 256, s), check,
                   keep=(arr,))
    return build


def _energies(n, c, seed):
    return [synth(n, c, 8, 8, seed + 1000 * v).pow(2).sum(dim=(-2, -1)) for v in range(VARIANTS)]


def _batch_sum():
    def build():
        lib = _lib.load()
        cpu = _energies(4, 70, 150)
        e = torch.empty_like(cpu[0], device=DEV)
        out = torch.empty(70, dtype=F32, device=DEV)

        def check(v, outs):  # test_gpu_parity.py
            assert torch.allclose(outs[0], cpu[v].sum(0), rtol=1e-6)
        return Run([e], [_dev([t]) for t in cpu], [out], None, lambda s: lib.dcts_batch_sum_f32(e.data_ptr(), 4, 70, out.data_ptr(), s), check)
    return build


def _running_mean(count):
    """count 0: dcts_running_mean_update_f32; else dcts_running_mean_update_multi_f32 with that many hook points."""
    def build():
        lib = _lib.load()
        k = max(count, 1)
        cs = [37 + (i % 3) for i in range(k)]
        cpus = [_energies(4, c, 160 + i) for i, c in enumerate(cs)]
        start = [torch.rand(c, generator=torch.Generator().manual_seed(170 + i)) + 0.5 for i, c in enumerate(cs)]
        es = [torch.empty_like(c[0], device=DEV) for c in cpus]
        frs = [torch.empty(c, dtype=F32, device=DEV) for c in cs]
        start_dev = _dev(start)

        def reset():
            for f, s0 in zip(frs, start_dev):
                f.copy_(s0)
        if count:
            descs = (_lib.UpdateDesc * k)()
            for d, e, f in zip(descs, es, frs):
                d.energy_nc, d.feature_result, d.N, d.C_count, d.total_before = e.data_ptr(), f.data_ptr(), 4, e.shape[1], 8.0
            call = lambda s: lib.dcts_running_mean_update_multi_f32(descs, k, s)  # noqa: E731
        else:
            descs = None
            call = lambda s: lib.dcts_running_mean_update_f32(es[0].data_ptr(), 4, cs[0], frs[0].data_ptr(), 8.0, s)  # noqa: E731

        def check(v, outs):  # test_gpu_parity.py: the reference's host rule, 2e-6 relative
            for c, s0, got in zip(cpus, start, outs):
                host = HostAccumulator()
                host.feature_result, host.total = s0.clone(), torch.tensor(8.)
                host.update(c[v])
                np.testing.assert_allclose(got.numpy(), host.scores(), rtol=2e-6)
        return Run(es, [_dev([c[v] for c in cpus]) for v in range(VARIANTS)], frs, None, call, check, inout=True, reset=reset,
                   keep=(descs, start_dev))
    return build


def _stream_read():
    """k_calib_read stores its sum only where it equals 123456.789f: one element of that value, and the store shows."""
    def build():
        lib = _lib.load()
        magic = torch.tensor([123456.789], dtype=F32)
        x, out = torch.empty(1, dtype=F32, device=DEV), torch.empty(1, dtype=F32, device=DEV)

        def check(v, outs):
            assert torch.equal(outs[0], magic)
        return Run([x], [[magic.to(DEV)] for _ in range(VARIANTS)], [out], None,
                   lambda s: lib.dcts_debug_stream_read_f32(x.data_ptr(), 1, out.data_ptr(), s), check)
    return build


A = ops
EX, CX = "dcts_energy_f32_ex", "dcts_dct2d_f32_ex"
CASES = [
    # ---- dcts_energy_f32_ex: every kernel family --------------------------------------------------------------------------
    Case("energy-codelet8", EX, "codelet", _single(EX, 8, 8, A.ALGO_AUTO), capture=True),  # several maps per wave
    Case("energy-codelet56", EX, "codelet", _single(EX, 56, 56, A.ALGO_AUTO)),
    Case("energy-prefetch16", EX, "codelet", _single(EX, 16, 16, A.ALGO_PREFETCH)),
    Case("energy-lane7", EX, "codelet", _single(EX, 7, 7, A.ALGO_AUTO)),
    Case("energy-rect28x14", EX, "rect", _single(EX, 28, 14, A.ALGO_AUTO), capture=True),
    Case("energy-direct13-built", EX, "direct", _single(EX, 13, 13, A.ALGO_DIRECT), capture=True),
    Case("energy-direct13-reused", EX, "direct", _single(EX, 13, 13, A.ALGO_DIRECT), capture=True, reuse_tables=True),
    Case("energy-split88", EX, "split", _single(EX, 88, 88, A.ALGO_AUTO), capture=True),
    Case("energy-split272", EX, "split_more", _single(EX, 272, 272, A.ALGO_AUTO, shape_nc=(1, 3)), capture=True),
    Case("energy-fused96", EX, "fused", _single(EX, 96, 96, A.ALGO_AUTO), capture=True),
    Case("energy-fused2-288", EX, "fused2", _single(EX, 288, 288, A.ALGO_AUTO, shape_nc=(1, 5)), capture=True),
    Case("energy-pipe128", EX, "pipe", _single(EX, 128, 128, A.ALGO_AUTO), capture=True),
    Case("energy-tile2d224", EX, "tile2d", _single(EX, 224, 224, A.ALGO_AUTO, shape_nc=(1, 5)), capture=True),
    Case("energy-tile2g72", EX, "tile2g", _single(EX, 72, 72, A.ALGO_AUTO), capture=True),
    Case("energy-tile2gpad71", EX, "tile2g", _single(EX, 71, 71, A.ALGO_AUTO, pad=1)),
    Case("energy-auto8", "dcts_energy_f32", "codelet", _single("dcts_energy_f32", 8, 8)),
    # ---- dcts_dct2d_f32_ex: the STORE kernels and k_assemble ----------------------------------------------------------------
    Case("coeff-codelet8", CX, "codelet", _single(CX, 8, 8, A.ALGO_AUTO, store=True)),
    Case("coeff-direct13", CX, "direct", _single(CX, 13, 13, A.ALGO_DIRECT, store=True)),
    Case("coeff-fused96", CX, "fused", _single(CX, 96, 96, A.ALGO_FUSED, store=True)),
    Case("coeff-tile2d224", CX, "tile2d", _single(CX, 224, 224, A.ALGO_TILE2D, store=True, shape_nc=(1, 3))),
    Case("coeff-tile2g72", CX, "tile2g", _single(CX, 72, 72, A.ALGO_TILE2D, store=True)),
    Case("coeff-fused2-288", CX, "fused2", _single(CX, 288, 288, A.ALGO_FUSED, store=True, shape_nc=(1, 3))),
    Case("coeff-auto8", "dcts_dct2d_f32", "codelet", _single("dcts_dct2d_f32", 8, 8, store=True)),
    # ---- the list entry points --------------------------------------------------------------------------------------------
    Case("multi-codelet14", "dcts_energy_multi_f32", "codelet", _multi(14, 14, 3)),
    Case("multi-lane7", "dcts_energy_multi_f32", "codelet", _multi(7, 7, 3)),
    Case("multi-tile2g72", "dcts_energy_multi_f32", "tile2g", _multi(72, 72, 3)),
    Case("multi-rect28x14", "dcts_energy_multi_f32", "rect", _multi(28, 14, 2)),
    Case("mixed-cifar-oddpad", "dcts_energy_mixed_f32", "codelet", _mixed()),
    # ---- weighted, band, entropy, low-pass, rank ----------------------------------------------------------------------------
    Case("weighted13", "dcts_weighted_energy_f32", "rect reduce", _weighted(13)),
    Case("weighted72", "dcts_weighted_energy_f32", "tile2g reduce", _weighted(72)),
    Case("band-fused14", "dcts_band_energy_f32", "band", _band(14, 3), capture=True),
    Case("band-fallback72", "dcts_band_energy_f32", "tile2g band", _band(72, 3)),
    Case("entropy-fused14", "dcts_spectral_entropy_f32", "entropy", _entropy(14), capture=True),
    Case("entropy-fallback72", "dcts_spectral_entropy_f32", "tile2g entropy", _entropy(72)),
    Case("lowpass-fused14", "dcts_dct2d_lowpass_f32", "lowpass", _lowpass(14, 14, 4), capture=True),
    Case("lowpass-fused56-dropdc", "dcts_dct2d_lowpass_f32", "lowpass", _lowpass(56, 56, 8, drop_dc=True)),
    Case("lowpass-fallback13x17", "dcts_dct2d_lowpass_f32", "rect lowpass", _lowpass(13, 17, 8)),
    Case("lowpass-fallback72-dropdc", "dcts_dct2d_lowpass_f32", "direct lowpass", _lowpass(72, 72, 8, drop_dc=True)),
    Case("rank14", "dcts_rank_f32", "rank", _rank(14), capture=True),
    # ---- geometric median -------------------------------------------------------------------------------------------------
    Case("gm-l2", "dcts_gm_distance_f32", "gm", _gm("l2", via_metric=False), capture=True),
    Case("gm-metric-l2", "dcts_gm_distance_metric_f32", "gm", _gm("l2")),
    Case("gm-metric-cosine", "dcts_gm_distance_metric_f32", "gm", _gm("cosine")),
    Case("gm-metric-correlation", "dcts_gm_distance_metric_f32", "gm", _gm("correlation")),
    Case("gm-pairs-l2", "dcts_gm_pairs_f32", "gm_pairs", _gm("l2", pairs=True, shape=po.REGIMES[0][1:3] + po.REGIMES[0][3])),
    Case("gm-pairs-cosine", "dcts_gm_pairs_f32", "gm gm_pairs", _gm("cosine", pairs=True, shape=po.REGIMES[0][1:3] + po.REGIMES[0][3]),
         capture=True),
    # ---- fp16 / bf16, channels-last ---------------------------------------------------------------------------------------
    Case("typed-f16-native14", "dcts_energy_typed", "half", _typed(F16, 14), capture=True),
    Case("typed-bf16-native14", "dcts_energy_typed", "half", _typed(BF16, 14)),
    Case("typed-f16-staged20", "dcts_energy_typed", "half codelet", _typed(F16, 20)),
    Case("typed-bf16-staged20", "dcts_energy_typed", "half codelet", _typed(BF16, 20)),
    Case("nhwc-f32-lane8", "dcts_energy_nhwc", "nhwc", _nhwc(F32, 8)),
    Case("nhwc-bf16-lane8", "dcts_energy_nhwc", "nhwc", _nhwc(BF16, 8)),
    Case("nhwc-f32-block14", "dcts_energy_nhwc", "nhwc", _nhwc(F32, 14), capture=True),
    Case("nhwc-bf16-block14", "dcts_energy_nhwc", "nhwc", _nhwc(BF16, 14)),
    Case("nhwc-f32-strip56", "dcts_energy_nhwc", "nhwc", _nhwc(F32, 56)),
    Case("nhwc-bf16-strip56", "dcts_energy_nhwc", "nhwc", _nhwc(BF16, 56)),
    # ---- reductions -------------------------------------------------------------------------------------------------------
    Case("batch-sum", "dcts_batch_sum_f32", "reduce", _batch_sum(), capture=True),
    Case("running-mean", "dcts_running_mean_update_f32", "reduce", _running_mean(0)),
    Case("running-mean-multi70", "dcts_running_mean_update_multi_f32", "reduce", _running_mean(70)),
    Case("stream-read", "dcts_debug_stream_read_f32", "reduce", _stream_read()),
]
