"""Operator-level seam: the tensor -> per-map energy call that replaces the reference's
Python list comprehension over maps (utils/common.py:265-270, :283-287, :299-303)."""
import torch

from . import _lib

ALGO_AUTO, ALGO_DIRECT, ALGO_CODELET, ALGO_SPLIT, ALGO_PREFETCH, ALGO_FUSED, ALGO_PIPE, ALGO_LANE, ALGO_TILE2D, ALGO_RECT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9

# one scratch buffer per (device, stream); grown on demand, reused across calls
_workspaces = {}


def _workspace(device, stream_ptr, nbytes):
    key = (device.index, stream_ptr)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:  # the allocator may hand these bytes out again
            _lib.load().dcts_workspace_invalidate_range(buf.data_ptr(), buf.numel())
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _lib.load().dcts_workspace_invalidate_range(buf.data_ptr(), buf.numel())
        _workspaces[key] = buf
    return buf


# dcts_energy_typed's DCTS_DTYPE_* of the 2-byte element types energy_nc takes besides float32
_HALF_DTYPES = {torch.float16: 1, torch.bfloat16: 2}


def _check_input(x, half_ok=False, algo=ALGO_AUTO):
    if not isinstance(x, torch.Tensor):
        raise TypeError("expected a torch.Tensor")
    if x.dim() != 4:
        raise ValueError("expected [N, C, H, W], got shape %s" % (tuple(x.shape),))
    if x.dtype != torch.float32 and not (half_ok and x.dtype in _HALF_DTYPES):
        raise TypeError("feature maps must be float32 (the reference path is fp32)%s, got %s"
                        % (", float16 or bfloat16" if half_ok else "", x.dtype))
    if not x.is_cuda:
        raise RuntimeError(
            "dct_pruning_amd runs on the GPU only: got a %s tensor. There is no CPU fallback; "
            "the CPU restatement under oracle/ is test infrastructure." % x.device)
    if x.dtype != torch.float32 and algo != ALGO_AUTO:
        raise ValueError("float16 / bfloat16 feature maps take ALGO_AUTO only, got algo=%r" % (algo,))


def _slice(x, c_begin, c_count):
    C = x.shape[1]
    if c_count is None:
        c_count = C - c_begin
    return int(c_begin), int(c_count)


def _rows(x, dense=False):
    """x with W-contiguous rows, copied if need be; dense: without a row pitch as well (the list entry points)."""
    W = x.shape[3]
    if x.stride(3) != 1 or (x.stride(2) != W if dense else x.stride(2) < W):
        x = x.contiguous()
    return x


def _open(x, c_begin, c_count, out=None, half_ok=False, algo=ALGO_AUTO, rows="pitched"):
    """The opening every entry point shares: input check, channel slice, the [N, c_count] output (out=None: a new one;
    a tensor: checked; False: the caller makes its own), the .contiguous() fallback (rows: "pitched", "dense" for the
    list entry points, None to leave x as it lies) and the current stream of x's device.
    Returns (x, c_begin, c_count, out, stream)."""
    _check_input(x, half_ok, algo)
    c_begin, c_count = _slice(x, c_begin, c_count)
    N = x.shape[0]
    if out is None:
        out = torch.empty((N, c_count), dtype=torch.float32, device=x.device)
    elif out is not False and (out.shape != (N, c_count) or out.dtype != torch.float32 or not out.is_contiguous()
                               or out.device != x.device):
        raise ValueError("out must be a contiguous float32 [N, c_count] tensor on x's device")
    if rows is not None:
        x = _rows(x, rows == "dense")
    return x, c_begin, c_count, out, torch.cuda.current_stream(x.device).cuda_stream


def _launch(device, fn, *args):
    """fn(*args) with `device` current; a status other than 0 raises (_lib.check)."""
    with torch.cuda.device(device):
        _lib.check(fn(*args))


def has_codelet(H, W):
    return bool(_lib.load().dcts_has_codelet(H, W))


def _call(fn_name, x, c_begin, c_count, pad_front_if_odd, out, algo, stream):
    lib = _lib.load()
    N, C, H, W = x.shape
    ws = _workspace(x.device, stream, lib.dcts_workspace_bytes(N, c_count, H, W))
    _launch(x.device, getattr(lib, fn_name),
            x.data_ptr(), N, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3),
            c_begin, c_count, 1 if pad_front_if_odd else 0, out.data_ptr(),
            ws.data_ptr(), ws.numel(), stream, algo)
    return out


def has_half_kernel(H, W):
    """True if float16 / bfloat16 maps of a dense (H, W) tile have a kernel of their own (no odd pad); every other
    shape is upcast chunk by chunk into the workspace and scored by the float32 kernels."""
    return bool(_lib.load().dcts_has_half_kernel(H, W))


def _call_half(x, c_begin, c_count, pad_front_if_odd, out, stream):
    lib = _lib.load()
    N, C, H, W = x.shape
    dtype = _HALF_DTYPES[x.dtype]
    nbytes = lib.dcts_typed_workspace_bytes(dtype, N, c_count, H, W)
    if lib.dcts_has_half_kernel(H, W) and (x.stride(2) != W or (pad_front_if_odd and H % 2 == 1)):
        # a native shape the kernel does not take is staged like the others: sized as the header says, for (H, W + 1)
        nbytes = lib.dcts_typed_workspace_bytes(dtype, N, c_count, H, W + 1)
    ws = _workspace(x.device, stream, nbytes)
    _launch(x.device, lib.dcts_energy_typed,
            x.data_ptr(), dtype, N, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3),
            c_begin, c_count, 1 if pad_front_if_odd else 0, out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    return out


def has_nhwc_kernel(H, W):
    """True if channels-last maps of a dense (H, W) tile have a kernel of their own (dcts_energy_nhwc; no odd pad);
    every other shape that is not W-contiguous is copied into the NCHW layout first."""
    return bool(_lib.load().dcts_has_nhwc_kernel(H, W))


ROUTE_NCHW, ROUTE_NHWC, ROUTE_COPY = 1, 2, 3


def energy_route(shape, stride, pad_front_if_odd=False, algo=ALGO_AUTO, has_kernel=None):
    """How energy_nc reaches a kernel for a tensor of this shape and these strides (elements), decided in this order:
    ROUTE_NCHW  rows are W-contiguous (stride(3) == 1, stride(2) >= W): the NCHW kernels read it as it is;
    ROUTE_NHWC  the channel stride is 1, stride(3) >= C, stride(2) >= W * stride(3), (H, W) has a channels-last kernel,
                no odd pad is taken and algo is ALGO_AUTO: dcts_energy_nhwc reads it as it is;
    ROUTE_COPY  everything else: .contiguous() first, then ROUTE_NCHW.
    `has_kernel(H, W)` defaults to has_nhwc_kernel (the built library); tests pass their own to stay off the GPU."""
    N, C, H, W = shape
    sN, sC, sH, sW = stride
    if sW == 1 and sH >= W:
        return ROUTE_NCHW
    pad = bool(pad_front_if_odd) and H % 2 == 1
    if sC == 1 and sW >= C and sH >= W * sW and not pad and algo == ALGO_AUTO:
        if (has_nhwc_kernel if has_kernel is None else has_kernel)(H, W):
            return ROUTE_NHWC
    return ROUTE_COPY


_NHWC_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _call_nhwc(x, c_begin, c_count, out, stream):
    N, C, H, W = x.shape
    _launch(x.device, _lib.load().dcts_energy_nhwc,
            x.data_ptr(), _NHWC_DTYPES[x.dtype], N, C, H, W, x.stride(0), x.stride(2), x.stride(3),
            c_begin, c_count, out.data_ptr(), None, 0, stream)
    return out


def energy_nc(x, c_begin=0, c_count=None, pad_front_if_odd=False, algo=ALGO_AUTO, out=None):
    """E[n, j] = sum_{u,v} dct_2d(x[n, c_begin+j], norm='ortho')[u,v]**2  -> [N, c_count] fp32.

    pad_front_if_odd=True reproduces torch2dct (utils/common.py:230-239): an odd-H map gets
    one zero row and one zero column in front before the transform.
    x may be float16 or bfloat16 as well (a forward pass under autocast): every element is upcast exactly and the
    arithmetic is fp32, so the result is that of x.float() without the copy (dcts_energy_typed; algo must be ALGO_AUTO).
    A channels-last tensor (torch.channels_last, or a channel slice / sample-strided view of one) of a shape
    has_nhwc_kernel names is read where it lies (energy_route: dcts_energy_nhwc, any of the three dtypes); every other
    tensor whose rows are not W-contiguous is copied with .contiguous() first.
    Enqueues on the current stream of x's device; no synchronisation.
    """
    x, c_begin, c_count, out, stream = _open(x, c_begin, c_count, out, half_ok=True, algo=algo, rows=None)
    if energy_route(x.shape, x.stride(), pad_front_if_odd, algo) == ROUTE_NHWC:
        return _call_nhwc(x, c_begin, c_count, out, stream)
    x = _rows(x)
    if x.dtype != torch.float32:
        return _call_half(x, c_begin, c_count, pad_front_if_odd, out, stream)
    return _call("dcts_energy_f32_ex", x, c_begin, c_count, pad_front_if_odd, out, algo, stream)


def dct2d(x, c_begin=0, c_count=None, pad_front_if_odd=False, algo=ALGO_AUTO):
    """Orthonormal 2-D DCT-II coefficients of every map -> [N, c_count, H', W'] fp32."""
    x, c_begin, c_count, _, stream = _open(x, c_begin, c_count, out=False)
    N, _, H, W = x.shape
    pad = 1 if (pad_front_if_odd and H % 2 == 1) else 0
    out = torch.empty((N, c_count, H + pad, W + pad), dtype=torch.float32, device=x.device)
    return _call("dcts_dct2d_f32_ex", x, c_begin, c_count, pad_front_if_odd, out, algo, stream)


def batch_sum(energy):
    """out[j] = sum_n energy[n, j] in the fixed order of dcts_batch_sum_f32 (include/dctscore.h): 16 interleaved slices,
    slice s adds n = s, s+16, ... ascending, then the 16 partial sums are added in slice order (fused variant for the
    bench / single-sweep mode; tests/reduce_oracle.py states the order in numpy)."""
    if energy.dim() != 2 or energy.dtype != torch.float32 or not energy.is_cuda:
        raise ValueError("expected a float32 CUDA tensor [N, C]")
    energy = energy.contiguous()
    out = torch.empty((energy.shape[1],), dtype=torch.float32, device=energy.device)
    stream = torch.cuda.current_stream(energy.device).cuda_stream
    _launch(energy.device, _lib.load().dcts_batch_sum_f32, energy.data_ptr(), energy.shape[0], energy.shape[1],
            out.data_ptr(), stream)
    return out


def _pack_item(t, x, c_begin, c_count):
    """Fills the dcts_tensor_item `t` for a channel slice of x; returns (x as the kernels read it, its [N, c_count]
    output, the workspace bytes it needs)."""
    x, c_begin, c_count, out, _ = _open(x, c_begin, c_count, rows="dense")
    t.x, t.out_nc = x.data_ptr(), out.data_ptr()
    t.N, t.C_total = x.shape[0], x.shape[1]
    t.strideN, t.strideC = x.stride(0), x.stride(1)
    t.c_begin, t.c_count = c_begin, c_count
    return x, out, _lib.load().dcts_workspace_bytes(x.shape[0], c_count, x.shape[2], x.shape[3])


def energy_multi(items, pad_front_if_odd=False):
    """energy_nc for several tensors of the SAME (H, W) in one launch.

    items: list of (x, c_begin, c_count) with x [N, C, H, W] fp32 CUDA (c_count None = to the end).
    Returns the list of [N, c_count] outputs. Tensors must stay alive until the stream has run."""
    lib = _lib.load()
    if not items:
        return []
    H, W = items[0][0].shape[2], items[0][0].shape[3]
    dev = items[0][0].device
    arr = (_lib.TensorItem * len(items))()
    outs, keep = [], []
    need = 0
    for i, (x, c_begin, c_count) in enumerate(items):
        x, out, nbytes = _pack_item(arr[i], x, c_begin, c_count)
        if x.shape[2] != H or x.shape[3] != W or x.device != dev:
            raise ValueError("energy_multi needs tensors of one tile shape on one device")
        keep.append(x)
        outs.append(out)
        need = max(need, nbytes)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _workspace(dev, stream, need)
    _launch(dev, lib.dcts_energy_multi_f32, arr, len(items), H, W, 1 if pad_front_if_odd else 0,
            ws.data_ptr(), ws.numel(), stream)
    return outs


def energy_mixed(items):
    """energy_nc for tensors of ANY tile shapes in one call (dcts_energy_mixed_f32): small square tiles
    (edges 2..32) of all shapes share one launch, the rest go shape by shape.

    items: list of (x, c_begin, c_count, pad_front_if_odd). Returns the list of [N, c_count] outputs;
    the tensors must stay alive until the stream has run."""
    lib = _lib.load()
    if not items:
        return []
    dev = items[0][0].device
    arr = (_lib.ShapedItem * len(items))()
    outs, keep = [], []
    need = 0
    for i, (x, c_begin, c_count, pad) in enumerate(items):
        x, out, nbytes = _pack_item(arr[i].t, x, c_begin, c_count)
        if x.device != dev:
            raise ValueError("energy_mixed needs tensors on one device")
        keep.append(x)
        outs.append(out)
        arr[i].H, arr[i].W, arr[i].pad_front_if_odd = x.shape[2], x.shape[3], 1 if pad else 0
        need = max(need, nbytes)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _workspace(dev, stream, need)
    _launch(dev, lib.dcts_energy_mixed_f32, arr, len(items), ws.data_ptr(), ws.numel(), stream)
    return outs


def weighted_energy_nc(x, weights, c_begin=0, c_count=None, pad_front_if_odd=False):
    """Coefficient-domain score variant: E[n, j] = sum_{u,v} weights[u,v] * dct_2d(x[n, c_begin+j])[u,v]**2.
    `weights`: [H', W'] fp32 on x's device (H' = H + 1 for an odd H with pad_front_if_odd). All ones gives energy_nc."""
    x, c_begin, c_count, out, stream = _open(x, c_begin, c_count)
    N, C, H, W = x.shape
    pad = 1 if (pad_front_if_odd and H % 2 == 1) else 0
    if weights.shape != (H + pad, W + pad) or weights.dtype != torch.float32 or weights.device != x.device:
        raise ValueError("weights must be a float32 [%d, %d] tensor on %s" % (H + pad, W + pad, x.device))
    weights = weights.contiguous()
    lib = _lib.load()
    ws = _workspace(x.device, stream, lib.dcts_weighted_workspace_bytes(N, c_count, H, W))
    _launch(x.device, lib.dcts_weighted_energy_f32,
            x.data_ptr(), N, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3), c_begin, c_count,
            1 if pad_front_if_odd else 0, weights.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    return out


def has_band_kernel(H, W):
    """True if the fused band kernel takes an (H, W) tile (sizes after the odd pad)."""
    return bool(_lib.load().dcts_has_band_kernel(H, W))


def band_energy_nc(x, weights, c_begin=0, c_count=None, pad_front_if_odd=False, algo=ALGO_AUTO):
    """K weighted energies per map in one pass: E[n, j, b] = sum_{u,v} weights[b,u,v] * dct_2d(x[n, c_begin+j])[u,v]**2
    -> [N, c_count, K] fp32. `weights`: [K, H', W'] fp32 on x's device, K = 1 ... 8 (H' = H + 1 for an odd H with
    pad_front_if_odd); one-hot weights (bands.partition) give the energy of K frequency bands.
    algo: ALGO_AUTO (fused kernel where it exists, else the fallback), ALGO_CODELET (fused only), ALGO_DIRECT
    (fallback only). Enqueues on the current stream of x's device; no synchronisation."""
    x, c_begin, c_count, _, stream = _open(x, c_begin, c_count, out=False)
    N, C, H, W = x.shape
    pad = 1 if (pad_front_if_odd and H % 2 == 1) else 0
    if (not isinstance(weights, torch.Tensor) or weights.dim() != 3 or tuple(weights.shape[1:]) != (H + pad, W + pad)
            or weights.dtype != torch.float32 or weights.device != x.device):
        raise ValueError("weights must be a float32 [K, %d, %d] tensor on %s" % (H + pad, W + pad, x.device))
    K = weights.shape[0]
    weights = weights.contiguous()
    lib = _lib.load()
    out = torch.empty((N, c_count, K), dtype=torch.float32, device=x.device)
    ws = _workspace(x.device, stream, max(lib.dcts_band_workspace_bytes(N, c_count, H, W, K), 16))
    _launch(x.device, lib.dcts_band_energy_f32,
            x.data_ptr(), N, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3), c_begin, c_count,
            1 if pad_front_if_odd else 0, weights.data_ptr(), K, out.data_ptr(), ws.data_ptr(), ws.numel(), stream, algo)
    return out


def has_entropy_kernel(H, W):
    """True if the fused spectral-entropy kernel takes an (H, W) tile (sizes after the odd pad)."""
    return bool(_lib.load().dcts_has_entropy_kernel(H, W))


def spectral_entropy_nc(x, c_begin=0, c_count=None, pad_front_if_odd=False, algo=ALGO_AUTO, out=None):
    """S[n, j] = -sum p ln p over p = c**2 / sum c**2, c = dct_2d(x[n, c_begin+j], norm='ortho') -> [N, c_count] fp32.

    The spectral entropy of every map (dcts_spectral_entropy_f32): how widely its energy spreads over the DCT
    coefficients, in [0, ln(H' * W')] (natural log; H' = H + 1 for an odd H with pad_front_if_odd). A flat or blob-like
    map is near 0, a textured one near the top; an all-zero map gives +0.0; scaling a map does not change its value.
    algo: ALGO_AUTO (fused kernel where it exists, else the fallback), ALGO_CODELET (fused only), ALGO_DIRECT
    (fallback only). float32 NCHW only; a tensor whose rows are not W-contiguous is copied with .contiguous() first.
    Enqueues on the current stream of x's device; no synchronisation."""
    x, c_begin, c_count, out, stream = _open(x, c_begin, c_count, out)
    N, C, H, W = x.shape
    lib = _lib.load()
    nbytes = lib.dcts_entropy_workspace_bytes(N, c_count, H, W)
    if nbytes == 0 and (x.stride(2) != W or algo == ALGO_DIRECT):
        # a fused shape that takes the fallback: sized as the header says, for (H, W + 1)
        nbytes = lib.dcts_entropy_workspace_bytes(N, c_count, H, W + 1)
    ws = _workspace(x.device, stream, nbytes) if nbytes else None
    _launch(x.device, lib.dcts_spectral_entropy_f32,
            x.data_ptr(), N, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3), c_begin, c_count,
            1 if pad_front_if_odd else 0, out.data_ptr(), ws.data_ptr() if nbytes else None, ws.numel() if nbytes else 0,
            stream, algo)
    return out


def rank_nc(x, c_begin=0, c_count=None, out=None):
    """R[n, j] = numerical rank of x[n, c_begin+j] -> [N, c_count] fp32 (exact integers; all-zero map: +0.0).

    The HRank criterion (dcts_rank_f32): #{sigma_i > max(H, W) * 2^-23 * sigma_max}, the default rule of
    torch.linalg.matrix_rank for fp32, computed in fp64. Edges up to 64 on each axis.
    Enqueues on the current stream of x's device; no synchronisation.
    """
    x, c_begin, c_count, out, stream = _open(x, c_begin, c_count, out)
    N, C, H, W = x.shape
    _launch(x.device, _lib.load().dcts_rank_f32, x.data_ptr(), N, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3),
            c_begin, c_count, out.data_ptr(), stream)
    return out


LOWPASS_DROP_DC = 1  # DCTS_LOWPASS_DROP_DC


def lowpass_nc(x, K, c_begin=0, c_count=None, drop_dc=False, out=None):
    """S[n, j] = dct_2d(x[n, c_begin+j], norm='ortho')[:K, :K] -> [N, c_count, min(K, H), min(K, W)] fp32.

    The low-pass signature of every map (dcts_dct2d_lowpass_f32): its K x K lowest DCT coefficients and nothing else, in one
    pass that reads the map once. An edge shorter than K keeps all its coefficients. drop_dc=True writes S[..., 0, 0] as +0.0
    (the signature of the centred map) and gives a flat map - every element equal, all-zero maps included - an all-+0.0
    signature; the test is made on the map itself, exactly. Dense square maps of an edge has_codelet names take one fused
    launch; every other shape up to 512 and every tensor whose rows have a pitch take the coefficient path of dct2d into the
    workspace and a gather, and give the corner of dct2d's output bit for bit.
    float32 NCHW only; a tensor whose rows are not W-contiguous is copied with .contiguous() first. `out`: a contiguous
    float32 tensor of the result's shape on x's device to overwrite. Enqueues on the current stream of x's device; no
    synchronisation."""
    K = int(K)
    if K < 1:
        raise ValueError("lowpass_nc needs K >= 1, got %r" % (K,))
    x, c_begin, c_count, _, stream = _open(x, c_begin, c_count, out=False)
    N, C, H, W = x.shape
    shape = (N, c_count, min(K, H), min(K, W))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif out.shape != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous float32 %s tensor on x's device" % (list(shape),))
    lib = _lib.load()
    nbytes = lib.dcts_dct2d_lowpass_workspace_bytes(N, c_count, H, W, K)
    if nbytes == 0 and (x.stride(2) != W or x.stride(1) != H * W):
        # a fused shape that takes the fallback: sized as the header says, for (H, W + 1)
        nbytes = lib.dcts_dct2d_lowpass_workspace_bytes(N, c_count, H, W + 1, K)
    ws = _workspace(x.device, stream, nbytes) if nbytes else None
    _launch(x.device, lib.dcts_dct2d_lowpass_f32,
            x.data_ptr(), N, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3), c_begin, c_count, K,
            LOWPASS_DROP_DC if drop_dc else 0, out.data_ptr(), ws.data_ptr() if nbytes else None, ws.numel() if nbytes else 0,
            stream)
    return out


GM_METRICS = {"l2": 0, "cosine": 1, "correlation": 2}  # DCTS_GM_*


def _gm_lowpass(fn, x, K, c_begin, c_count, ref_begin, ref_count, metric, out):
    """fn (gm_distance_nc or gm_pair_matrix) on the low-pass signatures of x: those of the channel hull of the two ranges,
    with both ranges shifted by the hull's start. "correlation" drops the DC term, which is the centring, and then compares
    as "cosine" does."""
    K = int(K)
    if K < 0:
        raise ValueError("lowpass must be >= 0, got %r" % (K,))
    if metric not in GM_METRICS:
        raise ValueError("metric must be one of %s, got %r" % (", ".join(GM_METRICS), metric))
    if K == 1 and metric == "correlation":
        raise ValueError("lowpass=1 under metric='correlation' keeps the DC term alone, which the centring removes: nothing is left")
    _check_input(x)
    c_begin, c_count = _slice(x, c_begin, c_count)
    ref_begin, ref_count = _slice(x, ref_begin, ref_count)
    lo, hi = min(c_begin, ref_begin), max(c_begin + c_count, ref_begin + ref_count)
    sig = lowpass_nc(x, K, c_begin=lo, c_count=hi - lo, drop_dc=(metric == "correlation"))
    return fn(sig, c_begin=c_begin - lo, c_count=c_count, ref_begin=ref_begin - lo, ref_count=ref_count, out=out,
              metric="cosine" if metric == "correlation" else metric)


def gm_distance_nc(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None, out=None, metric="l2", lowpass=0):
    """G[n, j] = sum_k ||x[n, c_begin+j] - x[n, k]||_2 over the reference channels k in [ref_begin, ref_begin + ref_count)
    -> [N, c_count] fp32 (ref_count None = to the end).

    The geometric-median criterion on feature maps (dcts_gm_distance_f32): the summed Euclidean distance (over the H * W
    elements) of every scored map to the maps of the reference set of its sample. A map close to the others, one they can
    stand in for, scores low; high = keep. Computed in the difference form: the term of a map with itself is exactly 0, two
    identical maps are at distance +0.0, and pieces of a channel range scored against the same reference set concatenate
    to the unsplit result bit for bit. There is no odd front pad: zeros in front of both maps change no distance.
    metric: "l2" compares the maps as they are. "cosine" and "correlation" (dcts_gm_distance_metric_f32) compare unit maps,
    x / ||x|| and (x - mean) / ||x - mean||, so that a map and a scaled copy of it are at distance 0 (exactly +0.0 for a power of
    two) and every term lies in [0, 2]. A map with nothing to normalise (all zeros; under "correlation" any constant map) counts
    as the zero map: distance 1 to every other map, exactly 0 to the other flat ones, so dead channels score low.
    lowpass=K > 0 takes the distance between the maps' low-pass signatures instead, d_K(a, b) = ||P_K DCT(a) - P_K DCT(b)||_2
    with P_K the K x K lowest frequencies of the orthonormal DCT (lowpass_nc; K >= max(H, W) is the plain distance up to
    rounding): two maps that share their coarse structure and differ in fine texture or noise are then close. The signatures
    of the channel hull of the two ranges are computed once and this function runs on them: "l2" as it is; "cosine" on the
    unit signatures; "correlation" as "cosine" on the signatures without their DC term (drop_dc: the mean of a map is its DC
    coefficient, so the centring is the dropped term), where a flat map is the zero map as above. Everything exact above holds
    of the signatures. A map with an edge below K keeps all its coefficients along that edge. A non-flat map whose low band
    is empty (all its structure above K) is compared by what its signature holds: round-off under a metric, which normalises
    it. The signature pass runs on every call, over the whole hull: scoring a layer in several channel ranges against the
    same reference set repeats it per range (same bits; a caller that minds computes lowpass_nc once and passes the
    signatures). ValueError for K < 0, and for K = 1 under "correlation" (nothing is left). lowpass=0 is the call it always was.
    float32 NCHW only; a tensor whose maps are not dense (stride(3) != 1 or stride(2) != W) is copied with .contiguous()
    first. Enqueues on the current stream of x's device; no synchronisation."""
    if lowpass:
        return _gm_lowpass(gm_distance_nc, x, lowpass, c_begin, c_count, ref_begin, ref_count, metric, out)
    if metric not in GM_METRICS:
        raise ValueError("metric must be one of %s, got %r" % (", ".join(GM_METRICS), metric))
    x, c_begin, c_count, out, stream = _open(x, c_begin, c_count, out, rows="dense")
    ref_begin, ref_count = _slice(x, ref_begin, ref_count)
    N, C, H, W = x.shape
    lib = _lib.load()
    args = (x.data_ptr(), N, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3), c_begin, c_count, ref_begin, ref_count,
            out.data_ptr(), stream)
    if metric == "l2":
        _launch(x.device, lib.dcts_gm_distance_f32, *args)
        return out
    ws = _workspace(x.device, stream, max(lib.dcts_gm_workspace_bytes(GM_METRICS[metric], N, c_count, ref_count), 16))
    _launch(x.device, lib.dcts_gm_distance_metric_f32, *args, GM_METRICS[metric], ws.data_ptr(), ws.numel())
    return out


def gm_pair_matrix(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None, metric="l2", out=None, lowpass=0):
    """D[j, k] = sum_n d(x[n, c_begin+j], x[n, ref_begin+k]) -> [c_count, ref_count] fp32 (ref_count None = to the end).

    The pair matrix of the geometric-median criterion (dcts_gm_pairs_f32): the terms gm_distance_nc adds up over the reference
    channels, every one kept and summed over the samples of the batch instead (a sum, not a mean: divide by x.shape[0]). d is
    gm_distance_nc's distance under `metric`, with everything that is exact there: D[c, c] = +0.0, identical maps (under a metric,
    power-of-two multiples) at +0.0, D[j, k] and D[k, j] of a square call the same bits, and the rows of a channel range scored
    against the same reference set are the rows of the whole matrix bit for bit. Selection rules on it are host arithmetic
    (dct_pruning_amd.pairs).
    float32 NCHW only; a tensor whose maps are not dense is copied with .contiguous() first. `out`: a contiguous float32
    [c_count, ref_count] tensor on x's device to overwrite. lowpass=K > 0: the distances between the maps' low-pass signatures,
    composed as gm_distance_nc composes them (same rules, same errors); lowpass=0 is the call it always was.
    Enqueues on the current stream of x's device; no synchronisation."""
    if lowpass:
        return _gm_lowpass(gm_pair_matrix, x, lowpass, c_begin, c_count, ref_begin, ref_count, metric, out)
    if metric not in GM_METRICS:
        raise ValueError("metric must be one of %s, got %r" % (", ".join(GM_METRICS), metric))
    x, c_begin, c_count, _, stream = _open(x, c_begin, c_count, out=False, rows="dense")
    ref_begin, ref_count = _slice(x, ref_begin, ref_count)
    if out is None:
        out = torch.empty((c_count, ref_count), dtype=torch.float32, device=x.device)
    elif (out.shape != (c_count, ref_count) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device):
        raise ValueError("out must be a contiguous float32 [c_count, ref_count] tensor on x's device")
    N, C, H, W = x.shape
    lib = _lib.load()
    ws = _workspace(x.device, stream, max(lib.dcts_gm_pairs_workspace_bytes(GM_METRICS[metric], N, c_count, ref_count), 16))
    _launch(x.device, lib.dcts_gm_pairs_f32, x.data_ptr(), N, C, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3),
            c_begin, c_count, ref_begin, ref_count, out.data_ptr(), stream, GM_METRICS[metric], ws.data_ptr(), ws.numel())
    return out
