"""CPU definitions of the band energies (dcts_band_energy_f32) - TEST INFRASTRUCTURE, no product import.

  band_energy_nc_f64   the definition: band b of a tensor is oracle.dct_oracle.weighted_energy_nc_f64(x, weights[b]),
                       stacked over b (float64, SciPy's transform).
  band_energy_nc_f32   "the reference" of the accuracy tests: the oracle's fp32 restatement of the reference's
                       transform (dct_2d, or torch2dct's fp32 SciPy dctn behind the odd front pad), with the band sums
                       taken in fp32. Its own error against float64 sets the tolerance (dct_probes' rule).
  band_energy_nc       band_energy_nc_f32 as a torch tensor with ops.band_energy_nc's signature: what the CPU tests
                       swap in for harness._band_energy_nc.
"""
import numpy as np
import torch

from oracle import dct_oracle as orc


def _weights_np(weights):
    w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)
    assert w.ndim == 3, "weights are [K, H', W']"
    return w


def band_energy_nc_f64(x, weights, c_begin=0, c_count=None, pad_front_if_odd=False):
    """numpy float64 [N, c_count, K]."""
    w = _weights_np(weights)
    return np.stack([orc.weighted_energy_nc_f64(x, w[b], c_begin, c_count, pad_front_if_odd) for b in range(w.shape[0])],
                    axis=-1)


def band_energy_nc_f32(x, weights, c_begin=0, c_count=None, pad_front_if_odd=False):
    """torch float32 [N, c_count, K]: fp32 transform (the oracle's restatement of the reference), fp32 band sums."""
    x = x.detach().cpu().float()
    w = torch.from_numpy(_weights_np(weights).astype(np.float32))
    if c_count is None:
        c_count = x.shape[1] - c_begin
    xs = x[:, c_begin:c_begin + c_count]
    if pad_front_if_odd and xs.shape[2] % 2 != 0:
        xs = torch.nn.functional.pad(xs, (1, 0, 1, 0))
        # torch2dct: SciPy's dctn on float32 input computes in float32
        d = torch.from_numpy(orc._scipy_dctn(xs.contiguous().numpy(), type=2, norm="ortho", axes=(-2, -1)).astype(np.float32))
    else:
        d = orc.dct_2d(xs.contiguous(), norm="ortho")
    assert tuple(w.shape[1:]) == tuple(d.shape[2:]), (tuple(w.shape), tuple(d.shape))
    sq = d * d
    return torch.stack([(w[b][None, None] * sq).sum(dim=(-2, -1)) for b in range(w.shape[0])], dim=-1)


def band_energy_nc(x, weights, c_begin=0, c_count=None, pad_front_if_odd=False, algo=0):
    return band_energy_nc_f32(x, weights, c_begin, c_count, pad_front_if_odd)


def map_energy_f64(x, c_begin=0, c_count=None):
    """E_map: float64 total energy of every scored map (Parseval: sum x^2; the zero pad adds nothing), numpy [N, c]."""
    a = x.detach().cpu().numpy().astype(np.float64)
    if c_count is None:
        c_count = a.shape[1] - c_begin
    a = a[:, c_begin:c_begin + c_count]
    return (a * a).sum(axis=(-2, -1))


def band_error(got, x, weights, c_begin=0, c_count=None, pad_front_if_odd=False):
    """max over maps and bands of |got[b] - f64[b]| / E_map (maps with E_map == 0 must be exactly +0.0 and are left out of
    the maximum). got: [N, c, K] tensor or array."""
    ref = band_energy_nc_f64(x, weights, c_begin, c_count, pad_front_if_odd)
    e_map = map_energy_f64(x, c_begin, c_count)
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    live = e_map > 0
    if (~live).any():
        dead = g[~live]
        assert (dead == 0).all() and not np.signbit(dead).any(), "a zero map must give +0.0 in every band"
    if not live.any():
        return 0.0
    err = np.abs(g - ref)[live] / e_map[live][:, None]
    err = np.where(np.isfinite(err), err, np.inf)
    return float(err.max())
