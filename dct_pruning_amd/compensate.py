"""Compensate a prune: merge the removed input channels of every consumer into the kept ones by least squares
 - the step behind prune_network(..., carry=True).

carry drops what a removed filter fed into the next layer. Where that filter's map is (nearly) a linear combination of
kept maps, x_D ~ A x_S, the consumer can have it back: W_S x_S + W_D x_D ~ (W_S + W_D A) x_S. The A that minimises
sum |x_D - A x_S|^2 over every position of a few calibration batches needs only the uncentred second moments of the
consumer's input, M = sum x x^T / n:

    A = M_DS pinv(M_SS)

    collect_moments   one sweep over the calibration batches with forward pre-hooks on the consumers: {module: Moments(n, G)},
                      G = sum x x^T in float64, [C_in, C_in], in the channel numbering of the full net;
    merge_matrix      (A, residual) from G, n and the kept channels S;
    compensate        W'[:, S] = W[rows][:, S] + W[rows][:, D] A for every consumer of transplant.dataflow(name) whose input
                      lost channels, written into the pruned net in place.

A pseudo-inverse, no ridge and no solve: kept channels that are dead or copies of each other make M_SS singular in every
real net. No intercept: the fit goes through the origin, so a zero input still maps to zero - what a conv's zero padding
needs - and only consumer weights change, no bias and no batch-norm tensor.

Host-side plumbing through PyTorch, on whatever device the nets live on: one [C, n] x [n, C] product per consumer per batch.
"""
import warnings
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import transplant as _tp

Moments = namedtuple("Moments", "n G")
Moments.__doc__ = """Second moments of one consumer's input: n positions (N*H*W of a conv's input, N of a linear layer's) and
G = sum over them of x x^T, float64 [C_in, C_in] on the device the net ran on; G / n is the uncentred moment matrix."""

Merged = namedtuple("Merged", "module n kept removed residual")
Merged.__doc__ = """What compensate did to one consumer: its name, the positions its moments were taken over, how many of its
input channels are kept (|S|) and removed (|D|), and the share of the removed channels' energy the fit does not explain."""


def _consumers(name):
    return [f for f in _tp.dataflow(name) if f.kind in ("conv", "linear") and f.sources]


def _images(batch):
    if isinstance(batch, dict):
        return batch["image"]
    if isinstance(batch, (tuple, list)):
        return batch[0]
    return batch


def _split(S, c, device):
    """(S, its complement in range(c) in ascending order) as index tensors."""
    S = torch.as_tensor(np.asarray(S, dtype=np.int64), device=device)
    gone = torch.ones(c, dtype=torch.bool, device=device)
    gone[S] = False
    return S, torch.nonzero(gone).flatten()


def collect_moments(name, full, batches, compress_rate=None, chunk_bytes=256 << 20):
    """{module name: Moments(n, G)} of `full` (an nn.Module of architecture `name`) over `batches`.

    A forward pre-hook sits on every conv and linear module of transplant.dataflow(name) with sources - with
    compress_rate given, only on those whose input loses channels at these rates ({} where none does). It sees the
    module's real input, pooling, up-sampling, concatenation and DenseNet's bn-ReLU applied: channel i is channel i of
    the full net's tensor, the numbering transplant._channels speaks. Per batch n += N*H*W (N for a linear layer) and
    G += sum x x^T, in float64 on the input's device; the input is upcast and multiplied in runs of samples whose float64
    copy stays under chunk_bytes (one sample at least).

    batches yields input tensors, (x, y) pairs or {"image": x} dicts; each goes to the device and dtype of the net's
    parameters. The net runs in eval mode under no_grad; every module's training flag is put back and every hook
    removed, whatever happens."""
    wanted = _consumers(name)
    if compress_rate is not None:
        from . import nets
        slim = nets.get_network(name, compress_rate)
        width_in = {n: m.weight.size(1) for n, m in slim.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}
        wanted = [f for f in wanted if width_in[f.module] != full.get_submodule(f.module).weight.size(1)]
    if not wanted:
        return {}
    count, gram = {}, {}

    def hook_for(module):
        def hook(mod, inputs):
            x = inputs[0].detach()
            if x.dim() == 4:
                per_sample, cols = x[0].numel(), lambda run: run.transpose(0, 1).reshape(x.size(1), -1)
            else:
                x = x.reshape(-1, x.size(-1))
                per_sample, cols = x.size(1), lambda run: run.t()
            c = x.size(1)
            if module not in gram:
                count[module], gram[module] = 0, torch.zeros(c, c, dtype=torch.float64, device=x.device)
            step = max(1, int(chunk_bytes) // (8 * per_sample))
            for i in range(0, x.size(0), step):
                m = cols(x[i:i + step]).double()  # [C, positions of this run]
                gram[module].addmm_(m, m.t())
            count[module] += x.numel() // c
        return hook

    flags = [(m, m.training) for m in full.modules()]
    handles = []
    like = next(full.parameters())
    try:
        for f in wanted:
            handles.append(full.get_submodule(f.module).register_forward_pre_hook(hook_for(f.module)))
        full.eval()
        with torch.no_grad():
            for batch in batches:
                full(_images(batch).to(device=like.device, dtype=like.dtype))
    finally:
        for h in handles:
            h.remove()
        for m, flag in flags:
            m.training = flag
    return {module: Moments(count[module], gram[module]) for module in gram}


def merge_matrix(G, n, S, rtol=1e-10):
    """(A, residual): the least-squares map from the kept channels S to the removed ones D (the complement of S, ascending),
    x_D ~ A x_S, under the moments M = G / n.

    A = M_DS pinv(M_SS), [|D|, |S|], the pseudo-inverse by torch.linalg.pinv(hermitian=True, rtol=rtol): eigenvalues of
    M_SS below rtol times the largest count as zero, so dead and duplicated kept channels do no harm. residual =
    tr(M_DD - A M_SD) / tr(M_DD), the share of the removed channels' energy the fit leaves (0 where they have none)."""
    if G.dim() != 2 or G.size(0) != G.size(1):
        raise ValueError("a moment matrix is square, got shape %s" % (list(G.shape),))
    M = G.double() / float(n)
    S, D = _split(S, M.size(0), M.device)
    m_ds = M.index_select(0, D).index_select(1, S)
    m_ss = M.index_select(0, S).index_select(1, S)
    A = m_ds @ torch.linalg.pinv(m_ss, hermitian=True, rtol=rtol)
    total = float(M.diagonal().index_select(0, D).sum())
    left = total - float((A * m_ds).sum())  # tr(A M_SD) = sum_ij A_ij M_DS_ij
    return A, (max(left, 0.0) / total if total > 0 else 0.0)  # below 0 only by the round-off of the difference


def compensate(name, pruned, full, imp_score, moments, rtol=1e-10):
    """Fold the removed input channels of every consumer into the kept ones, in `pruned` (an nn.Module, as
    prune_network(..., carry=True) returns it), in place; returns [Merged] in table order.

    full: the full-width module or its state dict; imp_score: what prune_network was given, so that the kept lists
    (transplant.kept_filters) are the same; moments: collect_moments' dict. For every conv and linear module of
    transplant.dataflow(name) whose input lost channels, with S = transplant._channels(sources, kept), D its complement
    and A = merge_matrix(G, n, S, rtol)[0]:

        W'[:, S] = W[rows][:, S] + W[rows][:, D] A        (a conv: per tap)

    in float64, rounded once to pruned's dtype, on pruned's device; rows is the consumer's own kept list. Nothing else
    changes: no bias, no batch-norm tensor, no module whose input kept its channels.

    KeyError names a needed module that `moments` lacks, ValueError a G that is not [C_in, C_in]; n < |S| - fewer
    positions than unknowns per row of A - warns and goes on."""
    ori = full.state_dict() if isinstance(full, nn.Module) else full
    params = dict(pruned.named_parameters())
    kept = _tp.kept_filters(name, pruned.state_dict(), ori, imp_score)
    done = []
    with torch.no_grad():
        for f in _consumers(name):
            w = ori[f.module + ".weight"]
            S = _tp._channels(f.sources, kept)
            if len(S) == w.size(1):
                continue
            if f.module not in moments:
                raise KeyError("no moments for %s, whose input lost %d of %d channels" % (f.module, w.size(1) - len(S), w.size(1)))
            n, G = moments[f.module]
            if tuple(G.shape) != (w.size(1), w.size(1)):
                raise ValueError("%s reads %d channels, its moment matrix has shape %s" % (f.module, w.size(1), list(G.shape)))
            if n < len(S):
                warnings.warn("%s: %d positions for %d kept channels, the fit is under-determined" % (f.module, n, len(S)))
            A, residual = merge_matrix(G, n, S, rtol)
            target = params[f.module + ".weight"]
            w = w.to(device=target.device, dtype=torch.float64)
            if f.kind == "conv":
                w = _tp._rows(w, kept[f.module])
            s_idx, d_idx = _split(S, w.size(1), w.device)
            w_s, w_d = w.index_select(1, s_idx), w.index_select(1, d_idx)
            A = A.to(w.device)
            merged = w_s + (torch.einsum("odhw,ds->oshw", w_d, A) if w.dim() == 4 else w_d @ A)
            target.copy_(merged.to(target.dtype))
            done.append(Merged(f.module, int(n), len(S), w.size(1) - len(S), residual))
    return done
