"""CPU fp64 oracle of the rank criterion (dcts_rank_f32): the singular values of the fp32 map, taken in fp64, and
the rule of torch.linalg.matrix_rank for fp32, rank = #{sigma_i > max(H, W) * 2^-23 * sigma_max}; an all-zero map
has rank 0. Test infrastructure only."""
import torch

EPS32 = 2.0 ** -23


def _svals(x, c_begin, c_count):
    x = x.detach().cpu()
    if c_count is None:
        c_count = x.shape[1] - c_begin
    a = x[:, c_begin:c_begin + c_count].double()
    s = torch.linalg.svdvals(a)  # [N, c, min(H, W)], descending
    tau = max(x.shape[2], x.shape[3]) * EPS32 * s[..., :1]
    return s, tau


def rank_nc(x, c_begin=0, c_count=None):
    """[N, c_count] fp32 ranks, the signature of ops.rank_nc (drop-in for harness._rank_nc)."""
    s, tau = _svals(x, c_begin, c_count)
    return (s > tau).sum(-1).to(torch.float32)


def undecidable(x, c_begin=0, c_count=None, band=1.5):
    """[N, c_count] bool: some sigma lies in [tau / band, band * tau], where fp32 round-off of the map's producer
    (or any fp64 method's own error, far smaller) could decide the comparison either way. All-zero maps are
    decidable."""
    s, tau = _svals(x, c_begin, c_count)
    near = (s >= tau / band) & (s <= tau * band) & (tau > 0)
    return near.any(-1)


def hrank_hook_scores(acts, c_begin=0, c_count=None):
    """HRank's hook body restated literally over a list of hooked batches: a per-map loop of ranks,
    c.view(a, -1).float().sum(0), then the running mean of utils/common.py:271-277."""
    feature_result = torch.tensor(0.)
    total = torch.tensor(0.)
    for output in acts:
        a = output.shape[0]
        b = output.shape[1]
        lo = c_begin if c_count is not None else 0
        hi = lo + c_count if c_count is not None else b
        c = torch.tensor([rank_nc(output[i:i + 1, j:j + 1])[0, 0].item() for i in range(a) for j in range(lo, hi)])
        c = c.view(a, -1).float()
        c = c.sum(0)
        feature_result = feature_result * total + c
        total = total + a
        feature_result = feature_result / total
    return feature_result.numpy()
