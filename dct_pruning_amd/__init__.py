"""dct_pruning_amd — MI355X-native DCT importance-score path of semchan/DCT_Pruning.

Scope: forward-hooked feature maps [N,C,H,W] -> per-map orthonormal 2-D
DCT-II -> sum of squared coefficients -> per-channel running mean -> .npy score files
(reference: utils/common.py:230-309 and :367-977). The arithmetic runs in hand-written
gfx950 HIP kernels behind the C ABI of include/dctscore.h; this package is the host-side
mirror of the reference's hook / imp_score interface. A second criterion, the HRank feature-map
rank (rank_nc, imp_score(criterion="rank")), shares everything above the kernel, and so does a third, the per-band
DCT energy spectrum (band_energy_nc, imp_score(criterion="bands"), bands.py: K frequency bands per map in one pass),
and a fourth, the spectral entropy of the DCT coefficients (spectral_entropy_nc, imp_score(criterion="entropy")): one
number per map that does depend on the transform. A fifth looks at more than one map at a time: the summed distance of
every map to the other maps of its layer (gm_distance_nc, imp_score(criterion="gm")), FPGM's geometric-median rule on feature maps;
its terms, the [C, C] matrix of pair distances per layer (gm_pair_matrix, imp_score(criterion="gm", gm_pairs=True)), feed the
host-side selection rules of pairs.py (row sum, nearest neighbour, farthest point). With lowpass=K both compare the maps' K x K
lowest DCT coefficients (lowpass_nc, imp_score(criterion="gm", gm_lowpass=K)): the one form of that distance the transform changes.
"""
from .ops import (  # noqa: F401
    ALGO_AUTO,
    ALGO_CODELET,
    ALGO_DIRECT,
    ALGO_FUSED,
    ALGO_PIPE,
    ALGO_LANE,
    ALGO_PREFETCH,
    ALGO_SPLIT,
    ALGO_TILE2D,
    ALGO_RECT,
    band_energy_nc,
    batch_sum,
    dct2d,
    energy_mixed,
    energy_multi,
    energy_nc,
    gm_distance_nc,
    gm_pair_matrix,
    has_band_kernel,
    has_codelet,
    has_entropy_kernel,
    has_half_kernel,
    has_nhwc_kernel,
    lowpass_nc,
    rank_nc,
    spectral_entropy_nc,
    weighted_energy_nc,
)

__all__ = ["energy_nc", "energy_multi", "energy_mixed", "dct2d", "batch_sum", "has_codelet", "weighted_energy_nc", "rank_nc", "band_energy_nc", "has_band_kernel", "has_half_kernel", "has_nhwc_kernel", "spectral_entropy_nc", "has_entropy_kernel", "gm_distance_nc", "gm_pair_matrix", "lowpass_nc", "ALGO_AUTO", "ALGO_DIRECT", "ALGO_CODELET", "ALGO_SPLIT", "ALGO_PREFETCH", "ALGO_FUSED", "ALGO_PIPE", "ALGO_LANE", "ALGO_TILE2D", "ALGO_RECT"]
