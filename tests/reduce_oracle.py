"""The batch sum and the running-mean update of reduce.hip (k_batch_sum, k_running_mean, k_running_mean_multi) as an exact
fp32 model in numpy: the order and the roundings that include/dctscore.h and DESIGN.md section 4.5 state, so that the
kernels are compared on bits, without a tolerance.

  batch sum     16 interleaved slices; slice s starts at +0.0f and adds e[n] for n = s, s+16, ... ascending, one fp32
                rounding per add; t starts at +0.0f and adds the 16 partials in slice order. A slice without samples
                (N < 16) contributes +0.0, so a column of -0.0 gives +0.0.
  running mean  fr <- f32(f32(f32(fr * total) + t) / f32(total + N)): three roundings on the value, no fused multiply-add,
                a division and not a multiplication by the reciprocal.

Every operation below is a numpy float32 op on float32 operands, which rounds once to nearest-even as the device's
v_add_f32 / v_mul_f32 and the correctly rounded division do. rule_f64 is the same rule in float64, for the bounds.
The mutants are what tests/test_reduce_cpu.py shows a bitwise comparison to catch, each a fault the kernels could have.
"""
import numpy as np

SLICES = 16  # kSumSl of reduce.hip

# the sample counts of tests/test_reduce_gpu.py: around the slice count, around the 64-sample (4 x 16) and the 256-sample
# (16 x 16) loop tiers of strip_batch_sum and their sums (272 = 256 + 16, 320 = 256 + 64), odd N mod 16, several trips (4099)
NS = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 79, 250, 255, 256, 257, 271, 272, 319, 320, 321, 777, 1000, 4099)
# channel counts: around the 32-channel strip, two strips, many blocks with a ragged last strip
CS = (1, 31, 32, 33, 37, 64, 65, 2049)
TOTALS = (0, 5, 261, 1000, 16777216)
WIDE = (17, 70001)


def energies(N, C, seed):
    """exp(normal(0, 2)) as float32: non-negative like real energies, about 12 binades wide."""
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(0.0, 2.0, size=(N, C))).astype(np.float32)


def feature_result(C, seed, total_before, N):
    """A random positive feature_result for an update by N samples after total_before: energies scaled by N / total_before,
    so that fr * total and the batch sum are of one magnitude. A product far below the sum hides how it was rounded (at
    fr ~ e, total 5 and N = 256 a fused multiply-add differs from the rule in under 1 % of the columns); here neither term
    hides the other, which is where a contracted update shows in the most columns."""
    fr = energies(1, C, seed)[0]
    return fr * np.float32(N / total_before) if total_before else fr


def _f32(e):
    e = np.asarray(e)
    assert e.dtype == np.float32 and e.ndim == 2, (e.dtype, e.shape)
    return e


def _sliced_sum(e, slices, descending=False):
    N, C = e.shape
    part = np.zeros((slices, C), np.float32)
    for n in range(N):
        part[n % slices] += e[n]
    t = np.zeros(C, np.float32)
    for s in (range(slices - 1, -1, -1) if descending else range(slices)):
        t += part[s]
    return t


def batch_sum_model(e):
    """[N, C] float32 -> the [C] float32 that dcts_batch_sum_f32 must produce, bit for bit."""
    return _sliced_sum(_f32(e), SLICES)


def running_mean_model(fr, total_before, e):
    """The [C] float32 that dcts_running_mean_update_f32 must leave in feature_result."""
    e = _f32(e)
    fr = np.asarray(fr)
    assert fr.dtype == np.float32 and fr.shape == (e.shape[1],)
    total = np.float32(total_before)
    den = np.float32(total + np.float32(e.shape[0]))
    prod = fr * total
    acc = prod + batch_sum_model(e)
    assert prod.dtype == acc.dtype == np.float32
    return acc / den


def chain_model(batches, C):
    """feature_result after the updates of `batches` (a list of [N_i, C] float32), starting from zeros and total 0; the
    total is kept as the accumulators keep it: an exact count, rounded to float32 when it is passed."""
    fr, total = np.zeros(C, np.float32), 0
    for e in batches:
        fr = running_mean_model(fr, total, e)
        total += e.shape[0]
    return fr


def rule_f64(batches):
    """The same update rule in float64 over a list of [N_i, C] batches, from zeros."""
    fr, total = np.zeros(batches[0].shape[1], np.float64), 0.0
    for e in batches:
        fr = (fr * total + np.asarray(e, np.float64).sum(0)) / (total + e.shape[0])
        total += e.shape[0]
    return fr


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- mutants ----------------------------------------------------------------------------------------------------------
def _ascending(e):
    return _sliced_sum(e, 1)


def _sum_with_repeat(e, k):
    """The 16-slice sum in which sample k is added twice, in its own slice, right after its first occurrence."""
    N, C = e.shape
    part = np.zeros((SLICES, C), np.float32)
    for n in range(N):
        part[n % SLICES] += e[n]
        if n == k:
            part[n % SLICES] += e[n]
    t = np.zeros(C, np.float32)
    for s in range(SLICES):
        t += part[s]
    return t


SUM_MUTANTS = {
    "ascending": _ascending,
    "8-slices": lambda e: _sliced_sum(e, 8),
    "32-slices": lambda e: _sliced_sum(e, 32),
    "descending-combine": lambda e: _sliced_sum(e, SLICES, descending=True),
    "last-dropped": lambda e: _sliced_sum(e[:-1], SLICES),
    "256-doubled": lambda e: _sum_with_repeat(e, 256),
}
# the order mutants that are the model itself up to N = 16: one sample per slice at most, and +0.0 + x is x
EQUAL_UP_TO_16 = ("ascending", "32-slices")


def _mean_single_rounding(fr, total_before, e):
    total = np.float32(total_before)
    den = np.float32(total + np.float32(e.shape[0]))
    acc = (fr.astype(np.float64) * np.float64(total) + batch_sum_model(e).astype(np.float64)).astype(np.float32)
    return acc / den


def _mean_reciprocal(fr, total_before, e):
    total = np.float32(total_before)
    den = np.float32(total + np.float32(e.shape[0]))
    acc = fr * total + batch_sum_model(e)
    return acc * (np.float32(1) / den)


MEAN_MUTANTS = {"single-rounding": _mean_single_rounding, "reciprocal": _mean_reciprocal}
