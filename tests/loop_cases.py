"""Millions of maps checked against a float64 reference of a few hundred: the cases of the grid-loop tests.

A case is a BANK of B = 251 distinct maps (synth-style relu(randn) * scale; several all zero, one scaled by 1e4 and one
by 1e-4) and a seeded random index idx[nmaps] into it; the scored tensor is bank[idx], gathered on the device. What
every map must score is known from the bank alone:

  (a) the float64 oracle of the bank, indexed by idx, within the bound the entry point's own test module uses;
  (b) bit for bit what ONE small call on the bank itself gives, indexed by idx: 251 maps stay far below one grid, and
      the headers promise that a map's value depends on that map alone;
  and every scored entry is finite, exactly +0.0 for a zero bank map, in an output pre-filled with NaN whose 64-float
  guard is still NaN afterwards.

THE INDEX IS RANDOM, NOT PERIODIC. A wave that re-reads its first group on every iteration reads the map `stride` places
before the right one; with idx periodic in the stride it would read an equal map and pass. With a random index it reads
another bank map with probability 250 / 251 per map. tests/test_grid_loops_cpu.py pins both halves of that.

check_scores runs on whatever device its tensors are on: the GPU tests (tests/test_grid_loops_gpu.py) compare there and
bring one boolean back, the CPU self-check (tests/test_grid_loops_cpu.py) puts a numpy model of the grid-stride schedule
(schedule_sources, multi_sources) with the fp32 oracle in the library's place through the same function.
No product import: torch and numpy only.
"""
import numpy as np
import torch

B = 251                        # bank maps: a prime, so no power-of-two stride is a period of anything derived from it
ZERO_MAPS = (3, 64, 127, 250)  # all-zero bank maps (more where relu(randn) happens to give one, as at 2 x 2)
BIG_MAP, SMALL_MAP = 17, 190   # scaled by 1e4 and by 1e-4
GUARD = 64                     # floats after the scored output that must stay NaN
CHUNK_ELEMS = 1 << 25          # check_scores compares at most this many output elements at a time


def make_bank(h, w, seed, dtype=torch.float32):
    """[B, h, w] on the CPU. In fp16 the 1e4 map is brought to a peak of 1 first, so that it stays finite (65504)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(B, h, w, generator=g)) * torch.exp(0.5 * torch.randn(B, generator=g))[:, None, None]
    x[list(ZERO_MAPS)] = 0
    if dtype == torch.float16:
        x[BIG_MAP] /= x[BIG_MAP].max().clamp_min(1.0)
    x[BIG_MAP] *= 1e4
    x[SMALL_MAP] *= 1e-4
    return x.to(dtype)


def make_rank_bank(h, w, seed):
    """[B, h, w] fp32 maps of KNOWN rank: map i is an exact small-integer product U V of rank 1 + (5 i) % min(h, w) times
    a power of two (far_views.make_maps' construction), so full-rank and rank-deficient maps alternate; ZERO_MAPS are zero."""
    out = np.zeros((B, h, w), np.float32)
    n = min(h, w)
    for i in range(B):
        if i in ZERO_MAPS:
            continue
        g = np.random.default_rng((seed, i))
        r = 1 + (5 * i) % n
        u, v = g.integers(-1, 2, (h, r)).astype(np.float64), g.integers(-1, 2, (r, w)).astype(np.float64)
        u[:r] += 16.0 * np.eye(r)
        v[:, :r] += 16.0 * np.eye(r)
        out[i] = (u @ v) * 2.0 ** int(g.integers(-3, 4))
    return torch.from_numpy(out)


def known_ranks(h, w):
    n = min(h, w)
    return torch.tensor([0.0 if i in ZERO_MAPS else 1.0 + (5 * i) % n for i in range(B)])


def random_index(nmaps, seed, device="cpu"):
    """The seeded random index of a case, generated on `device`."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(B, (nmaps,), generator=g, device=device)


def periodic_index(nmaps, period, seed, device="cpu"):
    """What the cases must NOT use: an index that repeats every `period` maps."""
    return random_index(period, seed, device)[torch.arange(nmaps, device=device) % period]


def guarded(nmaps, per_map, device):
    """(buffer, scored view [nmaps * per_map]): NaN everywhere, GUARD floats behind the scored part."""
    buf = torch.full((nmaps * per_map + GUARD,), float("nan"), dtype=torch.float32, device=device)
    return buf, buf[:nmaps * per_map]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _fail(what, msg, m, group, units):
    where = "map %d" % m
    if group:
        grp = m // group
        where += " (group %d" % grp + (", iteration %d of wave %d)" % (grp // units, grp % units) if units else ")")
    raise AssertionError("%s: %s %s" % (what, where, msg))


def check_scores(got, idx, ref64, twin, tol, denom64=None, guard=None, what="case", group=0, units=0, signed_zero=False):
    """got [nmaps, ...] fp32 scores of bank[idx]; ref64 [B, ...] float64 and twin [B, ...] fp32 (the small call on the
    bank); every |got - ref64[idx]| <= tol * denom64[idx] (denom64 [B]: default |ref64| itself), zero bank maps (denom
    == 0) exactly +0.0, every entry finite, got bitwise twin[idx], guard all NaN. Returns the worst relative error.
    twin=None leaves (b) out, tol=None leaves (a) and the +0.0 test out (the CPU self-check shows that each catches a mutant alone).
    signed_zero=True is for COEFFICIENTS, not scores: the headers promise +0.0 for the energy, band energies and rank of
    an all-zero map, while a coefficient of one is a difference or a product with a negative constant of the
    factorised transform and may be -0.0; there a zero bank map must give zeros of either sign (and the twin's bits).
    group / units (maps per group, waves of the grid) only name the failing map's place in the schedule."""
    nmaps = idx.shape[0]
    assert got.shape[0] == nmaps and got.shape[1:] == ref64.shape[1:], (got.shape, ref64.shape)
    assert twin is None or (twin.shape == ref64.shape and twin.dtype == torch.float32)
    assert got.dtype == torch.float32 and ref64.dtype == torch.float64
    per = max(1, int(np.prod(got.shape[1:])))
    extra = (1,) * (got.dim() - 1)
    denom = (ref64.abs() if denom64 is None else denom64.reshape((B,) + extra).expand_as(ref64)).contiguous()
    zero_map = (denom.reshape(B, -1) == 0).all(dim=1)
    worst = 0.0
    step = max(1, CHUNK_ELEMS // per)
    for lo in range(0, nmaps, step):
        g, i = got[lo:lo + step], idx[lo:lo + step]
        fin = torch.isfinite(g)
        if not bool(fin.all()):
            m = lo + int((~fin).reshape(len(i), -1).any(dim=1).nonzero()[0])
            _fail(what, "was not written or is not finite: %r" % got[m].reshape(-1)[:4].tolist(), m, group, units)
        z = zero_map[i]
        nonzero = (g != 0) if signed_zero else (_bits(g) != 0)
        if tol is not None and bool(z.any()) and bool(nonzero[z].any()):
            m = lo + int((z & nonzero.reshape(len(i), -1).any(dim=1)).nonzero()[0])
            _fail(what, "is a zero bank map and scores %r, expected %s" % (got[m].reshape(-1)[:4].tolist(), "zeros" if signed_zero else "+0.0"),
                  m, group, units)
        t = g if twin is None else twin[i]
        if not torch.equal(_bits(g), _bits(t)):
            m = lo + int((_bits(g) != _bits(t)).reshape(len(i), -1).any(dim=1).nonzero()[0])
            _fail(what, "(bank map %d) scores %r, the call on the bank alone gives %r"
                  % (int(idx[m]), got[m].reshape(-1)[:4].tolist(), twin[idx[m]].reshape(-1)[:4].tolist()), m, group, units)
        err = (g.double() - ref64[i]).abs()
        d = denom[i]
        bad = ~(err <= tol * d) if tol is not None else torch.zeros_like(err, dtype=torch.bool)
        if bool(bad.any()):
            m = lo + int(bad.reshape(len(i), -1).any(dim=1).nonzero()[0])
            _fail(what, "(bank map %d) scores %r, float64 gives %r: beyond %.3g relative"
                  % (int(idx[m]), got[m].reshape(-1)[:4].tolist(), ref64[idx[m]].reshape(-1)[:4].tolist(), tol), m, group, units)
        live = d > 0
        if bool(live.any()):
            worst = max(worst, float((err[live] / d[live]).max()))
    if guard is not None:
        assert guard.numel() == GUARD and bool(torch.isnan(guard).all()), "%s: the guard behind the output was written" % what
    return worst


# ----------------------------------------------------------------------------------------------------
# the numpy model of the grid-stride schedule (tests/test_grid_loops_cpu.py)
# ----------------------------------------------------------------------------------------------------
MUTANTS = ("once", "reread_first", "short_stride", "drop_ragged", "fence_leak")
MULTI_MUTANTS = ("t_stuck", "t_one_step")


def schedule_sources(nmaps, G, units, wg_waves=1, mutant=None):
    """src[m]: the position in the scored tensor whose map a capped grid of `units` waves (workgroups of wg_waves), each
    taking groups of G maps with `for (grp = wave; grp < ngroups; grp += units)`, scores into out[m]; -1 where out[m] is
    never written. mutant=None is the schedule of the kernels. The mutants:
      once           the loop body runs once
      reread_first   every iteration reads the wave's first group (and writes the right outputs)
      short_stride   the read position advances by a stride one workgroup short (an incremented pointer), the output
                     index by the right one
      drop_ragged    the last group is skipped when it is ragged
      fence_leak     the missing-fence picture: the odd maps of a group (the map, where a group is one) come out as those of the wave's NEXT group"""
    assert mutant is None or mutant in MUTANTS
    ngroups = -(-nmaps // G)
    src = np.full(nmaps, -1, np.int64)
    for wave in range(min(units, ngroups)):
        for it, grp in enumerate(range(wave, ngroups, units)):
            if mutant == "once" and it > 0:
                break
            lo, hi = grp * G, min(nmaps, (grp + 1) * G)
            if mutant == "drop_ragged" and hi - lo < G:
                continue
            m = np.arange(lo, hi)
            read = m
            if mutant == "reread_first":
                read = m - it * units * G
            elif mutant == "short_stride":
                read = m - it * wg_waves * G
            elif mutant == "fence_leak" and grp + units < ngroups:
                nxt = np.minimum(m + units * G, nmaps - 1)
                read = np.where((m - lo) % 2 == (1 if G > 1 else 0), nxt, m)
            src[m] = read
    return src


def multi_layout(sizes, G):
    """group_begin of every tensor and the total, as the multi-tensor descriptors hold them."""
    begin, total = [], 0
    for s in sizes:
        begin.append(total)
        total += -(-s // G)
    return begin, total


def multi_sources(sizes, G, units, mutant=None):
    """One src array per tensor (positions in that tensor, -1 = never written) for the walk of k_energy_codelet_multi:
    `while (t + 1 < count && grp >= begin[t + 1]) ++t` carried from one iteration to the next. The mutants:
      t_stuck      t is found for the wave's first group and never advances afterwards
      t_one_step   t advances by at most one tensor per iteration
    A group whose local index lies beyond its (wrong) tensor stores nothing, as the kernels' m < nmaps test has it."""
    assert mutant is None or mutant in MULTI_MUTANTS
    begin, total = multi_layout(sizes, G)
    srcs = [np.full(s, -1, np.int64) for s in sizes]
    for wave in range(min(units, total)):
        t = 0
        for it, grp in enumerate(range(wave, total, units)):
            true_t = max(i for i in range(len(sizes)) if begin[i] <= grp)
            if mutant is None or it == 0:
                t = true_t
            elif mutant == "t_one_step":
                t = min(true_t, t + 1)
            local = grp - begin[t]
            lo, hi = local * G, min(sizes[t], (local + 1) * G)
            if lo < hi:
                srcs[t][lo:hi] = np.arange(lo, hi)
    return srcs


def model_scores(src, idx, bank_scores):
    """What the modelled launch leaves in a NaN-filled output: bank_scores[idx[src[m]]], NaN where src[m] < 0."""
    s = torch.from_numpy(src)
    out = bank_scores[idx[s.clamp_min(0)]].clone()
    out[s < 0] = float("nan")
    return out


# ----------------------------------------------------------------------------------------------------
# sizes of the multi-tensor cases
# ----------------------------------------------------------------------------------------------------
def multi_sizes(total_maps, count=44, runs=((5, 4), (17, 3), (30, 5))):
    """Maps per tensor of a multi-tensor case: `count` tensors (more than kMultiItems = 32 and close to kMixedItems = 48,
    so the calls' chunking is crossed) from 1 map to a quarter of the total; runs of 1-map tensors (start, length) sit
    between large ones, so that a wave's next group lies two or more tensors ahead. Sums to total_maps exactly."""
    sizes = [0] * count
    tiny = {i for start, length in runs for i in range(start, start + length)}
    for i in tiny:
        sizes[i] = 1
    big = [i for i in range(count) if i not in tiny]
    left = total_maps - len(tiny)
    sizes[big[0]] = total_maps // 4                # a quarter of the total
    left -= sizes[big[0]]
    weights = [1 + (7 * k) % 5 for k in range(len(big) - 1)]
    for k, i in enumerate(big[1:]):
        sizes[i] = max(2, left * weights[k] // sum(weights))
    sizes[big[1]] += total_maps - sum(sizes)       # what the rounding left over
    assert sum(sizes) == total_maps and min(sizes) >= 1 and max(sizes) == total_maps // 4, (total_maps, sizes)
    return sizes
