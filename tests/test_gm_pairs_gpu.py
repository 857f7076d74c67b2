"""dcts_gm_pairs_f32 on the GPU against the float64 definition of tests/gm_pairs_oracle.py, at the tolerances derived there
(TOL = 8 R, R the fp32 restatement's own error on these inputs): shapes on both sides of every tile edge under the three
metrics, the three slice regimes (bit for bit against the restatement's order on maps whose squared distances are exact),
what the difference form makes exact, independence of the scored range and of the alignment bit for bit, views, the extent of
what is written, a poisoned map, the row sums against dcts_gm_distance_f32, the selection the matrix is for, and the
accumulator forms end to end."""
import functools

import numpy as np
import pytest
import torch

import dct_pruning_amd as dpa
import gm_oracle as go
import gm_pairs_oracle as po
import loop_cases as lc
from dct_pruning_amd import _lib, harness, pairs

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {"l2": 0, "cosine": 1, "correlation": 2}


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _reference(name, metric):
    """The float64 definition of a named input of gm_pairs_oracle.gpu_inputs(), computed once."""
    for nm, x, ranges in po.gpu_inputs():
        if nm == name:
            return x, ranges, po.pair_matrix_f64(x, metric, *ranges), po.exact_zeros(x, metric, ranges)
    raise KeyError(name)


def _check(got, name, metric):
    """got [c, r] float32 on the device against the definition: within TOL, +0.0 where it must be 0."""
    x, ranges, ref, zeros = _reference(name, metric)
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == ref.shape, (name, g.shape, ref.shape)
    assert np.isfinite(g).all(), name
    err = po.error(g, ref, metric, x.shape[0], zeros)
    print("GM_PAIRS %s %s error = %.3e (tol %.3e)" % (metric, name, err, po.TOL[metric]))
    assert err <= po.TOL[metric], (name, metric, err)
    assert (g[zeros].view(np.int32) == 0).all(), name  # +0.0, the sign bit too
    return x, g


# ----------------------------------------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", po.METRICS)
@pytest.mark.parametrize("c,hw", po.SWEEP, ids=["C%d-%dx%d" % (c, hw[0], hw[1]) for c, hw in po.SWEEP])
def test_shape_sweep(c, hw, metric):
    name = "C=%d %dx%d" % (c, hw[0], hw[1])
    xd = _reference(name, metric)[0].to(DEV)
    got = dpa.gm_pair_matrix(xd, metric=metric)
    assert got.shape == (c, c)
    _check(got, name, metric)
    assert torch.equal(_bits(got), _bits(dpa.gm_pair_matrix(xd, metric=metric)))  # repeated call
    assert torch.equal(_bits(got), _bits(got.t()))  # out[j, k] and out[k, j]: the same bits
    assert (_bits(torch.diagonal(got)) == 0).all()  # a channel with itself: +0.0
    if c >= 2:  # the duplicated channel: at +0.0 from its twin, and their rows are the same bits
        assert int(_bits(got[0, c - 1])) == 0 and torch.equal(_bits(got[0]), _bits(got[c - 1]))
    if (c, hw) == po.ZERO_SAMPLE_CASE:  # sample 1 is all zeros and adds +0.0 to every entry
        x = _reference(name, metric)[0]
        rest = dpa.gm_pair_matrix(x[[0, 2]].to(DEV), metric=metric)
        np.testing.assert_allclose(got.cpu().numpy(), rest.cpu().numpy(), rtol=1e-6, atol=0)


# ----------------------------------------------------------------------------------------------------
# the slice regimes
# ----------------------------------------------------------------------------------------------------
def test_the_three_slice_regimes_are_the_ones_tested():
    lib = _lib.load()
    seen = set()
    for name, n, c, hw in po.REGIMES:
        s = lib.dcts_gm_pairs_slices(n, c)
        assert s == po.slices(n, c) and tuple(po.regime_case(name).shape) == (n, c) + hw
        per = -(-n // s)
        if s == n and n > 1:
            seen.add("S=N")
        elif 1 < s < n and n - (s - 1) * per < per:
            seen.add("ragged")
        elif s == 1 and n > 1:
            seen.add("S=1")
    assert seen == {"S=N", "ragged", "S=1"} == {r[0] for r in po.REGIMES}


@pytest.mark.parametrize("metric", po.METRICS)
@pytest.mark.parametrize("name", [r[0] for r in po.REGIMES])
def test_slice_regime_against_float64(name, metric):
    xd = _reference(name, metric)[0].to(DEV)
    got = dpa.gm_pair_matrix(xd, metric=metric)
    _check(got, name, metric)
    assert torch.equal(_bits(got), _bits(got.t()))


@pytest.mark.parametrize("name", [r[0] for r in po.REGIMES])
def test_slice_order_bit_for_bit_on_exact_maps(name):
    """Small-integer maps: every squared distance is an integer, exact in fp32 whatever the order over p, and sqrt is correctly
    rounded on both sides. What is left is the order of the additions over the samples: n ascending within a slice, the
    slices ascending. One slice for all samples (or any other cut) gives other bits where the sums round."""
    x = po.integer_case(name)
    got = dpa.gm_pair_matrix(x.to(DEV)).cpu().numpy()
    want = po.pair_matrix_f32(x)
    assert got.tobytes() == want.tobytes()
    if name == "ragged":
        assert want.tobytes() != po.pair_matrix_f32(x, bounds=[(0, x.shape[0])]).tobytes()  # the order is visible here


# ----------------------------------------------------------------------------------------------------
# exactness
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", po.METRICS)
@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (8, 8)], ids=lambda s: "%dx%d" % s)
def test_identical_maps_and_all_zero_tensors_give_plus_zero(hw, metric):
    x = go.maps(3, 2, hw[0], hw[1], 31)  # C = 2: channel 1 is channel 0
    assert torch.equal(x[:, 0], x[:, 1]) and (x != 0).any()
    got = dpa.gm_pair_matrix(x.to(DEV), metric=metric)
    assert got.shape == (2, 2) and (_bits(got) == 0).all()
    for n, c in ((2, 70), (5, 3), (1, 130)):  # one slice per sample, several slices, one sample
        assert (_bits(dpa.gm_pair_matrix(torch.zeros(n, c, hw[0], hw[1], device=DEV), metric=metric)) == 0).all()


@pytest.mark.parametrize("metric", ["cosine", "correlation"])
def test_power_of_two_multiples_and_flat_maps_under_a_metric(metric):
    x = go.maps(4, 70, 5, 7, 11)  # channel 1 zero, channel 69 a copy of channel 0
    x[:, 3] = x[:, 2] * 2.0 ** 10
    x[:, 66] = x[:, 2] * 2.0 ** -9
    x[:, 5] = 0.1 if metric == "correlation" else 0.0  # flat: a constant map under the correlation, zeros under the cosine
    got = dpa.gm_pair_matrix(x.to(DEV), metric=metric)
    for j, k in ((2, 3), (2, 66), (3, 66), (0, 69), (1, 5)):  # multiples across tiles, the copy, two flat maps
        assert int(_bits(got[j, k])) == 0 and int(_bits(got[k, j])) == 0, (j, k)
    assert torch.equal(_bits(got[2]), _bits(got[3])) and torch.equal(_bits(got[2]), _bits(got[66]))
    assert torch.equal(_bits(got[1]), _bits(got[5]))  # a zero map and a flat map are the same unit map
    # a flat map is at distance 1 from every map that is not flat: N per entry
    live = [k for k in range(70) if k not in (1, 5)]
    np.testing.assert_allclose(got[1, live].cpu().numpy(), 4.0, rtol=1e-6)
    ref = po.pair_matrix_f64(x, metric)
    assert po.error(got.cpu().numpy(), ref, metric, 4, po.exact_zeros(x, metric)) <= po.TOL[metric]


@pytest.mark.parametrize("metric", po.METRICS)
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_poisoned_map_reaches_its_own_row_and_column_only(poison, metric):
    x = go.maps(3, 70, 7, 7, 42).to(DEV)
    clean = dpa.gm_pair_matrix(x, metric=metric)
    y = x.clone()
    y[1, 66, 3, 1] = poison
    got = dpa.gm_pair_matrix(y, metric=metric)
    keep = [k for k in range(70) if k != 66]
    assert torch.equal(_bits(got[keep][:, keep]), _bits(clean[keep][:, keep]))
    assert not bool(torch.isfinite(got[66]).any()) and not bool(torch.isfinite(got[:, 66]).any())


# ----------------------------------------------------------------------------------------------------
# independence, bit for bit
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", po.METRICS)
def test_channel_range_pieces_are_rows_of_the_unsplit_call(metric):
    xd = _reference("pieces", metric)[0].to(DEV)
    full = dpa.gm_pair_matrix(xd, metric=metric)
    _check(full, "pieces", metric)
    for cb, cc in ((1, 1), (7, 1), (3, 5), (65, 5), (1, 37), (39, 37), (63, 2)):
        piece = dpa.gm_pair_matrix(xd, c_begin=cb, c_count=cc, metric=metric)  # against the full reference set
        assert piece.shape == (cc, 77) and torch.equal(_bits(piece), _bits(full[cb:cb + cc])), (cb, cc)
    cuts = (0, 1, 6, 43, 77)
    cat = torch.cat([dpa.gm_pair_matrix(xd, c_begin=a, c_count=b - a, metric=metric) for a, b in zip(cuts, cuts[1:])], dim=0)
    assert torch.equal(_bits(cat), _bits(full))
    # a reference range that does not start at 0: the entries are those of the same pairs (an entry knows no position)
    sub = dpa.gm_pair_matrix(xd, c_begin=2, c_count=70, ref_begin=9, ref_count=66, metric=metric)
    assert lib_slices(4, 66) == lib_slices(4, 77) and torch.equal(_bits(sub), _bits(full[2:72, 9:75]))


def lib_slices(n, r):
    return _lib.load().dcts_gm_pairs_slices(n, r)


@pytest.mark.parametrize("metric", po.METRICS)
def test_scored_and_reference_ranges_that_differ(metric):
    x, ranges, _, _ = _reference("subrange", metric)
    xd = x.to(DEV)
    got = dpa.gm_pair_matrix(xd, c_begin=ranges[0], c_count=ranges[1], ref_begin=ranges[2], ref_count=ranges[3], metric=metric)
    assert got.shape == (40, 62)
    _check(got, "subrange", metric)
    # the transposed call: the same pairs, the same bits
    back = dpa.gm_pair_matrix(xd, c_begin=ranges[2], c_count=ranges[3], ref_begin=ranges[0], ref_count=ranges[1], metric=metric)
    assert torch.equal(_bits(back.t()), _bits(got))
    # the same maps as a tensor of their own
    own = torch.cat([xd[:, 5:45], xd[:, 3:65]], dim=1).contiguous()
    twin = dpa.gm_pair_matrix(own, c_begin=0, c_count=40, ref_begin=40, ref_count=62, metric=metric)
    assert torch.equal(_bits(twin), _bits(got))


# ----------------------------------------------------------------------------------------------------
# load paths, views
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", po.METRICS)
@pytest.mark.parametrize("hw", [(6, 6), (7, 7)], ids=lambda s: "%dx%d" % s)
def test_views_and_load_paths_give_the_bits_of_an_aligned_contiguous_copy(hw, metric):
    """h * w = 36 takes the 16-byte loads on an aligned dense tensor, 49 the dword loads; a base offset by one float takes the
    dword loads in both. No view may differ from the aligned copy by a bit."""
    h, w = hw
    name = "views %dx%d" % hw
    xd = _reference(name, metric)[0].to(DEV)
    assert xd.data_ptr() % 16 == 0
    base = dpa.gm_pair_matrix(xd, metric=metric)
    _check(base, name, metric)
    # a base that is 4-byte but not 16-byte aligned: the aligned twin's bits
    flat = torch.zeros(xd.numel() + 4, device=DEV)
    assert flat.data_ptr() % 16 == 0
    off = flat[1:1 + xd.numel()].view(xd.shape)
    off.copy_(xd)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    assert torch.equal(_bits(dpa.gm_pair_matrix(off, metric=metric)), _bits(base))
    # a sample-strided view: the matrix of the samples it holds
    v = xd[::2]
    assert not v.is_contiguous()
    assert torch.equal(_bits(dpa.gm_pair_matrix(v, metric=metric)), _bits(dpa.gm_pair_matrix(xd[::2].contiguous(), metric=metric)))
    # a channel-sliced view of a wider tensor: strideC unchanged, nothing is copied
    wide = torch.full((4, 30, h, w), 3.0, device=DEV)
    wide[:, 4:25] = xd
    sl = wide[:, 4:25]
    assert sl.stride(1) == h * w and sl.stride(0) == 30 * h * w and not sl.is_contiguous()
    assert torch.equal(_bits(dpa.gm_pair_matrix(sl, metric=metric)), _bits(base))
    assert torch.equal(_bits(dpa.gm_pair_matrix(wide, c_begin=4, c_count=21, ref_begin=4, ref_count=21, metric=metric)), _bits(base))
    # a row-pitched view goes through the operator's copy; the C entry refuses the pitch
    pitched = torch.full((4, 21, h, w + 3), 3.0, device=DEV)
    pitched[..., :w] = xd
    pv = pitched[..., :w]
    assert torch.equal(_bits(dpa.gm_pair_matrix(pv, metric=metric)), _bits(base))
    out = torch.empty(21, 21, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    rc = _lib.load().dcts_gm_pairs_f32(pv.data_ptr(), 4, 21, h, w, pv.stride(0), pv.stride(1), pv.stride(2), 1, 0, 21, 0, 21,
                                       out.data_ptr(), torch.cuda.current_stream().cuda_stream, CODE[metric], ws.data_ptr(), ws.numel())
    assert rc == -6


# ----------------------------------------------------------------------------------------------------
# what is written
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", po.METRICS)
@pytest.mark.parametrize("n,c,cb,cc", [(3, 70, 0, 70), (3, 70, 3, 65), (2, 12, 5, 1), (1, 130, 0, 130)], ids=["full", "piece", "one", "S1"])
def test_guard_words_around_the_output_and_the_workspace(n, c, cb, cc, metric):
    lib = _lib.load()
    x = go.maps(n, c, 7, 9, 41).to(DEV)
    want = dpa.gm_pair_matrix(x, c_begin=cb, c_count=cc, metric=metric)
    need = lib.dcts_gm_pairs_workspace_bytes(CODE[metric], n, cc, c)
    assert (need == 0) == (metric == "l2" and lib.dcts_gm_pairs_slices(n, c) == 1)
    front = 64
    obuf = torch.full((front + cc * c + lc.GUARD,), float("nan"), device=DEV)
    out = obuf[front:front + cc * c].view(cc, c)
    wbuf = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wbuf[256:256 + need]
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes):
        return lib.dcts_gm_pairs_f32(x.data_ptr(), n, c, 7, 9, x.stride(0), x.stride(1), 9, 1, cb, cc, 0, c, out.data_ptr(), stream,
                                     CODE[metric], ws.data_ptr() if need else None, nbytes)

    if need:  # one byte short: the error, and nothing is launched
        assert call(need - 1) == -5
        torch.cuda.synchronize()
        assert bool(torch.isnan(obuf).all()) and bool((wbuf == 0xA5).all())
    assert call(need) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    assert bool(torch.isnan(obuf[:front]).all()) and bool(torch.isnan(obuf[front + cc * c:]).all())
    assert bool((wbuf[:256] == 0xA5).all()) and bool((wbuf[256 + need:] == 0xA5).all())
    # the operator's `out`
    assert dpa.gm_pair_matrix(x, c_begin=cb, c_count=cc, metric=metric, out=out) is out
    with pytest.raises(ValueError):
        dpa.gm_pair_matrix(x, c_begin=cb, c_count=cc, metric=metric, out=torch.empty(cc, c + 1, device=DEV))


# ----------------------------------------------------------------------------------------------------
# against the existing kernel, and the selection the matrix is for
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", po.METRICS)
def test_row_sums_are_the_gm_scores_summed_over_the_samples(metric):
    x = go.maps(4, 77, 5, 13, 7501)
    xd = x.to(DEV)
    rows = dpa.gm_pair_matrix(xd, metric=metric).double().sum(1).cpu().numpy()
    scores = dpa.gm_distance_nc(xd, metric=metric).double().sum(0).cpu().numpy()
    if metric == "l2":  # both relative: the two tolerances added
        np.testing.assert_allclose(rows, scores, rtol=po.TOL["l2"] + go.TOL, atol=0)
    else:  # both absolute per term: N * r_count terms per row
        import gm_metric_oracle as mo
        assert np.abs(rows - scores).max() <= (po.TOL[metric] + mo.TOL[metric]) * 4 * 77


def test_kcenter_on_the_kernels_matrix_keeps_one_copy_of_each_pattern():
    x = po.duplicate_case()
    D64 = po.pair_matrix_f64(x)
    order = pairs.kcenter_order(D64)
    # the float64 side decides with margins far above the tolerance: between the two largest row sums of distinct patterns,
    # and at every step up to the sixth between the chosen channel and the best one of another pattern
    # (relative margins, as the tolerance is)
    top = np.sort(D64.sum(1)[:6])
    assert (top[-1] - top[-2]) / top[-1] > 1e-3
    for t in range(1, 6):
        mind = D64[:, order[:t]].min(axis=1)
        others = [k for k in range(12) if k not in order[:t] and k % 6 != order[t] % 6]
        assert (mind[order[t]] - mind[others].max()) / mind[order[t]] > 1e-3, t
    got = dpa.gm_pair_matrix(x.to(DEV)).cpu().numpy()
    assert po.error(got, D64, "l2", 3, po.exact_zeros(x, "l2")) <= po.TOL["l2"]
    assert pairs.kcenter_order(got).tolist() == order.tolist()
    imp = pairs.score(got / 3.0, "kcenter")
    kept = np.sort(np.argsort(imp)[6:])
    assert kept.tolist() == [0, 1, 2, 3, 4, 5]
    assert np.sort(np.argsort(pairs.score(got, "sum"))[6:]).tolist() == [0, 3, 4, 6, 9, 10]  # the row sum keeps three patterns twice


# ----------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ranges", [("full", None), ("last12", None), ("full", [("a", 0, 5), ("b", 5, 24)])],
                         ids=["full", "last12", "ranges"])
def test_point_hook_device_and_host_accumulators_give_identical_bytes(kind, ranges, monkeypatch):
    monkeypatch.setattr(harness, "_gm_metric", "l2")
    xs = [go.maps(3, 24, 6, 5, 21).to(DEV), go.maps(2, 24, 6, 5, 22).to(DEV)]
    base, count = (12, 12) if kind == "last12" else (0, 24)
    scores = {}
    for form in ("host", "device"):
        hook = harness._PointHook(kind, form, torch.device(DEV), key="w", criterion="gm", pairs=True, ranges=ranges,
                                  nominal_c=count if ranges else None)
        for x in xs:
            hook(None, (x,), x)
        keys = ["w"] if ranges is None else [k for k, _, _ in ranges]
        scores[form] = np.concatenate([hook.scores(k) for k in keys])
        assert (hook.accs[keys[0]].sum.is_cuda) == (form == "device")
    assert scores["host"].shape == (count, count) and scores["host"].dtype == np.float32
    assert scores["host"].tobytes() == scores["device"].tobytes()
    want = sum(po.pair_matrix_f64(x.cpu(), "l2", base, count, base, count) for x in xs) / 5.0
    np.testing.assert_allclose(scores["host"], want, rtol=po.TOL["l2"] + 1e-6, atol=0)
    whole = harness._PointHook(kind, "device", torch.device(DEV), key="w", criterion="gm", pairs=True)
    for x in xs:
        whole(None, (x,), x)
    assert whole.scores("w").tobytes() == scores["device"].tobytes()  # the pieces are rows of the whole, bit for bit
