"""The KLD calibration kernels on hand-built inputs (tests/_kld.py; conditions on them: test_kld_table_cpu.py).

k_kld_search / k_kld_pick see histograms chosen to hit their index arithmetic, uploaded straight through cnnq_kld_search; k_kld_hist
sees float32 values on and next to the bin edges, chunk boundaries on both load paths, more rows than CUs, and rows that are not
finite.  Histograms are integer work: exact against numpy.histogram.  The 994 divergences are compared with the longdouble
restatement T.divergences64 at |div - div64| <= TOL * mag, mag = sum |p_k log(p_k / q_k)| (an absolute TOL where mag is 0).

MEASURED on the MI355X: the worst |div - div64| / mag over every case of this file is 2.63e-13 ('smooth_ulp', candidate 3, whose P and
Q nearly coincide: mag = 1.3e-4 while the terms' p_k sum to 1, so the 3e-17 absolute rounding of an fp64 sum weighs that much; a
plain fp64 evaluation on the CPU sits as far from the longdouble one).  Everywhere else the ratio is below 3e-14 ('ones',
candidate 993, mag 5e-3), on data-like histograms 4e-16 .. 2e-15.  So T.TOL = 8 x 2.63e-13 = 2.1e-12; the condition on it is TOL <=
1e-10, four orders below what an fp32 accumulation shows (1.1e-6).  Every test prints its ratios (-s)."""
import numpy as np
import pytest
import torch

import _kld as T
from cnn_quantization_amd import _lib, ops

pytestmark = pytest.mark.gpu
KCHUNK = 65536                                 # elements of one row per workgroup of k_kld_hist


def search(hists, rowmm):
    """One call of cnnq_kld_search on an int64 [rows, 2001] table and float32 (min, max) pairs -> (div [rows, 994], out [rows, 3])."""
    hists = np.asarray(hists, dtype=np.int64)
    rows = hists.shape[0]
    assert hists.shape == (rows, T.NB) and hists.max() < 2 ** 31
    h = torch.from_numpy(hists.astype(np.int32)).cuda()            # the kernel reads uint32: the same bits below 2^31
    mm = torch.tensor(np.asarray(rowmm, dtype=np.float32).T.copy()).cuda()      # [2, rows]: the MIN row, then the MAX row
    div = torch.full((rows, T.NC), -7., dtype=torch.float64, device='cuda')
    out = torch.full((rows, 3), -7., dtype=torch.float64, device='cuda')
    _lib.check(_lib.load().cnnq_kld_search(ops._ptr(h), rows, ops._ptr(mm), ops._ptr(div), ops._ptr(out), ops._stream(h)),
               'cnnq_kld_search')
    return div.cpu().numpy(), out.cpu().numpy()


def check_search(names, hists, rowmm, div, out):
    """Every requirement of the search and the pick, row by row -> the worst |div - div64| / mag met."""
    worst = 0.
    for r, (name, hist, (mn, mx)) in enumerate(zip(names, hists, rowmm)):
        div64, mag = T.divergences64(hist)
        nan = np.isnan(div64)
        assert np.array_equal(np.isnan(div[r]), nan), name
        ok = ~nan
        scale = np.where(mag[ok] == 0, np.longdouble(1), mag[ok])
        ratio = np.abs(div[r][ok] - div64[ok]) / scale
        if ratio.size:
            c = int(np.argmax(ratio))
            print('%-22s worst |div - div64| / mag = %.3g (candidate %d, mag %.3g)' % (name, ratio[c], np.flatnonzero(ok)[c], mag[ok][c]))
            worst = max(worst, float(ratio[c]))
        assert (ratio <= T.TOL).all(), name
        k = int(out[r, 2])
        assert out[r, 2] == k and 0 <= k < T.NC, name
        if nan.any():
            assert k == 0 and nan[0], name
        else:
            assert div64[k] <= div64.min() + T.TOL * (mag[k] if mag[k] else 1), (name, k, T.pick64(hist))
            if T.is_clear(hist):
                assert k == T.pick64(hist), name
        assert out[r, 1:2].view(np.int64)[0] == div[r, k:k + 1].view(np.int64)[0], name            # div[k] bit for bit
        assert out[r, 0] == T.edges64(mn, mx)[T.ZERO + (k + T.HALF_Q) + 1], (name, k, mn, mx)
    return worst


def test_search_and_pick_on_hand_built_histograms():
    names = T.CASE_NAMES
    hists = [T.CASES[n] for n in names]
    rowmm = [T.ROWMM[r % len(T.ROWMM)] for r in range(len(names))]
    div, out = search(np.stack(hists), rowmm)
    worst = check_search(names, hists, rowmm, div, out)
    print('worst ratio %.3g, TOL %.3g' % (worst, T.TOL))
    # k = 993: the edge is `last` itself, which 2001 * step + first misses on this range (test_kld_table_cpu.py)
    assert out[names.index('ones'), 2] == T.NC - 1 and out[names.index('ones'), 0] == T.F32_MAX


def hist_parts(x):
    out, hist, div = ops.kld_thresholds(x, want_parts=True)
    return out.cpu().numpy(), hist.cpu().numpy().astype(np.int64), div.cpu().numpy()


@pytest.mark.parametrize('length_mod4,drop_parity', [(0, 1), (1, 0)])
def test_histogram_on_edge_valued_rows(length_mod4, drop_parity):
    batch = T.edge_batch(length_mod4, drop_parity)
    x = torch.from_numpy(batch).cuda()
    assert x.data_ptr() % 16 == 0 and x.shape[1] % 4 == length_mod4        # k_kld_hist<4> in one call, <1> in the other
    out, hist, div = hist_parts(x)
    refs = [T.numpy_hist(row) for row in batch]
    for r, th in enumerate(T.EDGE_TH):
        bad = np.flatnonzero(hist[r] != refs[r])
        assert bad.size == 0, 'th = %r: bins %s hold %s, numpy %s' % (float(th), bad[:8], hist[r][bad[:8]], refs[r][bad[:8]])
    names = ['th=%r' % float(th) for th in T.EDGE_TH]
    worst = check_search(names, refs, [(row.min(), row.max()) for row in batch], div, out)
    print('worst ratio %.3g, TOL %.3g' % (worst, T.TOL))


CHUNK_VALUES = np.array([-1., -0.999, -0.75, -0.5, -0.3333, -0.25, -0.1, -0.001, -0., 0., 0.0005, 0.001, 0.2, 0.3, 0.5, 0.7, 0.9,
                         0.9995, 0.99999, 1.], dtype=np.float32)


@pytest.mark.parametrize('aligned', [True, False])
@pytest.mark.parametrize('length', [KCHUNK - 1, KCHUNK, KCHUNK + 1, 2 * KCHUNK + 4])
def test_chunk_geometry(length, aligned):
    rows = 3
    rng = np.random.default_rng(length)
    scale = np.array([[1.], [0.37], [250.]], dtype=np.float32)
    weight = np.where(np.isin(CHUNK_VALUES, (0.5, -0.25)), 8., 1.)          # two bins collect a quarter of the row each
    x_np = CHUNK_VALUES[rng.choice(CHUNK_VALUES.size, (rows, length), p=weight / weight.sum())] * scale
    x_np[:, 0], x_np[:, -1] = scale[:, 0], -scale[:, 0]                     # the extremes sit on the row's first and last element
    base = torch.zeros(rows * length + 1, dtype=torch.float32, device='cuda')
    x = base[0 if aligned else 1:][:rows * length].view(rows, length)
    x.copy_(torch.from_numpy(x_np))
    # a view one element into its storage is contiguous but not 16-byte aligned: the scalar path, across the chunks
    assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == aligned
    out, hist, div = hist_parts(x)
    for r in range(rows):
        ref = T.numpy_hist(x_np[r])
        assert ref.max() > 15000                                            # one bin through the eight replicas and the merge
        assert hist[r].sum() == length
        assert np.array_equal(hist[r], ref), (r, np.flatnonzero(hist[r] != ref)[:8])


def test_many_rows():
    rows, length = 300, 64
    rng = np.random.default_rng(11)
    x_np = (rng.laplace(0.1, 1., (rows, length)) * np.geomspace(1e-3, 1e3, rows)[:, None]).astype(np.float32)
    out, hist, div = hist_parts(torch.from_numpy(x_np).cuda())
    refs = [T.numpy_hist(row) for row in x_np]
    assert np.array_equal(hist, np.stack(refs))
    pickr = [int(r) for r in np.linspace(0, rows - 1, 8)]
    worst = check_search(['row %d' % r for r in pickr], [refs[r] for r in pickr], [(x_np[r].min(), x_np[r].max()) for r in pickr],
                         div[pickr], out[pickr])
    print('worst ratio %.3g, TOL %.3g' % (worst, T.TOL))
    # every other row: the pick belongs to its own row's curve and range
    for r in range(rows):
        k = int(out[r, 2])
        assert out[r, 0] == T.edges64(x_np[r].min(), x_np[r].max())[T.ZERO + (k + T.HALF_Q) + 1]
        assert k == T.pick(div[r]) and (out[r, 1] == div[r, k] or np.isnan(div[r, k]))


def assert_no_range(hist_row, div_row, out_row):
    assert not hist_row.any()
    assert np.isnan(div_row).all()
    assert np.isnan(out_row[0]) and np.isnan(out_row[1]) and out_row[2] == 0


@pytest.mark.parametrize('length', [1000, 1001])
def test_non_finite_rows(length):
    """numpy.histogram refuses a non-finite range, so the reference raises; a device call cannot.  A row whose min or max is not
    finite gets an all-zero histogram and out = (NaN, NaN, 0); its neighbours are what they are without it."""
    rng = np.random.default_rng(3)
    good = rng.laplace(0., 0.7, (4, length)).astype(np.float32)
    x_np = np.stack([good[0], good[1], good[1], good[2], good[2], good[3], good[3]])
    x_np[1, 17] = np.nan
    x_np[2, length - 1] = np.inf
    x_np[4, 0] = -np.inf
    x_np[5, 500] = np.inf
    x_np[5, 501] = -np.inf
    bad, fine = [1, 2, 4, 5], [0, 3, 6]
    out, hist, div = hist_parts(torch.from_numpy(x_np).cuda())
    out0, hist0, div0 = hist_parts(torch.from_numpy(np.ascontiguousarray(x_np[fine])).cuda())
    assert np.array_equal(hist[fine], hist0) and np.array_equal(hist0, np.stack([T.numpy_hist(x_np[r]) for r in fine]))
    assert np.array_equal(div[fine].view(np.int64), div0.view(np.int64)) and np.array_equal(out[fine].view(np.int64), out0.view(np.int64))
    for r in bad:
        assert_no_range(hist[r], div[r], out[r])
    assert np.isnan(out[:, 0].max()) and np.isnan(torch.from_numpy(out)[:, 0].max().item())       # what kld_th becomes


def test_non_finite_range_given_by_hand():
    """The C ABI takes (min, max) from the caller: one non-finite word is enough, whichever it is, whatever the histogram holds."""
    lib = _lib.load()
    inf, nan = np.inf, np.nan
    rowmm = [(-1., 1.), (nan, 1.), (-1., nan), (-inf, 1.), (-1., inf), (-inf, inf), (nan, nan), (-2., 0.5)]
    rows, length = len(rowmm), 260
    x_np = np.tile(np.linspace(-1., 1., length, dtype=np.float32), (rows, 1))
    x = torch.from_numpy(x_np).cuda()
    mm = torch.tensor(np.asarray(rowmm, dtype=np.float32).T.copy()).cuda()
    hist = torch.full((rows, T.NB), 5, dtype=torch.int32, device='cuda')                   # cnnq_kld_hist zeroes it
    _lib.check(lib.cnnq_kld_hist(ops._ptr(x), rows, length, ops._ptr(mm), ops._ptr(hist), ops._stream(x)), 'cnnq_kld_hist')
    hist = hist.cpu().numpy().astype(np.int64)
    ref = T.numpy_hist(x_np[0])
    assert np.array_equal(hist[0], ref) and hist[7].sum() == length
    for r in range(1, 7):
        assert not hist[r].any(), rowmm[r]
    div, out = search(np.stack([T.CASES['laplace']] * rows), rowmm)
    for r in range(1, 7):
        assert np.isnan(out[r, 0]) and np.isnan(out[r, 1]) and out[r, 2] == 0, rowmm[r]
    check_search(['finite'] * 2, [T.CASES['laplace']] * 2, [rowmm[0], rowmm[7]], div[[0, 7]], out[[0, 7]])
