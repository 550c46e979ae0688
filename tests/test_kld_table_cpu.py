"""tests/_kld.py pinned without a GPU: the longdouble restatement of the KLD divergences against the oracle and the golden rows,
the device's histogram index rule (restated in numpy) against numpy.histogram on the edge-valued rows, and the conditions on the
inputs that test_kld_table_gpu.py relies on - asserted here, from the reference alone, so the GPU test cannot hide behind them."""
import numpy as np
import pytest

import _kld as T
from oracle import kld_oracle as K

RTOL, ATOL = 2e-5, 2e-7                       # test_kld_gpu.py's: float32 sums in the oracle, longdouble sums in the restatement


@pytest.mark.parametrize('name', T.CASE_NAMES)
def test_restatement_is_the_oracle_up_to_its_float32_sums(name):
    hist = T.CASES[name]
    _, odiv = K.divergences(np.asarray(hist), T.edges64(-1., 1.))
    div, mag = T.divergences64(hist)
    assert np.array_equal(np.isnan(div), np.isnan(odiv))
    assert np.array_equal(np.isnan(div), np.isnan(mag))
    ok = ~np.isnan(odiv)
    use = np.abs(div[ok].astype(np.float64) - odiv[ok]) / (ATOL + RTOL * np.abs(odiv[ok]))
    print('%s: %.2f of the tolerance' % (name, use.max() if use.size else 0.))
    assert (use <= 1).all()
    assert (mag[ok] >= np.abs(div[ok])).all()


@pytest.mark.parametrize('name', ['laplace', 'relu', 'gauss_outlier', 'band', 'zeros', 'tiny', 'grid', 'negskew', 'huge_zero'])
def test_restatement_picks_the_recorded_threshold(golden, name):
    g = golden('kld')
    x = g.np('in_' + name)
    hist = T.numpy_hist(x)
    k = T.pick64(hist)
    assert T.edges64(x.min(), x.max())[T.ZERO + (k + T.HALF_Q) + 1] == float(g.np('th_' + name))


def test_empty_row_is_nan():
    div, mag = T.divergences64(np.zeros(T.NB, dtype=np.int64))
    assert np.isnan(div).all() and np.isnan(mag).all()


def test_the_restatement_resolves_what_the_tolerance_claims():
    """A float32 accumulation, and a smoothing constant formed in float32, move a divergence by far more than TOL * mag: the GPU
    test's tolerance separates them from the kernel's fp64 arithmetic."""
    parts = T.smoothed(T.CASES['laplace'])
    div, mag = T.divergences64(T.CASES['laplace'])
    d32, _ = T._kl(*parts, np.float32)
    assert np.max(np.abs(d32 - div) / mag) > 1000 * T.TOL
    # 'smooth_ulp', candidate 95: the two roundings of the constant differ and change float32(count + constant)
    f = np.float32
    once, twice = f(-(T.EPS * 158. / 47.)), -(f(T.EPS) * f(158) / f(47))
    assert once != twice and f(9) + once != f(9) + twice and f(16) + once != f(16) + twice
    start, stop, _ = T._bounds(95)
    p = T.CASES['smooth_ulp'][start:stop]
    assert (p == 0).sum() == 158 and p.size == 205 and T.CASES['smooth_ulp'].sum() == p.sum()


@pytest.mark.parametrize('length_mod4,drop_parity', [(0, 1), (1, 0)])
def test_device_index_rule_gives_numpy_counts_on_edge_rows(length_mod4, drop_parity):
    batch = T.edge_batch(length_mod4, drop_parity)
    assert batch.shape[1] % 4 == length_mod4
    downs = ups = 0
    for r, th in enumerate(T.EDGE_TH):
        row = batch[r]
        assert np.abs(row).max() == th and (row.max() < th) == T.edge_drops(r, drop_parity)
        ref = T.numpy_hist(row)
        assert ref.sum() == row.size
        idx, down, up = T.device_index(row)
        assert np.array_equal(np.bincount(idx, minlength=T.NB), ref), 'th = %r' % float(th)
        downs, ups = downs + down, ups + up
    assert downs > 0 and ups > 0              # both corrections of the estimate are exercised, not only available


def test_conditions_on_the_inputs():
    assert 0 < T.TOL <= T.TOL_CAP
    for name, hist in T.CASES.items():
        assert hist.shape == (T.NB,) and hist.min() >= 0 and hist.sum() < 2 ** 31, name
    clear = [name for name in T.CASE_NAMES if T.is_clear(T.CASES[name])]
    assert 4 * len(clear) >= 3 * len(T.CASES), clear
    # the near tie the 'either may win' clause exists for: float32 sums and longdouble sums choose differently
    h = T.CASES['ends_2p30']
    assert int(np.argmin(K.divergences(np.asarray(h), T.edges64(-1., 1.))[1])) != T.pick64(h)
    # every rounding of a count: 2^24 + 1 is not a float32, the folded ends lie above 2^24
    assert np.float32(T.CASES['big24'].max()) != T.CASES['big24'].max() and h[0] > 2 ** 24 and h[-1] > 2 ** 24
    # range 2001.0: step 2, every edge an odd integer, float32-exact
    e = T.edges64(-2001., 2001.)
    assert np.array_equal(e.astype(np.float32).astype(np.float64), e) and np.array_equal(e, -2001. + 2. * np.arange(T.NB + 1))
    for parity in (0, 1):
        for r, th in enumerate(T.EDGE_TH):
            assert T.edge_row(th, T.edge_drops(r, parity)).size >= 5000, float(th)
    # the group cases: the last group of GROUP_CAND is wider than the others
    start, stop, w = T._bounds(T.GROUP_CAND)
    assert (stop - start) % T.NQ != 0 and w * T.NQ < stop - start
    # candidate 993's edge is `last` itself, which k * step + first misses for at least one hand-given range
    e = T.edges64(*T.ROWMM[T.CASE_NAMES.index('ones') % len(T.ROWMM)])
    assert T.pick64(T.CASES['ones']) == T.NC - 1 and T.NB * ((e[-1] - e[0]) / T.NB) + e[0] != e[-1]
