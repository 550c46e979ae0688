"""tests/_params.py pinned to the oracle (no GPU): params_ref reproduces the parameter parts of the oracle's end-to-end
functions and the bit-allocation golden bit for bit, and every bit-allocation input the GPU tests use keeps every live
channel's log2(bins) at least 2e-5 away from a rounding boundary - with the fp32 oracle equal to an fp64 restatement on it -
so a kernel that sums the prior in another order or takes its log2 an ulp apart has to give the same bits."""
import math

import numpy as np
import pytest
import torch

import _params as P
from conftest import bits_equal
from oracle import quant_oracle as O


def _table_of(x):
    st = O.act_stats_perchannel(x, ['min', 'max', 'std', 'b'])
    mean = O.act_stats_perchannel(x, ['mean'], avg_over_batch=True)['mean']          # the mean act_clipping_qdq uses
    return P.make_table(x.shape[1], st['min'], st['max'], mean, st['std'], st['b'])


BA_KW = [dict(), dict(bit_alloc_act=True), dict(bit_alloc_act=True, bit_alloc_round=False),
         dict(bit_alloc_act=True, bit_alloc_target=5.3), dict(bit_alloc_act=True, bit_alloc_prior='laplace')]


@pytest.mark.parametrize('shape,seed', [((4, 12, 7, 5), 1), ((3, 70, 4, 6), 2)])
def test_params_ref_reproduces_the_oracle(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen) * (torch.rand(1, shape[1], 1, 1, generator=gen) * 3 + 0.05) + 0.4
    table = _table_of(x)
    for nb in (4, 3):
        for half in (False, True):
            for kw in BA_KW:
                ba = kw.get('bit_alloc_act', False)
                pb = kw.get('bit_alloc_prior', 'gaus') == 'laplace'
                args = (ba, pb, kw.get('bit_alloc_target'), kw.get('bit_alloc_round', True))
                for clip in ('no', 'laplace', 'gaus', '2std'):
                    if clip == 'no':
                        _, parts = O.act_per_channel_qdq(x, nb, half_range=half, return_parts=True, **kw)
                    else:
                        _, parts = O.act_clipping_qdq(x, nb, clip, half_range=half, return_parts=True, **kw)
                    scale, zp, qmax, bits, alpha, delta, offset = P.params_ref(table, nb, half, clip, *args, False)
                    key = (nb, half, kw, clip)
                    assert bits_equal(scale, parts['scale']), key
                    assert bits_equal(zp, parts['zero_point']), key
                    assert bits_equal(qmax, np.broadcast_to(P.f32(parts['qmax']), qmax.shape)), key
                    if ba:
                        assert bits_equal(bits, parts['bit_alloc']), key
                    else:
                        assert parts['bit_alloc'] is None and bool((bits == nb).all()), key
                    if clip != 'no':
                        assert bits_equal(alpha, parts['alpha']) and bits_equal(offset, np.broadcast_to(P.f32(parts['offset']), offset.shape)), key
                        assert bits_equal(delta, P.f32(parts['max']) - P.f32(parts['min'])), key


def test_params_ref_reproduces_the_bit_alloc_golden(golden):
    g = golden('bit_alloc')
    for k in range(int(g.np('n_cases'))):
        std, target, rnd = g.t('k%d_std' % k), float(g.np('k%d_target' % k)), bool(g.np('k%d_round' % k))
        C = std.numel()
        table = P.make_table(C, -torch.ones(C), torch.ones(C), torch.zeros(C), std, std * 0.8)
        assert bits_equal(P.params_ref(table, 4, False, 'no', True, False, target, rnd, False)[3], g.np('k%d_bits' % k)), k


def _guard(prior, target, rnd, what):
    bits64, margin = P.bit_alloc_f64(prior, target, rnd)
    assert margin > P.MARGIN, (what, margin)
    got = O.bits_alloc_fixed_target(prior, P._target(4, target), rnd).numpy().astype(np.float64)
    assert np.array_equal(got, bits64), what


def test_seed_guard():
    """Every (C, target, round_mode, seed) of the GPU test: margin > 2e-5, fp32 oracle == fp64 restatement."""
    cases = P.ba_cases()
    assert len(cases) == 10 * len(P.BA_COMBOS) + 2
    for C, target, rnd, seed in cases:
        assert C > 1 or (rnd and target == int(target))
        _guard(P.guarded_prior(C, seed), target, rnd, (C, target, rnd, seed))
    for target, rnd in P.BA_COMBOS:
        hi = P.hi_prior(P.HI_SEED)
        _guard(hi, target, rnd, ('hi', target, rnd))
        _guard(hi.flip(0), target, rnd, ('hi flipped', target, rnd))
    table = P.edge_table()
    for nb, rnd in P.EDGE_BA:
        for row in (P.STAT_STD, P.STAT_B):
            _guard(table[row], nb, rnd, ('edge', nb, rnd, row))


def test_clamped_targets_have_no_live_channel():
    """The all-8 and all-0 targets of the GPU test: no channel ever comes near a rounding boundary (margin inf)."""
    for C in (65, 6000):
        pr = P.guarded_prior(C, 0)
        for target, want in ((40, 8.), (-40, 0.)):
            for rnd in (True, False):
                bits64, margin = P.bit_alloc_f64(pr, target, rnd)
                assert margin == math.inf and bool((bits64 == want).all())
                assert bool((O.bits_alloc_fixed_target(pr, target, rnd) == want).all())


def test_pt_params_ref_is_the_oracle_route():
    """pt_params_ref's words reproduce what O.float2gemmlowp derives inside: quantizing with them as given range / offset /
    true-zero flag gives O.gemmlowp_minmax_qdq's output on the same extrema."""
    gen = torch.Generator().manual_seed(3)
    for shift in (0.2, 3.0, -3.0):
        x = torch.randn(6, 40, generator=gen) + shift
        for avg in (True, False):
            mins, maxs = x.min(dim=1)[0], x.max(dim=1)[0]
            for etz in (True, False):
                for bits in (2, 8):
                    w = P.pt_params_ref(mins, maxs, 0 if avg else 1, False, bits, False, etz)
                    mn, mx = P.pt_extrema(mins, maxs, 0 if avg else 1, False)
                    want = O.gemmlowp_minmax_qdq(x, bits, enforce_true_zero=etz, min_=mn, max_=mx)
                    got = O.float2gemmlowp(x, w[5], w[6], bits, False, bool(w[3]))
                    assert bits_equal(got, want)
                    assert w[2] == 2 ** bits - 1 and w[4] == 0. and w[7] == 0.
    # the exact ceiling of log2: powers of two map to themselves
    for k in range(-140, 128):
        assert P.exact_ceil_log2(2. ** k) == k
    assert P.exact_ceil_log2(np.float32(1.0000001)) == 1 and P.exact_ceil_log2(np.float32(0.99999994)) == 0
