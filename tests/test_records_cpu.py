"""tests/_records.py pinned, without a GPU: the restatement of the record-merge kernels computes the reference's
statistics, is exact where it claims to be, and the hand-built records have at stake what their names say - computed from the
restatement alone, so that no case of test_records_table_gpu.py can pass on the device by having nothing to lose.

The only tolerances here are the tiers of test_hip_parity.test_stats_collect_set_vs_oracle (the fixtures' rows come from float32
torch reductions) and the 1 ulp of float32 of the dyadic check."""
import warnings

import numpy as np
import pytest
import torch

import _records as R
from conftest import bits_equal

F64, F32 = np.float64, np.float32
PAIRS = [(G, C) for G in R.GRID_G for C in R.GRID_C]


def test_constants_are_the_library_s():
    from cnn_quantization_amd import _lib as L
    for name in ('MOM_MIN', 'MOM_MAX', 'MOM_SUM', 'MOM_SUMSQ', 'MOM_COUNT', 'MOM_SUM_RELU', 'MOM_SUMSQ_RELU', 'NMOM', 'STAT_MIN',
                 'STAT_MAX', 'STAT_MEAN', 'STAT_STD', 'STAT_B', 'STAT_KURT', 'STAT_STD_POS', 'NSTAT', 'DEV_ABS', 'DEV_Z4', 'NDEV'):
        assert getattr(R, name) == getattr(L, name), name


def test_the_grid_reaches_every_lane_layout_and_every_border():
    segs = {R.mseg_of(G, C) for G, C in PAIRS}
    assert segs == set(R.SEGS)
    assert [R.mseg_of(G, 512) for G in (16, 17, 64, 65)] == [1, 8, 8, 64]
    assert [R.mseg_of(G, 511) for G in (16, 17, 64, 65)] == [64] * 4
    for seg in R.SEGS:                                  # workgroups full, short by one and one over, per layout
        cpw = R.TPB // seg
        assert {0, 1, cpw - 1} <= {C % cpw for G, C in PAIRS if R.mseg_of(G, C) == seg and C > 1}, seg


# ------------------------------------------------------------------------------------------ the formulas are the reference's
def sample_records(x):
    """one pass-A record per sample of x [N, C, H, W] float32, in numpy float64"""
    N, C = x.shape[:2]
    t = x.reshape(N, C, -1).astype(F64)
    r = np.maximum(t, 0.)
    part = np.empty((N, R.NMOM, C), dtype=F64)
    part[:, R.MOM_MIN], part[:, R.MOM_MAX] = t.min(-1), t.max(-1)
    part[:, R.MOM_SUM], part[:, R.MOM_SUMSQ] = t.sum(-1), (t * t).sum(-1)
    part[:, R.MOM_COUNT] = t.shape[-1]
    part[:, R.MOM_SUM_RELU], part[:, R.MOM_SUMSQ_RELU] = r.sum(-1), (r * r).sum(-1)
    return part


def sample_dev_records(x, stats):
    """one pass-B record per sample from the float32 mean and std of `stats`, the per-element arithmetic of k_absdev"""
    N, C = x.shape[:2]
    t = x.reshape(N, C, -1)
    d = (t - stats[R.STAT_MEAN].reshape(1, C, 1)).astype(F32)
    with np.errstate(all='ignore'):
        z = (d * (F32(1) / stats[R.STAT_STD]).reshape(1, C, 1)).astype(F32)
        z2 = (z * z).astype(F32)
        z4 = (z2 * z2).astype(F32)
    part2 = np.empty((N, R.NDEV, C), dtype=F64)
    part2[:, R.DEV_ABS], part2[:, R.DEV_Z4] = np.abs(d).astype(F64).sum(-1), z4.astype(F64).sum(-1)
    return part2


def fixture_cases(golden):
    g = golden('collect')
    for bi in range(2):
        for k in range(3):
            yield 'collect b%d x%d' % (bi, k), g.np('b%d_x%d' % (bi, k)), {s: g.np('b%d_%s' % (bi, s))[k] for s in
                                                                         ('max', 'min', 'std', 'mean', 'kurtosis', 'b', 'std_pos')}, bi == 0
    g = golden('collect_flat')
    for k in range(2):
        yield 'collect_flat x%d' % k, g.np('x%d' % k), {s: g.np('b0_%s' % s)[k] for s in
                                                        ('max', 'min', 'std', 'mean', 'kurtosis', 'b', 'std_pos')}, True


def test_the_formulas_are_the_reference_s(golden):
    """records of the fixtures' x, one per sample, through combine_ref / combine_dev_ref against the reference-generated rows:
    extrema bit for bit, the rest at the tiers of test_hip_parity.test_stats_collect_set_vs_oracle"""
    n = 0
    for name, x, want, exact_extrema in fixture_cases(golden):
        part = sample_records(np.ascontiguousarray(x, dtype=F32))
        mom, stats = R.combine_ref(part, 1)
        part2 = sample_dev_records(x, stats)
        dev, stats = R.combine_dev_ref(part2, mom, 1, stats)
        if exact_extrema:                                   # (batch_avg: the reference averages the per-sample extrema)
            assert bits_equal(stats[R.STAT_MIN], want['min']) and bits_equal(stats[R.STAT_MAX], want['max']), name
        for row, key in ((R.STAT_MEAN, 'mean'), (R.STAT_STD, 'std'), (R.STAT_B, 'b'), (R.STAT_STD_POS, 'std_pos')):
            np.testing.assert_allclose(stats[row], want[key], rtol=5e-6, atol=2e-6, err_msg='%s %s' % (name, key))
        np.testing.assert_allclose(stats[R.STAT_KURT], want['kurtosis'], rtol=1e-3, atol=5e-4, err_msg=name)
        assert np.array_equal(mom[R.MOM_COUNT], np.full(x.shape[1], x.shape[0] * x.shape[2] * x.shape[3], dtype=F64))
        n += 1
    assert n == 8


def ulps32(a, b):
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return np.abs(a.astype(F64) - b.astype(F64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(F64)


@pytest.mark.parametrize('shape', [(1, 1, 1, 2), (3, 5, 7, 7), (17, 4, 3, 5), (64, 3, 2, 2), (130, 2, 1, 3)])
def test_dyadic_tensors_against_torch_in_float64(shape):
    """values k / 64: every float64 sum and sum of squares is exact, so combine_ref must be torch's float64 mean / std(unbiased) /
    clamp(min=0).std rounded to float32, within 1 ulp of float32 (the two differ in how the variance is formed, not in its sums)"""
    rng = np.random.default_rng(shape[0] + shape[1])
    x = (rng.integers(-256, 257, size=shape).astype(F64) / 64.).astype(F32)
    part = sample_records(x)
    for seg in R.SEGS:
        mom, stats = R.combine_ref(part, 1, seg=seg)
        t = torch.from_numpy(x).double().transpose(0, 1).reshape(shape[1], -1)
        assert np.array_equal(mom[R.MOM_SUM], t.sum(1).numpy()) and np.array_equal(mom[R.MOM_SUMSQ], (t * t).sum(1).numpy())
        assert bits_equal(stats[R.STAT_MIN], t.min(1)[0].float()) and bits_equal(stats[R.STAT_MAX], t.max(1)[0].float())
        for row, ref in ((R.STAT_MEAN, t.mean(1)), (R.STAT_STD, t.std(1, unbiased=True)),
                         (R.STAT_STD_POS, t.clamp(min=0).std(1, unbiased=True))):
            assert (ulps32(stats[row], ref.float().numpy()) <= 1).all(), (seg, row)


# ------------------------------------------------------------------------------------------ exactness on integers
@pytest.mark.parametrize('G,C', [(1, 1), (2, 5), (17, 65), (65, 513), (130, 63), (256, 1031)])
def test_integer_records_merge_exactly_in_every_order(G, C):
    part = R.integer_records(G, C)
    assert (np.abs(part) < 2 ** 21).all() and (part == np.rint(part)).all()
    assert (part[:, R.MOM_MIN] < part[:, R.MOM_MAX]).all() and (part[:, R.MOM_COUNT] > 0).all()
    # every word differs from its neighbours in g, row and c
    for axis in range(3):
        if part.shape[axis] > 1:
            assert (np.diff(np.abs(part), axis=axis) != 0).all(), axis
    want = part.sum(0)
    want[R.MOM_MIN], want[R.MOM_MAX] = part[:, R.MOM_MIN].min(0), part[:, R.MOM_MAX].max(0)
    for seg in R.SEGS:
        for ascending in (False, True):
            mom, stats = R.combine_ref(part, 1, seg=seg, ascending=ascending)
            assert R.same_bits64(mom, want), (seg, R.first_diff(mom, want))
    mom0, stats0 = R.combine_ref(part, 0)
    assert (mom0[R.MOM_SUM_RELU:] == 0).all() and (stats0[R.STAT_STD_POS] == 0).all()
    assert R.same_bits64(mom0[:R.MOM_SUM_RELU], want[:R.MOM_SUM_RELU])


@pytest.mark.parametrize('G,C', [(2, 3), (17, 65), (64, 512), (130, 5), (256, 513)])
def test_two_level_merge_is_the_one_level_merge_on_integers(G, C):
    part = R.integer_records(G, C)
    mom1, stats1 = R.combine_ref(part, 1)
    for W in R.TWO_LEVEL_W:
        if W > G:
            continue
        moms, (mom2, stats2) = R.two_level_ref(part, W, 1)
        assert moms.shape == (W, R.NMOM, C)
        assert R.same_bits64(mom2, mom1) and R.same_bits32(stats2, stats1), W


def test_the_older_restatement_agrees():
    """test_distributed_cpu.merge_records / stats_from_record ("the arithmetic of cnnq_pc_combine") against combine_ref"""
    import test_distributed_cpu as D
    for G, C in ((2, 6), (3, 65), (8, 513)):
        part = R.integer_records(G, C)
        mom, stats = R.combine_ref(part, 1)
        merged = D.merge_records(torch.from_numpy(part.copy()))
        assert R.same_bits64(merged.numpy(), mom)
        mn, mx, mean, std = (t.numpy() for t in D.stats_from_record(merged))
        for row, got in ((R.STAT_MIN, mn), (R.STAT_MAX, mx), (R.STAT_MEAN, mean), (R.STAT_STD, std)):
            assert R.same_bits32(got, stats[row]), (G, C, row)


# ------------------------------------------------------------------------------------------ the named channels
def named_tables():
    """(G, C, rot, part, named) for a spread of the grid; every name occurs"""
    for G, C in ((1, 5), (2, 63), (3, 1031), (16, 512), (17, 513), (64, 64), (65, 1031), (256, 63)):
        for rot in R.ROTATIONS:
            part, named = R.with_named(R.ordered_records(G, C, R.ordered_seed(G, C)), rot)
            yield G, C, rot, part, named


def test_named_channels_do_what_their_names_say():
    seen = set()
    for G, C, rot, part, named in named_tables():
        base = R.ordered_records(G, C, R.ordered_seed(G, C))
        others = [c for c in range(C) if c not in named]
        assert R.same_bits64(part[:, :, others], base[:, :, others])           # neighbours untouched
        mom, stats = R.combine_ref(part, 1)
        assert not np.isnan(stats[:, others]).any() and not np.isnan(mom[:, others]).any()
        for ch, name in named.items():
            seen.add(name)
            where = (G, C, rot, ch, name)
            m, s = mom[:, ch], stats[:, ch]
            if name in R.TOTALS:
                ts, tss, tcnt = R.TOTALS[name][:3]
                for seg in R.SEGS:                     # the totals come out exactly, whatever the order
                    for ascending in (False, True):
                        mm = R.combine_ref(part[:, :, ch:ch + 1], 1, seg=seg, ascending=ascending)[0][:, 0]
                        assert (mm[R.MOM_SUM], mm[R.MOM_SUMSQ], mm[R.MOM_COUNT]) == (ts, tss, tcnt), where
                        assert (mm[R.MOM_SUM_RELU], mm[R.MOM_SUMSQ_RELU]) == (ts, tss), where
                assert bits_equal(s[R.STAT_STD_POS], s[R.STAT_STD]) or (np.isnan(s[R.STAT_STD]) and np.isnan(s[R.STAT_STD_POS]))
                if G > 2:
                    assert len(set(part[:, R.MOM_SUM, ch])) > 1                 # the records differ from one another
                var = (F64(tss) - F64(ts) * (F64(ts) / F64(tcnt)))
            if name == 'count_one':
                assert np.isnan(s[R.STAT_STD]) and s[R.STAT_MEAN] == F32(2.5), where
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')                            # "degrees of freedom is <= 0"
                    assert bool(torch.isnan(torch.tensor([2.5], dtype=torch.float64).std(unbiased=True)))    # what torch.std gives
            elif name == 'count_two':
                assert bits_equal(s[R.STAT_STD], F32(np.sqrt(0.5))) and s[R.STAT_MEAN] == F32(1.5), where
                assert float(torch.tensor([1., 2.], dtype=torch.float64).std()) == float(np.sqrt(0.5))    # (s = 3, ss = 5)
            elif name in ('negative_variance', 'constant'):
                assert var < 0, where                                          # the clamp has something to clamp
                assert s[R.STAT_STD] == 0 and not np.signbit(s[R.STAT_STD]), where
                if name == 'constant':
                    assert s[R.STAT_MEAN] == F32(0.1), where
            elif name in ('mean_tie', 'mean_tie_up'):
                mean = F64(ts) / F64(tcnt)
                lo, hi = (F32(1), np.nextafter(F32(1), F32(2))) if name == 'mean_tie' else \
                    (np.nextafter(F32(1), F32(2)), F32(1) + F32(2. ** -22))
                assert mean - F64(lo) == F64(hi) - mean > 0, where             # exactly halfway between two floats
                even = lo if name == 'mean_tie' else hi
                assert even.view(np.uint32) % 2 == 0 and bits_equal(s[R.STAT_MEAN], even), where
            elif name == 'count_2p24_plus_1':
                want = F32(F64(2. ** 24) / F64(2. ** 24 + 1))
                assert want == np.nextafter(F32(1), F32(0)) and bits_equal(s[R.STAT_MEAN], want), where
                assert F32(2. ** 24) / F32(2. ** 24 + 1) == F32(1)             # a float32 count would answer 1
            elif name == 'huge':
                assert s[R.STAT_STD] == np.inf and np.isfinite(np.sqrt(F64(1e300) / 9)) and s[R.STAT_MEAN] == 0, where
            elif name == 'empty_among_full':
                twin = R.empty_twin(part, ch)
                empty = R.empty_positions(G, ch, rot)
                assert 0 < twin.shape[0] == G - int(empty.sum()) and (G < 3 or empty.any()), where
                tm, ts_ = R.combine_ref(twin, 1)
                assert R.same_bits64(tm[:, 0], m) and R.same_bits32(ts_[:, 0], s), where
                assert not np.isnan(s).any() and np.isfinite(m).all(), where
            elif name == 'all_empty':
                assert m[R.MOM_MIN] == np.inf and m[R.MOM_MAX] == -np.inf and m[R.MOM_COUNT] == 0, where
                assert s[R.STAT_MIN] == np.inf and s[R.STAT_MAX] == -np.inf, where
                assert np.isnan(s[R.STAT_MEAN]) and np.isnan(s[R.STAT_STD]), where
            elif name == 'nan_record':
                assert int(np.isnan(part[:, R.MOM_SUM, ch]).sum()) == 1, where
                assert np.isnan(s[[R.STAT_MIN, R.STAT_MAX, R.STAT_MEAN, R.STAT_STD]]).all(), where
                assert np.isnan(m[[R.MOM_MIN, R.MOM_MAX, R.MOM_SUM, R.MOM_SUMSQ]]).all() and m[R.MOM_COUNT] > 0, where
            elif name == 'inf_extrema':
                assert s[R.STAT_MAX] == np.inf and s[R.STAT_MEAN] == np.inf and np.isnan(s[R.STAT_STD]), where
                assert np.isfinite(s[R.STAT_MIN]), where
            elif name == 'signed_zero':
                col = part[:, :, ch]
                assert (col[:, R.MOM_MIN] >= 0).all() and (col[:, R.MOM_MAX] <= 0).all(), where
                assert s[R.STAT_MIN] == 0 and s[R.STAT_MAX] == 0, where
                if G > 1:
                    assert sorted(np.signbit(col[col[:, R.MOM_MIN] == 0, R.MOM_MIN])) == [False, True], where
    assert seen == set(R.NAMES)


def test_the_sign_of_a_zero_minimum_depends_on_the_restated_pmind():
    """fmin / fmax or another tie rule would give another sign somewhere: the restated pmind / pmaxd are observable on the
    signed_zero channel (what the sign IS is the restatement's, pinned on the device)"""
    signs = set()
    for G, C, rot, part, named in named_tables():
        for ch, name in named.items():
            if name == 'signed_zero' and G > 1:
                s = R.combine_ref(part[:, :, ch:ch + 1], 1, seg=R.mseg_of(G, C))[1]
                signs.add((bool(np.signbit(s[R.STAT_MIN, 0])), bool(np.signbit(s[R.STAT_MAX, 0]))))
    assert len(signs) > 1, signs                   # both outcomes occur: the sign follows the records' positions


def test_pass_b_named_channels():
    seen = set()
    for G, C in ((1, 3), (3, 65), (17, 513), (65, 1031)):
        for rot in (0, 1, 2, 3):
            part2, mom, named = R.dev_records(G, C, 5 + G, rot)
            sentinel = np.full((R.NSTAT, C), 77., dtype=F32)
            for want_kurt in (0, 1):
                dev, stats = R.combine_dev_ref(part2, mom, want_kurt, sentinel)
                keep = [r for r in range(R.NSTAT) if r not in ((R.STAT_B, R.STAT_KURT) if want_kurt else (R.STAT_B,))]
                assert (stats[keep] == 77).all()
                for ch, name in named.items():
                    seen.add(name)
                    if name == 'count_zero':
                        assert stats[R.STAT_B, ch] == np.inf
                    elif name == 'count_zero_sum_zero':
                        assert np.isnan(stats[R.STAT_B, ch])
                    elif name == 'z4_nan_without_kurt':
                        assert np.isnan(dev[R.DEV_Z4, ch]) and np.isfinite(stats[R.STAT_B, ch])
                        assert stats[R.STAT_B, ch] == F32(part2[:, R.DEV_ABS, ch].sum() / mom[R.MOM_COUNT, ch])
                        assert np.isnan(stats[R.STAT_KURT, ch]) if want_kurt else stats[R.STAT_KURT, ch] == 77
                    elif name == 'kurt_minus_3' and want_kurt:
                        assert stats[R.STAT_KURT, ch] == -3
    assert seen == set(R.DEV_NAMES)


# ------------------------------------------------------------------------------------------ the order test has teeth
@pytest.mark.parametrize('G,C', [(G, C) for G, C in PAIRS if G >= 16 and C >= 63])
def test_the_order_of_addition_is_observable(G, C):
    """a condition on the inputs, not a measurement: under each order a slip could take instead (R.alternatives), at least
    ORDER_MIN_CHANNELS channels of the very table the GPU test uses change the bits of SUM or SUMSQ.  If a seed does not clear
    it, change the seed (R.ordered_seed), never the bound."""
    part = R.ordered_records(G, C, R.ordered_seed(G, C))
    alts = R.alternatives(G, C)
    assert alts
    for seg, ascending in alts:
        n = R.order_sensitive_channels(part, G, C, seg, ascending)
        assert n >= R.ORDER_MIN_CHANNELS, (G, C, seg, ascending, n)
    part2, _, _ = R.dev_records(G, C, R.ordered_seed(G, C))
    own = R.merge_col(part2, R.mseg_of(G, C), rows_min=(), rows_max=())
    for seg, ascending in alts:
        alt = R.merge_col(part2, seg, rows_min=(), rows_max=(), ascending=ascending)
        assert int((own.view(np.uint64) != alt.view(np.uint64)).any(0).sum()) >= R.ORDER_MIN_CHANNELS, (G, C, seg, ascending)


def test_the_orders_left_out_are_the_same_order():
    """R.alternatives leaves out 8 against 64 lanes with G <= 16, and the reversed tree of one lane: term for term the same sums"""
    for G in (2, 15, 16):
        part = R.ordered_records(G, 70, 3)
        assert R.same_bits64(R.combine_ref(part, 1, seg=8)[0], R.combine_ref(part, 1, seg=64)[0])
    part = R.ordered_records(17, 70, 3)
    assert not R.same_bits64(R.combine_ref(part, 1, seg=8)[0], R.combine_ref(part, 1, seg=64)[0])
    part = R.ordered_records(16, 70, 3)
    assert R.same_bits64(R.combine_ref(part, 1, seg=1)[0], R.combine_ref(part, 1, seg=1, ascending=True)[0])
