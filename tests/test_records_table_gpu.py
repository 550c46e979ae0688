"""The record-merge kernels (csrc/cnnq_stats.hip.h: k_combine, k_combine_dev, k_combine_all and the prologue of k_absdev<RAW>)
against tests/_records.py on hand-built records, DESIGN.md section 15c.

Every comparison is R.same_bits64 / R.same_bits32 on BOTH outputs - the merged record `mom` (float64) and the table `stats`
(float32): NaN in the same places, every other word bit for bit.  There is no tolerance in this file.  test_records_cpu.py pins
the restatement to the reference and proves that every hand-built case has something at stake."""
import ctypes

import numpy as np
import pytest
import torch

import _records as R

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
SENT64, SENT32, PAD = -777.0625, 77.0625, 64      # (no record word, total or result equals either)
EINVAL = -1


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


class Placed:
    """an output of n words as a view inside a larger sentinel-filled buffer: PAD guard words in front and behind"""

    def __init__(self, shape, dtype, sentinel, wanted=True):
        self.shape, self.n, self.sentinel, self.wanted = shape, int(np.prod(shape)), sentinel, wanted
        self.buf = torch.full((self.n + 2 * PAD,), sentinel, dtype=dtype, device='cuda')

    def ptr(self):
        return self.buf[PAD:].data_ptr() if self.wanted else None

    def take(self, what):
        b = host(self.buf)
        assert (b[:PAD] == self.sentinel).all() and (b[PAD + self.n:] == self.sentinel).all(), 'guard words around %s' % what
        if not self.wanted:
            assert (b == self.sentinel).all(), what
            return None
        return b[PAD:PAD + self.n].reshape(self.shape).copy()


def combine(part_d, G, C, has_relu, want_mom=True, want_stats=True, rc_want=0):
    """cnnq_pc_combine itself -> (mom [NMOM, C] or None, stats [NSTAT, C] or None) on the host; the guard words checked"""
    L, _ = mods()
    mom, stats = Placed((R.NMOM, C), torch.float64, SENT64, want_mom), Placed((R.NSTAT, C), torch.float32, SENT32, want_stats)
    rc = L.load().cnnq_pc_combine(part_d.data_ptr() if part_d is not None else None, G, C, has_relu, mom.ptr(), stats.ptr(), stream())
    assert rc == rc_want, rc
    return mom.take('mom'), stats.take('stats')


def combine_dev(part2_d, G, C, mom_d, want_kurt, want_dev=True, want_stats=True, rc_want=0):
    """cnnq_pc_combine_dev itself, the table pre-filled with SENT32 -> (dev [NDEV, C] or None, stats or None)"""
    L, _ = mods()
    out, stats = Placed((R.NDEV, C), torch.float64, SENT64, want_dev), Placed((R.NSTAT, C), torch.float32, SENT32, want_stats)
    rc = L.load().cnnq_pc_combine_dev(part2_d.data_ptr() if part2_d is not None else None, G, C,
                                      mom_d.data_ptr() if mom_d is not None else None, want_kurt, out.ptr(), stats.ptr(), stream())
    assert rc == rc_want, rc
    return out.take('dev_out'), stats.take('stats')


def check(got, want, where):
    same = R.same_bits64 if want.dtype == np.float64 else R.same_bits32
    assert same(got, want), (where, R.first_diff(got, want))


# ------------------------------------------------------------------------------------------ cnnq_pc_combine
def test_every_lane_layout_occurs():
    assert {R.mseg_of(G, C) for G in R.GRID_G for C in R.GRID_C} == set(R.SEGS)
    for C in (511, 512):
        assert [R.mseg_of(G, C) for G in (16, 17, 64, 65)] == ([1, 8, 8, 64] if C == 512 else [64] * 4)


def tables(G, C):
    """(name, part, named): the integer records, then the order-sensitive ones with the named channels at two rotations"""
    yield 'integer', R.integer_records(G, C), {}
    base = R.ordered_records(G, C, R.ordered_seed(G, C))
    for rot in R.ROTATIONS:
        part, named = R.with_named(base, rot + G)
        yield 'ordered rot %d' % rot, part, named


@pytest.mark.parametrize('C', R.GRID_C)
@pytest.mark.parametrize('G', R.GRID_G)
def test_combine_on_hand_built_records(G, C):
    for name, part, named in tables(G, C):
        plain = [c for c in range(C) if c not in named]
        for has_relu in (1, 0):
            where = (G, C, R.mseg_of(G, C), name, has_relu)
            if not has_relu:                        # the rectified rows hold NaN: the kernel must not read them
                part = part.copy()
                part[:, R.MOM_SUM_RELU:] = np.nan
            part_d = dev(part)
            want_mom, want_stats = R.combine_ref(part, has_relu)
            mom, stats = combine(part_d, G, C, has_relu)
            check(mom, want_mom, where + ('mom',))
            check(stats, want_stats, where + ('stats',))
            # the table is written completely: no sentinel left, B and KURT +0.0
            assert not (stats == SENT32).any() and not (mom == SENT64).any(), where
            for row in (R.STAT_B, R.STAT_KURT):
                assert (stats[row].view(np.uint32) == 0).all(), where
            if not has_relu:
                assert (mom[R.MOM_SUM_RELU:].view(np.uint64) == 0).all() and (stats[R.STAT_STD_POS].view(np.uint32) == 0).all(), where
            assert not np.isnan(mom[:, plain]).any() and not np.isnan(stats[:, plain]).any(), where
            if name == 'integer':                   # exact in any order: the sums are numpy's
                assert np.array_equal(mom[R.MOM_SUM:R.MOM_SUM_RELU], part[:, R.MOM_SUM:R.MOM_SUM_RELU].sum(0)), where
                assert np.array_equal(mom[R.MOM_MIN], part[:, R.MOM_MIN].min(0)) and np.array_equal(mom[R.MOM_MAX], part[:, R.MOM_MAX].max(0))
            # either output alone
            only_mom, none = combine(part_d, G, C, has_relu, want_stats=False)
            none2, only_stats = combine(part_d, G, C, has_relu, want_mom=False)
            assert none is None and none2 is None
            check(only_mom, want_mom, where + ('mom alone',))
            check(only_stats, want_stats, where + ('stats alone',))
            for ch, nm in named.items():
                if nm == 'empty_among_full':        # the same channel with the empty records removed, as a table of its own
                    twin = R.empty_twin(part, ch)
                    if not has_relu:
                        twin[:, R.MOM_SUM_RELU:] = np.nan
                    tm, ts = combine(dev(twin), twin.shape[0], 1, has_relu)
                    check(mom[:, ch], tm[:, 0], where + (ch, nm, 'mom'))
                    check(stats[:, ch], ts[:, 0], where + (ch, nm, 'stats'))


def test_combine_refuses_bad_arguments():
    part_d = dev(R.integer_records(2, 4))
    for args in ((None, 2, 4), (part_d, 0, 4), (part_d, 2, 0), (part_d, -1, 4)):
        mom, stats = combine(*args, 1, rc_want=EINVAL)
        assert (mom == SENT64).all() and (stats == SENT32).all(), args[1:]
    assert combine(part_d, 2, 4, 1, want_mom=False, want_stats=False, rc_want=EINVAL) == (None, None)
    torch.cuda.synchronize()


TWO_LEVEL = [(G, C) for G in (2, 3, 16, 17, 64, 65, 130, 256) for C in (5, 65, 512, 1031)]


@pytest.mark.parametrize('G,C', TWO_LEVEL)
def test_two_level_merge(G, C):
    """the sharded route: W consecutive groups merged on their own, their `mom` stacked [W, NMOM, C] as all_gather_records lays
    them out, merged again - `mom` is a valid input record (row layout, extrema as doubles, count)"""
    _, ops = mods()
    integer = R.integer_records(G, C)
    ordered, _ = R.with_named(R.ordered_records(G, C, R.ordered_seed(G, C)), G)
    for name, part in (('integer', integer), ('ordered', ordered)):
        part_d = dev(part)
        one_mom, one_stats = R.combine_ref(part, 1)
        for W in R.TWO_LEVEL_W:
            if W > G:
                continue
            groups = np.array_split(np.arange(G), W)
            moms_d = torch.stack([ops.pc_combine(part_d[int(g[0]):int(g[-1]) + 1], True)[0] for g in groups])
            assert moms_d.shape == (W, R.NMOM, C) and moms_d.is_contiguous()
            mom_d, stats_d = ops.pc_combine(moms_d, True)
            want_moms, (want_mom, want_stats) = R.two_level_ref(part, W, 1)
            where = (G, C, W, name)
            check(host(moms_d), want_moms, where + ('groups',))
            check(host(mom_d), want_mom, where + ('mom',))
            check(host(stats_d), want_stats, where + ('stats',))
            if name == 'integer':
                check(host(mom_d), one_mom, where + ('one level',))
                check(host(stats_d), one_stats, where + ('one level',))


# ------------------------------------------------------------------------------------------ cnnq_pc_combine_dev
@pytest.mark.parametrize('C', R.GRID_C)
@pytest.mark.parametrize('G', R.GRID_G)
def test_combine_dev_on_hand_built_records(G, C):
    sentinel = np.full((R.NSTAT, C), SENT32, dtype=F32)
    for rot in (0, 2):
        part2, mom, named = R.dev_records(G, C, R.ordered_seed(G, C), rot + G)
        part2_d, mom_d = dev(part2), dev(mom)
        for want_kurt in (0, 1):
            where = (G, C, R.mseg_of(G, C), rot, want_kurt)
            want_dev, want_stats = R.combine_dev_ref(part2, mom, want_kurt, sentinel)
            out, stats = combine_dev(part2_d, G, C, mom_d, want_kurt)
            check(out, want_dev, where + ('dev',))
            check(stats, want_stats, where + ('stats',))
            keep = [r for r in range(R.NSTAT) if r != R.STAT_B and not (want_kurt and r == R.STAT_KURT)]
            assert (stats[keep] == SENT32).all(), where          # MIN .. STD, STD_POS - and KURT without want_kurt - untouched
            assert not (stats[R.STAT_B] == SENT32).any()
            only_dev, none = combine_dev(part2_d, G, C, None, want_kurt, want_stats=False)      # the sums alone need no mom
            none2, only_stats = combine_dev(part2_d, G, C, mom_d, want_kurt, want_dev=False)
            assert none is None and none2 is None
            check(only_dev, want_dev, where + ('dev alone',))
            check(only_stats, want_stats, where + ('stats alone',))
            for ch, nm in named.items():
                if nm == 'z4_nan_without_kurt':
                    assert np.isfinite(stats[R.STAT_B, ch]), where
                    assert np.isnan(stats[R.STAT_KURT, ch]) if want_kurt else stats[R.STAT_KURT, ch] == SENT32, where


def test_combine_dev_refuses_bad_arguments():
    part2, mom, _ = R.dev_records(2, 4, 1)
    part2_d, mom_d = dev(part2), dev(mom)
    for args in ((part2_d, 2, 4, None), (None, 2, 4, mom_d), (part2_d, 0, 4, mom_d), (part2_d, 2, 0, mom_d)):
        out, stats = combine_dev(*args, 1, rc_want=EINVAL)
        assert (out == SENT64).all() and (stats == SENT32).all(), args[1:3]
    assert combine_dev(part2_d, 2, 4, mom_d, 1, want_dev=False, want_stats=False, rc_want=EINVAL) == (None, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ the two chains
# (shape, rectified, (G, lanes) the planner must give or None): each lane layout through real plans (the plan words of
# tests/_corrections.py CLASSES)
CHAINS = [((16, 520, 2, 2), False, (16, 1)), ((64, 640, 14, 14), False, (64, 8)), ((4, 16, 14, 14), False, None),
          ((3, 5, 7, 7), False, None), ((2, 3, 33, 35), False, None), ((1, 300, 4, 4), False, None), ((4, 16, 14, 14), True, None),
          ((16, 520, 2, 2), True, (16, 1))]
NEEDS = [(True, False, False), (True, True, False), (True, True, True), (False, False, False)]


@pytest.mark.parametrize('shape,rectified,plan', CHAINS, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) and len(v) == 4 else None)
def test_split_and_fused_chains_agree(shape, rectified, plan):
    """split: pc_moments -> pc_combine -> pc_absdev -> pc_combine_dev (what the collective multi-GPU route runs); fused:
    cnnq_pc_stats (k_moments -> k_absdev<RAW>, whose prologue merges the sums itself -> k_combine_all).  The mean the fused pass B
    subtracts must be bit for bit the mean of the table, so both give the same table and the same record; and each merge of the
    split chain is the restatement's on the chain's own records."""
    _, ops = mods()
    from test_stats_single_gpu import acts
    N, C, H, W = shape
    HW = H * W
    x = acts(shape, 3 + C + HW)
    if rectified:
        x = x.clamp(min=0)
    xd = x.cuda()
    for need_b, need_kurt, need_relu in NEEDS:
        where = (shape, rectified, need_b, need_kurt, need_relu)
        part = ops.pc_moments(xd, N, C, HW, need_relu)
        G = part.shape[0]
        if plan is not None:
            assert (G, R.mseg_of(G, C)) == plan, where          # a planner change must not silently un-test the layout
        else:
            assert R.mseg_of(G, C) == 64
        mom, stats = ops.pc_combine(part, need_relu)
        want_mom, want_stats = R.combine_ref(host(part), int(need_relu))
        check(host(mom), want_mom, where + ('pc_combine mom',))
        check(host(stats), want_stats, where + ('pc_combine stats',))
        assert np.array_equal(want_mom[R.MOM_COUNT], np.full(C, float(N * HW)))
        if need_b or need_kurt:
            part2 = ops.pc_absdev(xd, N, C, HW, stats, need_kurt)
            assert part2.shape[0] == G
            sums = ops.pc_combine_dev(part2, mom, stats, need_kurt, want_sums=True)
            want_dev, want_stats = R.combine_dev_ref(host(part2), want_mom, int(need_kurt), want_stats)
            check(host(sums), want_dev, where + ('pc_combine_dev sums',))
            check(host(stats), want_stats, where + ('pc_combine_dev stats',))
        ops._ACIQ_SINGLE = False
        try:
            fstats, fmom = ops.pc_stats(xd, N, C, HW, need_b=need_b, need_kurt=need_kurt, need_relu=need_relu)
        finally:
            ops.reload_switches()
        check(host(fmom), host(mom), where + ('fused mom',))
        check(host(fstats), host(stats), where + ('fused stats',))
        if C > 2 and need_kurt and not rectified:
            assert np.isnan(host(fstats)[R.STAT_KURT, C // 2])  # the constant channel: 0 * inf
