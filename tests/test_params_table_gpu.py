"""cnnq_pc_params (k_params: bit_alloc_block + channel_params) on hand-built statistics tables - what `-sm use` feeds it -
against tests/_params.params_ref (the oracle's own pieces, pinned by test_params_table_cpu.py): all of qp and diag, bit for
bit.  Channel counts around every path of bit_alloc_block (one wave, ragged waves, 1024 threads, the 4096 channels kept in
registers, the recompute loop beyond), both priors, round / ceil, clamped targets, every clip mode on the statistics that
decide its branches, NaN / inf statistics, and the non-finite prior.  Bit-allocation inputs come from the
guarded list of _params (margin 2e-5 to a rounding boundary, computed from the reference).  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import _params as P
from cnn_quantization_amd import _lib as L

pytestmark = pytest.mark.gpu

NAMES = ('scale', 'zp', 'qmax', 'bits', 'alpha', 'delta', 'offset')


@pytest.fixture(scope='module')
def ops():
    from cnn_quantization_amd import ops as _ops
    return _ops


def run(ops, table, *args):
    """ops.pc_params -> the seven rows in params_ref's order."""
    qp, diag = ops.pc_params(table.cuda(), *args)
    qp, diag = qp.cpu().numpy(), diag.cpu().numpy()
    return (qp[L.QP_SCALE], qp[L.QP_ZP], qp[L.QP_QMAX], diag[L.DIAG_BITS], diag[L.DIAG_ALPHA], diag[L.DIAG_DELTA],
            diag[L.DIAG_OFFSET])


def check(got, want, what, names=None):
    for nm, a, b in zip(NAMES, got, want):
        if not P.same_bits(a, b):
            i, x, y = P.first_diff(a, b)
            ch = names[i] if names else i
            raise AssertionError('%s: %s of channel %s is %r, the reference has %r' % (what, nm, ch, x, y))


def ba_table(prior, gen):
    """A table whose STD and B rows both hold `prior` (each configuration reads one of them as the prior, the Laplace clip the
    other as b) under ordinary extrema."""
    C = prior.numel()
    mean = torch.randn(C, generator=gen) * 0.2
    return P.make_table(C, mean - 1 - torch.rand(C, generator=gen), mean + 1 + torch.rand(C, generator=gen), mean, prior, prior)


@pytest.mark.parametrize('C', sorted({c[0] for c in P.ba_cases()}))
def test_bit_allocation_channel_counts(ops, C):
    assert C in (1, 2, 63, 64, 65, 1000, 1024, 1025, 4096, 4097, 6000)
    gen = torch.Generator().manual_seed(C)
    for c, target, rnd, seed in P.ba_cases():
        if c != C:
            continue
        table = ba_table(P.guarded_prior(C, seed), gen)
        for prior_is_b in (False, True):
            for clip, positive in (('laplace', False), ('no', True)):
                args = (4, positive, clip, True, prior_is_b, target, rnd, False)
                check(run(ops, table, *args), P.params_ref(table, *args), (C, target, rnd, seed, prior_is_b, clip))


@pytest.mark.parametrize('C', [65, 6000])
def test_targets_that_clamp_every_channel(ops, C):
    table = ba_table(P.guarded_prior(C, 0), torch.Generator().manual_seed(C))
    for target, want in ((40, 8.), (-40, 0.)):
        for rnd in (True, False):
            args = (4, False, 'laplace', True, False, target, rnd, False)
            got = run(ops, table, *args)
            assert bool((got[3] == want).all()), (target, rnd)
            check(got, P.params_ref(table, *args), (C, target, rnd))
    # 0 bits: qmax 0, the scale at its floor and zp = rint(-offset / 1e-8)
    assert bool((got[2] == 0.).all()) and bool((got[0] == np.float32(1e-8)).all())
    assert P.same_bits(got[1], np.rint(np.float32(0.) - got[6] / np.float32(1e-8)))


def test_recompute_loop_channels_permute(ops):
    """C = 6000 with every varied channel at an index >= 4096 (the recompute loop that writes bits_ws inside the iteration),
    and the same prior reversed so that they sit in the register slots: the same bits, reversed."""
    hi = P.hi_prior(P.HI_SEED)
    gen = torch.Generator().manual_seed(1)
    t_hi = ba_table(hi, gen)
    t_lo = t_hi.flip(1).contiguous()
    for target, rnd in P.BA_COMBOS:
        args = (4, False, 'laplace', True, False, target, rnd, False)
        a, b = run(ops, t_hi, *args), run(ops, t_lo, *args)
        assert len(set(a[3][4096:].tolist())) > 2, 'the varied channels must sit beyond 4096'
        check(a, P.params_ref(t_hi, *args), ('hi', target, rnd))
        check(b, P.params_ref(t_lo, *args), ('lo', target, rnd))
        for nm, x, y in zip(NAMES, a, b):
            assert P.same_bits(x, y[::-1]), (nm, target, rnd)


@pytest.mark.parametrize('clip', ['no', 'laplace', 'gaus', '2std', '0.5std'])
def test_clip_modes_on_edge_rows(ops, clip):
    table = P.edge_table()
    for positive in (False, True):
        for direct in (False, True):
            for nb in range(2, 9):
                args = (nb, positive, clip, False, False, None, True, direct)
                check(run(ops, table, *args), P.params_ref(table, *args), (clip, positive, direct, nb), P.EDGE_NAMES)
            for nb, rnd in P.EDGE_BA:
                for prior_is_b in (False, True):
                    args = (nb, positive, clip, True, prior_is_b, None, rnd, direct)
                    got = run(ops, table, *args)
                    check(got, P.params_ref(table, *args), (clip, positive, direct, nb, 'ba', rnd, prior_is_b), P.EDGE_NAMES)
                    z = P.EDGE_NAMES.index('zero_bits')
                    assert got[3][z] == 0. and got[2][z] == 0. and got[0][z] == np.float32(1e-8)
                    assert got[1][z] == np.rint(np.float32(0.) - got[6][z] / np.float32(1e-8))


NONFINITE = [(3, P.STAT_MIN, 'nan'), (10, P.STAT_MAX, 'nan'), (17, P.STAT_MEAN, 'nan'), (24, P.STAT_STD, 'nan'), (31, P.STAT_B, 'nan'),
             (38, P.STAT_MAX, 'inf'), (45, P.STAT_MIN, '-inf'), (52, P.STAT_STD, 'inf'), (59, P.STAT_MEAN, '-inf'),
             (62, P.STAT_MEAN, 'inf'), (66, P.STAT_B, 'inf')]


@pytest.mark.parametrize('clip', ['no', 'laplace', 'gaus', '2std'])
def test_nonfinite_statistics_in_single_channels(ops, clip):
    """Without bit allocation the channels are independent: a NaN / inf statistic gives that channel what the oracle's
    arithmetic gives (np.maximum and torch.max propagate NaN), every other channel what the clean table gives."""
    C = 70
    gen = torch.Generator().manual_seed(4)
    clean = ba_table(P.guarded_prior(C, 5), gen)
    clean[P.STAT_B] = clean[P.STAT_STD] * 0.8
    dirty = clean.clone()
    for c, row, v in NONFINITE:
        dirty[row, c] = float(v)
    hit = np.zeros(C, dtype=bool)
    hit[[c for c, _, _ in NONFINITE]] = True
    for positive in (False, True):
        for direct in (False, True):
            for nb in (2, 4, 8):
                args = (nb, positive, clip, False, False, None, True, direct)
                got = run(ops, dirty, *args)
                check(got, P.params_ref(dirty, *args), (clip, positive, direct, nb))
                for nm, a, b in zip(NAMES, got, run(ops, clean, *args)):
                    assert P.same_bits(a[~hit], b[~hit]), (nm, clip, positive, direct, nb)


@pytest.mark.parametrize('prior_is_b', [False, True])
@pytest.mark.parametrize('kind', ['zero', 'nan', 'inf'])
def test_nonfinite_prior(ops, kind, prior_is_b):
    """The reference raises here (int(nan) when it looks up the Laplace factor).  The library's choice, DESIGN.md 3 - a NaN
    prior must not poison channels whose own statistics are fine (tests/test_aciq_single_gpu.py pins that end to end): NaN
    bits stay NaN in diag and give a NaN qmax; the Laplace factor is the 0-bit one, taken by a range check; the scale is the
    1e-8 floor, as torch.where(qmax > 0, ...) gives on a NaN qmax; after one +inf prior the finite channels get 0 bits."""
    C, j = 200, 77
    gen = torch.Generator().manual_seed(6)
    table = ba_table(P.guarded_prior(C, 0), gen)
    table[P.STAT_B] = table[P.STAT_STD] * 0.8
    row = P.STAT_B if prior_is_b else P.STAT_STD
    if kind == 'zero':
        table[row] = 0.
    else:
        table[row, j] = float(kind)
    dead = np.ones(C, dtype=bool) if kind != 'inf' else (np.arange(C) == j)
    for positive in (False, True):
        for rnd in (True, False):
            for clip in ('laplace', 'no'):
                args = (4, positive, clip, True, prior_is_b, None, rnd, False)
                scale, zp, qmax, bits, alpha, delta, offset = got = run(ops, table, *args)
                what = (kind, prior_is_b, positive, rnd, clip)
                for nm, v in (('bits', bits), ('qmax', qmax)):
                    assert bool(np.isnan(v[dead]).all()) and not np.isnan(v[~dead]).any(), (nm, what)
                assert bool((bits[~dead] == 0.).all()) and bool((qmax[~dead] == 0.).all()), what
                # every channel has NaN or 0 bits: the scale at its floor, zp = rint(-offset / 1e-8), the 0-bit Laplace factor
                assert bool((scale == np.float32(1e-8)).all()), what
                assert P.same_bits(zp, np.rint(np.float32(0.) - offset / np.float32(1e-8))), what
                if clip == 'laplace':
                    fac = np.float32(1.86 if positive else 1.05)
                    assert P.same_bits(alpha, table[P.STAT_B].numpy() * fac), what
                else:
                    assert not np.isnan(offset).any() and not np.isnan(delta).any(), what
                check(got, P.params_ref(table, *args), what)


@pytest.mark.parametrize('C', [1, 65, 1000, 1025, 4097])
def test_params_write_only_their_tables(ops, C):
    """qp [3, C] and diag [4, C] inside one arena of sentinels (the C ABI, as other tests call it): bit_alloc_block's final
    write-back runs over 4 * blockDim slots, of which only those below C may be stored."""
    import ctypes
    PAD = 8192
    table = ba_table(P.guarded_prior(C, P.BA_SEEDS[(C, 4, True)]), torch.Generator().manual_seed(C)).cuda()
    arena = torch.full((PAD + L.NQP * C + PAD + L.NDIAG * C + PAD,), -7., device='cuda')
    qp = arena[PAD:PAD + L.NQP * C]
    diag = arena[2 * PAD + L.NQP * C:2 * PAD + (L.NQP + L.NDIAG) * C]
    args = (4, False, 'laplace', True, False, 4, True, False)
    cfg = ops._params_cfg(*args)
    rc = L.load().cnnq_pc_params(ops._ptr(table), C, ctypes.byref(cfg), ops._ptr(qp), ops._ptr(diag), ops._stream(table))
    assert rc == 0
    a = arena.cpu().numpy()
    for lo, hi in ((0, PAD), (PAD + L.NQP * C, 2 * PAD + L.NQP * C), (2 * PAD + (L.NQP + L.NDIAG) * C, a.size)):
        assert bool((a[lo:hi] == -7.).all()), 'a store outside qp / diag, C = %d' % C
    qp, diag = qp.cpu().numpy().reshape(L.NQP, C), diag.cpu().numpy().reshape(L.NDIAG, C)
    got = (qp[L.QP_SCALE], qp[L.QP_ZP], qp[L.QP_QMAX], diag[L.DIAG_BITS], diag[L.DIAG_ALPHA], diag[L.DIAG_DELTA], diag[L.DIAG_OFFSET])
    check(got, P.params_ref(table.cpu(), *args), C)
