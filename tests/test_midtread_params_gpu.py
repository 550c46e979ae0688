"""cnnq_pc_midtread_params (k_mt_params: mt_omega_alpha + mt_channel) on hand-built statistics and interpolation tables against
tests/_midtread_params.mt_ref (the oracle's own pieces, pinned by test_midtread_params_cpu.py to the reference's get_omega /
get_alpha_mult): rows OMEGA, ALPHA, DELTA, CMIN, CMAX and WSTART, bit for bit.  Channel counts around every path of the workgroup
reductions (one wave, ragged waves, 1024 threads, the strided loop beyond), both ranges, with and without clipping, integer and
fractional targets, the half-to-even tie; the search at, between, below and beyond the knots on three hand-built tables and the real
one; the statistics that decide each branch of mt_channel, among ordinary channels and alone at C = 1; NaN / inf / constant
tables (the library's choices where the reference raises); the window start at every wave boundary; stores outside
mt; refusals; and the window start of the launches that guess it from the std.  Every input comes from M.gpu_tables(), whose std
vectors are guarded (margin 2e-5 to a rounding boundary).  One workgroup per call.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import _midtread_params as M
from cnn_quantization_amd import _lib as L

pytestmark = pytest.mark.gpu

EINVAL = -1          # CNNQ_EINVAL of include/cnnq_hip.h

TABLES = M.gpu_tables()
REAL = M.real_tables()


@pytest.fixture(scope='module')
def ops():
    from cnn_quantization_amd import ops as _ops
    return _ops


def dev_tabs(tabs):
    return torch.tensor(np.stack([tabs[0], tabs[1]]), dtype=torch.float64, device='cuda')


def run(ops, table, target, clip, sym, tabs=REAL):
    """cnnq_pc_midtread_params through the C ABI -> the six rows in mt_ref's order."""
    st = torch.as_tensor(M.f32(table)).cuda().contiguous()
    C = st.shape[1]
    dt = dev_tabs(tabs)
    mt = torch.full((L.NMT, C), -7., dtype=torch.float32, device='cuda')
    rc = L.load().cnnq_pc_midtread_params(ops._ptr(st), C, float(target), int(clip), int(sym), ops._ptr(dt), dt.shape[1], ops._ptr(mt),
                                          ops._stream(st))
    assert rc == 0
    mt = mt.cpu().numpy()
    return tuple(mt[r] for r in M.ROW_INDEX)


def check(got, want, what, names=None):
    for nm, a, b in zip(M.ROWS, got, want):
        if not M.same_bits(a, b):
            i, x, y = M.first_diff(a, b)
            raise AssertionError('%s: %s of channel %s is %r, the reference has %r' % (what, nm, names[i] if names else i, x, y))


def both(ops, table, target, tabs, what, names=None, clips=(1, 0)):
    for sym in (1, 0):
        for clip in clips:
            check(run(ops, table, target, clip, sym, tabs), M.mt_ref(table, target, clip, sym, *tabs), (what, 'sym', sym, 'clip', clip), names)


# ------------------------------------------------------------------------------------------------ channel counts
@pytest.mark.parametrize('C', sorted({c for c, _ in M.CELLS}))
def test_channel_counts(ops, C):
    """psum over 1024 threads and the fold of the 16 waves' window starts through the reused sh[], at ragged channel counts; (65, 8)
    and (65, 9.5) take omega beyond the last knot."""
    assert C in (1, 2, 63, 64, 65, 1000, 1024, 1025, 4096, 4097, 6000)
    targets = [t for c, t in M.CELLS if c == C]
    assert any(t == int(t) for _, t in M.CELLS) and any(t != int(t) for _, t in M.CELLS)
    for target in targets:
        table, _ = TABLES[('cell', C, target)]
        both(ops, table, target, REAL, (C, target))


def test_half_to_even_tie(ops):
    """B == 5.0f, both priors 1: the quotient is 2.5 exactly -> 2 (rintf), not 3 (roundf).  No powf rounding is involved."""
    for sym in (1, 0):
        for clip in (1, 0):
            got = run(ops, M.tie_table(), M.TIE_TARGET, clip, sym)
            assert got[0].tolist() == [2., 2.]
            check(got, M.mt_ref(M.tie_table(), M.TIE_TARGET, clip, sym, *REAL), ('tie', sym, clip))


# ------------------------------------------------------------------------------------------------ the search and the interpolation
@pytest.mark.parametrize('name', sorted(M.HAND))
def test_hand_built_interpolation_tables(ops, name):
    """searchsorted(side='left') at a knot, between knots, below the first knot (numpy's wrap to the last entry) and beyond the last
    (the library's extrapolation); the doubled omega of the non-negative range leaves the table at half the omega.  Table C tells
    side='left' from side='right', which agree wherever the arithmetic is exact."""
    tabs, omegas, values = M.HAND[name]
    table, target = TABLES[name]
    both(ops, table, target, tabs, name, names=omegas)
    got = run(ops, table, target, 1, 1, tabs)
    assert got[0].tolist() == [float(k) for k in omegas]
    for k, want in values.items():                                             # the values worked out by hand
        assert got[1][omegas.index(k)] == np.float32(want), (k, want)
    got = run(ops, table, target, 1, 0, tabs)
    for k, want in values.items():
        if k % 2 == 0 and k // 2 in omegas:
            assert got[1][omegas.index(k // 2)] == np.float32(want), (k, want)


@pytest.mark.parametrize('sym', [1, 0])
def test_real_table_every_reachable_segment(ops, sym):
    """One omega in every segment of the 101-entry table an integer can reach (an even one for the doubled form), every integer
    knot, omega 0 and two beyond 955."""
    table, target = TABLES[('real', bool(sym))]
    omegas = M.omegas_covering(bool(sym), REAL[0])
    both(ops, table, target, REAL, ('real', sym), names=omegas)
    assert run(ops, table, target, 1, sym)[0].tolist() == [float(k) for k in omegas]


# ------------------------------------------------------------------------------------------------ edge statistics
def test_edge_statistics_among_ordinary_channels(ops):
    table, target = TABLES['edge']
    both(ops, table, target, REAL, 'edge', names=M.EDGE_NAMES)
    both(ops, table, target, M.HAND_B, 'edge on table B', names=M.EDGE_NAMES)
    got = dict(zip(M.ROWS, run(ops, table, target, 1, 1)))
    z = M.EDGE_NAMES.index('std0')
    assert got['omega'][z] == 0 and got['delta'][z] == np.float32(M.F32_MAX)
    assert got['cmin'][z] == got['cmax'][z] == np.float32(0.3) / np.float32(M.F32_MAX)


@pytest.mark.parametrize('row', M.ORD_ROWS + M.EDGE_ROWS, ids=lambda r: r[0])
def test_edge_statistics_alone(ops, row):
    """C = 1, the per-tensor form cnnq_pt_midtread uses: omega == 2^target, the row's own bound is the window start."""
    table, target = TABLES[('single', row[0])]
    both(ops, table, target, REAL, row[0])


@pytest.mark.parametrize('name, value', M.POISON_STD)
def test_one_std_changes_every_channel(ops, name, value):
    """A NaN or negative std poisons the sum, as in the reference: every channel gets what mt_ref says (NaN omega, NaN multiplier,
    Delta = FLT_MAX); +inf leaves the others 0 bins; a huge finite one takes them all."""
    table, target = TABLES[('poison', name)]
    both(ops, table, target, REAL, name)
    got = run(ops, table, target, 1, 1)
    if name in ('std_nan', 'std_neg'):
        assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and bool((got[2] == np.float32(M.F32_MAX)).all())
    table, target = TABLES[('poison1', name)]
    both(ops, table, target, REAL, name + ' alone')


@pytest.mark.parametrize('C', [1, 2, 65, 1025])
def test_all_channels_constant(ops, C):
    """psum == 0: the reference raises IndexError (omega is 0 / 0); the library writes NaN omega / multiplier / bounds, Delta =
    FLT_MAX and the clamped window start."""
    table, target = TABLES[('constant', C)]
    both(ops, table, target, REAL, ('constant', C))
    got = dict(zip(M.ROWS, run(ops, table, target, 1, 1)))
    assert np.isnan(got['omega']).all() and np.isnan(got['alpha']).all() and np.isnan(got['cmin']).all() and np.isnan(got['cmax']).all()
    assert bool((got['delta'] == np.float32(M.F32_MAX)).all()) and bool((got['wstart'] == -65536).all())


# ------------------------------------------------------------------------------------------------ WSTART
@pytest.mark.parametrize('C', sorted(M.WSTART_SLOTS))
def test_window_start_from_every_wave(ops, C):
    """The channel holding the smallest clamp bound at the ends of the first wave, of the workgroup and of the strided loop; C = 63:
    fifteen waves hold no channel.  The non-negative range: exactly 0; no clipping: -CNNQ_MT_HIST_WINDOW / 2."""
    for slot in M.WSTART_SLOTS[C]:
        table, target = TABLES[('wstart', C, slot)]
        want = M.mt_ref(table, target, 1, 1, *REAL)
        got = run(ops, table, target, 1, 1)
        check(got, want, ('wstart', C, slot))
        assert got[5][0] == np.floor(want[3][slot]) and bool((got[5] == got[5][0]).all())
        assert bool((run(ops, table, target, 1, 0)[5] == 0).all())
        assert bool((run(ops, table, target, 0, 1)[5] == -L.MT_HIST_WINDOW // 2).all())


@pytest.mark.parametrize('kind', ['clamp', 'nan', 'ninf'])
def test_window_start_bounds(ops, kind):
    """A bound below -CNNQ_MT_HIST_BINS / 2, a NaN bound (counts as -1e9) and a -inf bound, each in one channel of 1025."""
    table, target = TABLES[('wstart', kind)]
    got = run(ops, table, target, 1, 1)
    check(got, M.mt_ref(table, target, 1, 1, *REAL), ('wstart', kind))
    assert bool((got[5] == -L.MT_HIST_BINS // 2).all())


# ------------------------------------------------------------------------------------------------ stores, refusals
@pytest.mark.parametrize('C', [1, 65, 1000, 1025, 4097])
def test_params_write_only_their_table(ops, C):
    """mt [6, C] inside one arena of sentinels; the statistics table and the interpolation tables come back unchanged."""
    PAD = 8192
    table, target = TABLES[('cell', C, 4)]
    st = table.cuda().contiguous()
    dt = dev_tabs(REAL)
    st0, dt0 = st.clone(), dt.clone()
    arena = torch.full((PAD + L.NMT * C + PAD,), -7., device='cuda')
    mt = arena[PAD:PAD + L.NMT * C]
    for clip, sym in ((1, 1), (1, 0), (0, 1)):
        rc = L.load().cnnq_pc_midtread_params(ops._ptr(st), C, float(target), clip, sym, ops._ptr(dt), dt.shape[1], ops._ptr(mt), ops._stream(st))
        assert rc == 0
        a = arena.cpu().numpy()
        assert bool((a[:PAD] == -7.).all()) and bool((a[PAD + L.NMT * C:] == -7.).all()), 'a store outside mt, C = %d' % C
        assert torch.equal(st.view(torch.int32), st0.view(torch.int32)) and torch.equal(dt.view(torch.int64), dt0.view(torch.int64))
        got = mt.cpu().numpy().reshape(L.NMT, C)
        check(tuple(got[r] for r in M.ROW_INDEX), M.mt_ref(table, target, clip, sym, *REAL), (C, clip, sym))


def test_refusals_write_nothing(ops):
    """ntab < 2, null pointers, C <= 0 and C >= 2^31: CNNQ_EINVAL and no store."""
    C = 65
    table, target = TABLES[('cell', C, 4)]
    st = table.cuda().contiguous()
    dt = dev_tabs(REAL)
    mt = torch.full((L.NMT, C), -7., device='cuda')
    fn = L.load().cnnq_pc_midtread_params
    s = ops._stream(st)
    calls = [(ops._ptr(st), C, ops._ptr(dt), 1, ops._ptr(mt)), (ops._ptr(st), C, ops._ptr(dt), 0, ops._ptr(mt)),
             (ops._ptr(st), C, ops._ptr(dt), -3, ops._ptr(mt)), (None, C, ops._ptr(dt), 101, ops._ptr(mt)),
             (ops._ptr(st), C, None, 101, ops._ptr(mt)), (ops._ptr(st), C, ops._ptr(dt), 101, None),
             (ops._ptr(st), 0, ops._ptr(dt), 101, ops._ptr(mt)), (ops._ptr(st), -5, ops._ptr(dt), 101, ops._ptr(mt)),
             (ops._ptr(st), 1 << 31, ops._ptr(dt), 101, ops._ptr(mt)), (ops._ptr(st), (1 << 40) + C, ops._ptr(dt), 101, ops._ptr(mt))]
    for stp, c, tp, ntab, mp in calls:
        assert fn(stp, c, float(target), 1, 1, tp, ntab, mp, s) == EINVAL, (c, ntab)
    torch.cuda.synchronize()
    assert bool((mt == -7.).all())
    assert fn(ops._ptr(st), C, float(target), 1, 1, ops._ptr(dt), 2, ops._ptr(mt), s) == 0          # ntab == 2 is a table


# ------------------------------------------------------------------------------------------------ the <GUESS> window start
def check_guessed_window(parts, target, guessed):
    """Row WSTART of a launch's published mt against mt_ref on its published statistics table - with b replaced by std *
    0.70710678f where the launch computes the window before b is known.  The published std is the device's own reduction, so the
    guard is asserted on it here."""
    st = parts['stats'].cpu()
    assert M.omega_margin(st[M.STAT_STD], target) > M.MARGIN
    want = M.mt_ref(M.with_guess_b(st) if guessed else st, target, 1, True, *REAL)
    w = parts['mt'][L.MT_WSTART].cpu().numpy()
    assert M.same_bits(w, want[5]), (w[0], want[5][0])
    assert M.same_bits(parts['mt'][L.MT_OMEGA].cpu(), want[0])
    return want


def test_guessed_window_start_fp32_single_launch(ops):
    from test_midtread_single_gpu import acts
    N, C, H, W = shape = (6, 3, 64, 64)
    xd = acts(shape, 11 + C + H * W, relu=False).cuda()
    ops.group_status(xd, clear=True)
    res = ops.mid_tread_qdq_single(xd, N, C, H * W, 4, True, ops._midtread_tables(xd.device), want_entropy=True, want_parts=True)
    assert res is not None
    want = check_guessed_window(res[2], 4, True)
    assert want[5][0] < 0 and ops.group_status(xd) == 0


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_guessed_window_start_half_whole_channel_route(ops, dtype):
    from test_half_collect_gpu import half
    from test_half_midtread_gpu import route
    import _half_collect as HC
    shape = (3, 6, 7, 14)                                                       # the smallest resident case of tests/_half_aciq.py
    x = half(HC.values(shape, HC.seed_of(shape, 0)), dtype, 0)
    assert route(x, True, 2)[3] == 3
    _, _, parts = ops.mid_tread_qdq_half(x, 5.3, True, want_entropy=True, want_parts=True, single_launch=2)
    want = check_guessed_window(parts, 5.3, True)
    assert want[5][0] < 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_window_start_channels_last(ops, dtype):
    """The channels_last form knows b before it allocates (cnnq_pc_midtread_nhwc runs k_mt_params on the finished table): its
    window start is mt_ref's on the published table as it stands."""
    from test_channels_last_gpu import cl, values
    for shape in ((1, 3, 1, 2), (3, 5, 7, 9)):
        x = cl(values(shape, seed=4), dtype, 0)
        _, _, parts = ops.mid_tread_qdq_nhwc(x, 4, True, want_entropy=True, want_parts=True)
        check_guessed_window(parts, 4, False)
