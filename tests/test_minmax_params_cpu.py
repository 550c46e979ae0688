"""tests/_minmax_params.py pinned to the oracle, and its table of named channels shown to have teeth: what
test_minmax_params_table_gpu.py holds the kernels to is the reference's arithmetic, the builder keeps its promise in all three
dtypes, every named channel has at stake what its name says, and every slip a hand-written copy of the arithmetic could hold
changes the bits of at least one of them.  Bit for bit: no tolerance in this file."""
import numpy as np
import pytest
import torch

import _minmax_params as M
from oracle import quant_oracle as O

F32 = np.float32
SHAPES = [(3, 8, 7, 7), (2, 8, 14, 14), (5, 3, 28, 28), (4, 260, 1, 4), (1, 1100, 2, 2)]


def named(mode, dtype=torch.float32):
    return {n: (a, b) for n, a, b in M.table(mode, dtype)}


def one(mode, name):
    a, b = named(mode)[name]
    sc, zp, qm = M.params_ref([a], [b], mode[0], mode[1])
    return a, b, sc[0], zp[0], qm


# ------------------------------------------------------------------------------------------ the restatement is the reference's
@pytest.mark.parametrize('shape', SHAPES[:3], ids=str)
@pytest.mark.parametrize('mode', M.MODES, ids=str)
def test_restatement_equals_oracle_on_builder_tensors(mode, shape):
    _, positive = mode
    rows = M.mixed(mode)
    for k, win in enumerate(M.windows(rows, shape[1])):
        x, mn, mx = M.window_tensor(shape, win, 100 + k)
        for bits in (2, 4, 8, mode[0]):
            sc, zp, qm = M.params_ref(mn, mx, bits, positive)
            y, parts = O.act_per_channel_qdq(x, bits, half_range=positive, return_parts=True)
            where = (mode, shape, k, bits, [w[0] for w in win])
            assert M.same_bits(parts['scale'].numpy(), sc), where
            assert M.same_bits(parts['zero_point'].numpy(), zp), where
            assert float(qm) == float(F32(parts['qmax']))
            ry, rq = M.qdq_ref(x.numpy(), sc, zp, qm)
            assert M.same_bits(ry, y.numpy()), (where, M.first_diff(ry, y.numpy()))
            assert M.same_bits(rq, parts['codes'].numpy()), where
            # the same through qdq_core on channel rows, with the table's extrema handed in
            off = np.zeros_like(mn) if positive else mn
            with np.errstate(all='ignore'):
                delta = mx - off
            y2, _, sc2, zp2, _ = O.qdq_core(x.transpose(0, 1).reshape(shape[1], -1), torch.from_numpy(delta), torch.from_numpy(off),
                                            num_bits=bits, return_parts=True)
            assert M.same_bits(sc2.numpy(), sc) and M.same_bits(zp2.numpy(), zp), where
            assert M.same_bits(y2.view(shape[1], shape[0], *shape[2:]).transpose(0, 1).numpy(), ry), where


def test_restatement_equals_the_reference_made_fixture(golden):
    """tests/golden/act_pc.npz was written by the reference itself: its config-2 floats, and its scale / zero point where it holds them"""
    g = golden('act_pc')
    n = held = 0
    for key in g.np('names'):
        key = str(key)
        name, si = key.rsplit('_s', 1)
        if not name.startswith('cfg2') or 'baa' in name:
            continue
        x = g.np('x' + si)
        bits, half = int(g.np(key + '_bits')), bool(g.np(key + '_half'))
        t = torch.from_numpy(x).transpose(0, 1).reshape(x.shape[1], -1)
        mn, mx = t.min(1)[0].numpy(), t.max(1)[0].numpy()
        sc, zp, qm = M.params_ref(mn, mx, bits, half)
        y, _ = M.qdq_ref(x, sc, zp, qm)
        assert M.same_bits(y, g.np(key + '_y')), key
        for word, mine in (('_scale', sc), ('_zero_point', zp), ('_zp', zp)):
            if key + word in g:
                assert M.same_bits(g.np(key + word).reshape(-1), mine), (key, word)
                held += 1
        n += 1
    assert n >= 12
    print('act_pc.npz: %d config-2 cases, %d parameter rows held by the fixture' % (n, held))


# ------------------------------------------------------------------------------------------ the builder keeps its promise
@pytest.mark.parametrize('dtype', list(M.DTYPES), ids=str)
@pytest.mark.parametrize('shape', SHAPES + [(9, 4, 56, 56)], ids=str)
def test_builder_holds_the_table(shape, dtype):
    dt = M.DTYPES[dtype]
    N, C, H, W = shape
    for mode in M.MODES:
        rows = M.mixed(mode, dt)
        for n, a, b in rows:                                # the sub-tables cast exactly
            for v in (a, b):
                back = torch.tensor([float(v)]).to(dt).float().numpy()
                assert v != v or back.view(np.uint32)[0] == np.array([v], dtype=F32).view(np.uint32)[0], (n, dtype)
        for k, win in enumerate(M.windows(rows, C)):
            x, mn, mx = M.window_tensor(shape, win, 7 * k + C, dt)
            assert x.dtype == dt and x.is_contiguous() and tuple(x.shape) == shape
            xf = x.float().numpy().reshape(N, C, H * W)
            for c in range(C):
                ch, name = xf[:, c], win[c][0]
                if mn[c] != mn[c]:
                    assert np.isnan(ch).sum() == 1 and np.nanmin(ch) > -1 and np.nanmax(ch) < 1, name
                    continue
                assert M.same_bits(ch.min(), mn[c]) and M.same_bits(ch.max(), mx[c]), (name, dtype)
                pa, pb = M.place(shape, c)
                if mn[c] == mx[c]:
                    assert (ch.view(np.uint32) == ch.view(np.uint32)[0, 0]).all(), name
                    continue
                assert (ch == mn[c]).sum() == 1 and (ch == mx[c]).sum() == 1, name
                assert M.same_bits(ch[pa], mn[c]) and M.same_bits(ch[pb], mx[c]) and pa != pb, name
                assert np.isfinite(np.delete(ch.reshape(-1), [pa[0] * H * W + pa[1], pb[0] * H * W + pb[1]])).all(), name
                if N * H * W > 4:
                    addr = lambda p: (p[0] * C + c) * H * W + p[1]        # noqa: E731
                    assert addr(pa) // 4 != addr(pb) // 4, (name, pa, pb)
    # the six places occur, and the ragged ones are what they say
    pos = M.positions(N, H * W)
    assert {M.place(shape, c)[0] for c in range(min(C, 6))} == set(pos[:min(C, 6)])
    assert pos[1] == (N - 1, H * W - 1) and pos[4][1] == H * W - 1
    if N * H * W > 1024:
        assert (pos[5][0] * H * W + pos[5][1] + 1) % 1024 == 0


# ------------------------------------------------------------------------------------------ every name has something at stake
def test_named_channels_have_at_stake_what_they_say():
    with np.errstate(all='ignore'):
        for mode in ((4, False), (4, True)):
            qm = M.qmax_ref(4)
            below, at, above = (named(mode)['floor_' + w] for w in ('below', 'at', 'above'))
            raw = [F32(F32(b - (0 if mode[1] else a)) / qm) for a, b in (below, at, above)]
            assert raw[0] == np.nextafter(M.FLOOR, F32(0)) and raw[1] == M.FLOOR and raw[2] > M.FLOOR, raw
            # the float just above the floor is no float32 divided by 15: floor_above is the smallest scale above it that 4 bits reach
            d_at, d_above = (F32(b - (0 if mode[1] else a)) for a, b in (at, above))
            assert np.nextafter(d_at, F32(1)) == d_above
            assert [one(mode, 'floor_' + w)[2] for w in ('below', 'at', 'above')] == [M.FLOOR, M.FLOOR, raw[2]]
        F = (4, False)
        for name, q, even, away in (('tie_down', 1.5, 2.0, 2.0), ('tie_up', 2.5, 2.0, 3.0)):
            a, b, sc, zp, _ = one(F, name)
            assert sc == 1.0 and F32(0) - a / sc == q and zp == even, name
            assert M.params_mutant('round_half_away', [a], [b], 4, False)[1][0] == away
        a, b, sc, zp, _ = one(F, 'neg_zero_zp')
        assert 0 < a < sc / 4 and zp == 0 and np.signbit(zp)
        a, b, sc, zp, _ = one(F, 'overflow')
        assert np.isfinite(a) and np.isfinite(b) and np.isinf(F32(b - a)) and np.isinf(sc) and zp == 0 and not np.signbit(zp)
        assert one(F, 'const_quarter')[2:4] == (M.FLOOR, F32(-25000000.0))
        a, b, sc, zp, _ = one(F, 'const_2p70')
        assert sc == M.FLOOR and zp < -1e29 and M.fast_domain_ref(a, b, sc)
        a, b, sc, zp, _ = one((4, True), 'neg_under_positive')
        assert b < 0 and sc == M.FLOOR and zp == 0 and not np.signbit(zp)
        a, b, sc, zp, _ = one(F, 'denormal')
        assert 0 < b < 2.0 ** -126 and sc == M.FLOOR and zp == 0
        for mode, stem in (((4, False), 'scale_%s_2p30'), ((4, True), 'scale_%s_2p30'), ((32, False), 'abs_%s_2p70'),
                           ((32, False), 'neg_abs_%s_2p70')):
            at, above = (one(mode, stem % w) for w in ('at', 'above'))
            assert M.fast_domain_ref(at[0], at[1], at[2]) and not M.fast_domain_ref(above[0], above[1], above[2]), (mode, stem)
            if 'scale' in stem:
                assert at[2] == M.P30 and M.P30 < above[2] < M.P30 * F32(1.01)      # (one bfloat16 step of the maximum above)
            else:
                assert max(abs(at[0]), abs(at[1])) == M.P70 and max(abs(above[0]), abs(above[1])) == np.nextafter(M.P70, F32(np.inf))
        for mode in M.MODES:
            fast, slow = M.split(mode)
            assert len(fast) >= 4 and len(slow) >= 2, mode
            slow_names = {r[0] for r in slow}
            assert {'pinf', 'nan'} <= slow_names and not any('_above_' in r[0] for r in fast) and not any('_at_' in n for n in slow_names)
            for dt in (torch.bfloat16, torch.float16):
                assert len(M.split(mode, dt)[0]) >= 2 and len(M.split(mode, dt)[1]) >= 2, (mode, dt)
        assert {'tie_down', 'tie_up', 'neg_zero_zp', 'const_2p70', 'scale_at_2p30', 'denormal'} <= set(named((4, False), torch.bfloat16))
        assert {'tie_down', 'tie_up', 'neg_zero_zp', 'const_quarter'} <= set(named((4, False), torch.float16))


# ------------------------------------------------------------------------------------------ the table has teeth
def test_every_mutant_changes_a_named_channel(capsys):
    """A condition, not a measurement: each slip a hand-written copy could hold changes the bits of at least one named channel in
    the mode where the GPU file runs it.  Two of the list are no slips and are asserted to be none: `<=` for `<` in the floor's
    select (at equality both arms are f32(1e-8)) and qmax from an exact float32 powf (2^b is exact, and 2^b - 1 rounds to the same
    float in one step or two, at every width 1 .. 32); `(1 << bits) - 1` in an int stands in for the latter."""
    lines = []
    for kind in M.PARAM_MUTANTS:
        caught = []
        for mode in M.MODES:
            for n, a, b in M.table(mode):
                ref = M.params_ref([a], [b], *mode)
                mut = M.params_mutant(kind, [a], [b], *mode)
                if not all(M.same_bits(r, m) for r, m in zip(ref, mut)):
                    caught.append('%s@%d%s' % (n, mode[0], 'p' if mode[1] else ''))
        lines.append((kind, caught))
        if kind == 'floor_le':
            grid = np.arange(0x32000000, 0x33000000, 7, dtype=np.uint32).view(F32)          # every scale around the floor
            grid = np.concatenate([grid, [M.FLOOR, np.nextafter(M.FLOOR, F32(0)), np.nextafter(M.FLOOR, F32(1)), np.nan]]).astype(F32)
            with np.errstate(all='ignore'):
                assert M.same_bits(np.where(grid <= M.FLOOR, M.FLOOR, grid), np.maximum(grid, M.FLOOR))
            assert caught == []
        elif kind == 'qmax_powf':
            assert caught == [] and all(M.params_mutant(kind, [0.], [1.], b, False)[2] == M.qmax_ref(b) for b in range(1, 33))
        else:
            assert caught, kind
    for kind in M.DOMAIN_MUTANTS:
        caught = []
        for mode in M.MODES:
            for n, a, b in M.table(mode):
                sc = M.params_ref([a], [b], *mode)[0]
                if bool(M.fast_domain_ref(a, b, sc[0])) != bool(M.fast_domain_mutant(kind, a, b, sc[0], *mode)):
                    caught.append('%s@%d%s' % (n, mode[0], 'p' if mode[1] else ''))
        lines.append((kind, caught))
        assert caught, kind
    with capsys.disabled():
        print()
        for kind, caught in lines:
            print('  %-34s %s' % (kind, ', '.join(caught) if caught else '- (equivalent: the same bits for every scale)'))
    by = dict(lines)
    assert {'tie_up@4'} <= set(by['round_half_away']) and 'nan@4' in by['floor_drops_nan']
    assert 'neg_zero_zp@4' not in by['rint_of_minus_q'] and any(n.startswith(('const_zero', 'floor', 'all_pos')) for n in by['rint_of_minus_q'])
    assert set(M.EQUIVALENT_MUTANTS) == {k for k, v in lines if not v} and any(n.endswith('@32') for n in by['qmax_int32'])
    assert all(n.endswith('p') for n in by['offset_mn_under_positive'] + by['delta_mx_minus_mn_under_positive'])
    assert any(n.startswith('scale_at_2p30') for n in by['domain_lt']) and any(n.startswith('abs_at_2p70') for n in by['domain_lt'])
