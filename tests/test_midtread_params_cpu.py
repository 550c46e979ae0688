"""tests/_midtread_params.py pinned to the reference and the oracle (no GPU): mt_ref reproduces the reference's own get_omega /
get_alpha_mult (tests/golden/midtread_params.npz), the oracle's mid_tread_core given statistics, and the mid-tread golden's
intermediates, bit for bit; every std vector the GPU test uses keeps every channel's real-valued omega more than 2e-5 (relative, at
least absolute) away from a half-integer and keeps its omega when the priors and their sum move by 4 ulps; and every case of the
GPU test really takes the branch it is named for."""
import math

import numpy as np
import pytest
import torch

import _midtread_params as M
from cnn_quantization_amd import _lib as L
from conftest import bits_equal
from oracle import quant_oracle as O

REAL = M.real_tables()


def _int_target(t):
    return int(t) if float(t) == int(t) else float(t)


def test_the_layout_constants_are_the_library_s():
    assert (M.MT_DELTA, M.MT_CMIN, M.MT_CMAX, M.MT_OMEGA, M.MT_ALPHA, M.MT_WSTART, M.NMT) == (
        L.MT_DELTA, L.MT_CMIN, L.MT_CMAX, L.MT_OMEGA, L.MT_ALPHA, L.MT_WSTART, L.NMT)
    assert (M.HIST_BINS, M.HIST_WINDOW) == (L.MT_HIST_BINS, L.MT_HIST_WINDOW)
    assert (M.STAT_MIN, M.STAT_MAX, M.STAT_MEAN, M.STAT_STD, M.STAT_B) == (L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD, L.STAT_B)


def test_mt_ref_reproduces_the_reference_fixture(golden):
    g = golden('midtread_params')
    names = [str(n) for n in g.np('names')]
    assert len(names) == len(M.GOLDEN_CELLS)
    for (C, target), key in zip(M.GOLDEN_CELLS, names):
        std = g.t(key + '_std')
        assert float(g.np(key + '_target')) == target and std.numel() == C
        assert bits_equal(std, M.guarded_prior(C, M.CELLS[(C, target)])), key            # the fixture's inputs are the GPU test's
        table = M.make_table(C, -torch.ones(C), torch.ones(C), torch.zeros(C), std, std * 0.8)
        for sym in (True, False):
            omega, alpha = M.mt_ref(table, _int_target(target), 1, sym, *REAL)[:2]
            assert bits_equal(omega, g.np(key + '_omega')), (key, sym)
            assert bits_equal(alpha, g.np('%s_alpha_sym%d' % (key, sym)).astype(np.float32)), (key, sym)


def _oracle_parts(table, target, clip, sym, tabs):
    """O.mid_tread_core on the table: std / mean / b handed over, min / max through a two-column tensor (the non-negative range
    reads max alone, iq.py:196)."""
    t = torch.stack([table[M.STAT_MIN] if sym else table[M.STAT_MAX], table[M.STAT_MAX]], dim=1)
    stats = dict(std=table[M.STAT_STD], mean=table[M.STAT_MEAN], b=table[M.STAT_B])
    with np.errstate(all='ignore'):
        return O.mid_tread_core(t, target, bool(clip), bool(sym), *tabs, return_parts=True, stats=stats)[2]


def _check_against_oracle(table, target, tabs, what):
    C = table.shape[1]
    for sym in (True, False):
        for clip in (1, 0):
            omega, alpha, delta, cmin, cmax, wstart = M.mt_ref(table, target, clip, sym, *tabs)
            p = _oracle_parts(table, target, clip, sym, tabs)
            key = (what, sym, clip)
            assert bits_equal(omega, p['omega']) and bits_equal(delta, p['Delta']), key
            if clip:
                assert bits_equal(alpha, p['alpha_mult']) and bits_equal(cmax, p['c_max']), key
                assert bits_equal(cmin, p['c_min'] * torch.ones(C)), key
                assert bool((wstart == wstart[0]).all()), key
                if np.isfinite(cmin).all():
                    assert wstart[0] == max(math.floor(float(cmin.min())), -65536), key
            else:
                # the oracle's weight path has no multiplier and no clamp
                assert p['alpha_mult'] is None and p['c_min'] is None and p['c_max'] is None
                assert bool((alpha == 0).all()) and bool((cmin == -math.inf).all()) and bool((cmax == math.inf).all())
                assert bool((wstart == -64).all())


def test_mt_ref_reproduces_the_oracle_on_every_guarded_cell():
    n = 0
    for C, target, seed in M.cells():
        table = M.cell_table(C, seed)
        om = M.mt_ref(table, _int_target(target), 0, True, *REAL)[0]
        for sym in (True, False):
            if float(om.max()) * (1 if sym else 2) > REAL[0][-1]:
                # beyond the table the oracle raises, as the reference does: that is where the library's choice begins
                with pytest.raises(IndexError):
                    _oracle_parts(table, _int_target(target), 1, sym, REAL)
        if float(om.max()) * 2 <= REAL[0][-1]:
            _check_against_oracle(table, _int_target(target), REAL, (C, target))
            n += 1
    assert n >= 18
    assert float(M.mt_ref(M.cell_table(65, M.CELLS[(65, 8)]), 8, 0, True, *REAL)[0].max()) > 955          # (65, 8) leaves the table


def test_mt_ref_reproduces_the_oracle_on_the_chosen_omegas_and_edge_rows():
    for tabs, omegas, _ in M.HAND.values():
        inside = [k for k in omegas if 2 * k <= tabs[0][-1]]
        table, target = M.interp_table(inside, 3)
        _check_against_oracle(table, target, tabs, 'hand')
    for sym in (True, False):
        inside = [k for k in M.omegas_covering(sym, REAL[0]) if 2 * k <= REAL[0][-1]]
        table, target = M.interp_table(inside, 4)
        _check_against_oracle(table, target, REAL, 'real')
    # the edge rows whose omegas the reference has a multiplier for: all of them (omega <= 9)
    table, target = M.edge_table()
    _check_against_oracle(table, target, REAL, 'edge')
    _check_against_oracle(M.tie_table(), M.TIE_TARGET, REAL, 'tie')


def test_mt_ref_reproduces_the_midtread_golden(golden):
    g = golden('midtread')
    for key in [str(n) for n in g.np('names')]:
        si = int(key[-1])
        x = g.t('x%d' % si)
        C = x.shape[1]
        t = x.transpose(0, 1).contiguous().view(C, -1)
        mu = t.mean(-1)
        table = M.make_table(C, t.min(-1)[0], t.max(-1)[0], mu, t.std(-1), (t - mu[:, None]).abs().mean(-1))
        target, sym = _int_target(float(g.np(key + '_target'))), not bool(g.np(key + '_half'))
        omega, alpha = M.mt_ref(table, target, 1, sym, *REAL)[:2]
        assert bits_equal(omega, g.np(key + '_omega')), key
        assert bits_equal(alpha, g.np(key + '_alpha_mult').astype(np.float32)), key


# ------------------------------------------------------------------------------------------------ the guard
def _guard(std, target, what):
    margin = M.omega_margin(std, target)
    assert margin > M.MARGIN, (what, margin)
    if M.quotients(std, target) is None:
        return
    base = M.omega_moved(std, target, 0, 0)
    for kp in (-4, 4):
        for ks in (-4, 4):
            assert M.same_bits(M.omega_moved(std, target, kp, ks), base), (what, kp, ks)
    # the fp32 oracle agrees with the fp64 quotient it is guarded by
    assert np.array_equal(base.astype(np.float64), np.rint(M.quotients(std, target))), what


def test_every_gpu_input_is_guarded():
    tables = M.gpu_tables()
    assert len(tables) > 70
    for what, (table, target) in tables.items():
        _guard(table[M.STAT_STD], target, what)
    # the guard sees what it is there for: a quotient next to a half-integer, and the tie itself
    assert M.omega_margin(torch.tensor([1., 1.]), M.TIE_TARGET) == 0.
    assert M.omega_margin(torch.tensor([1., 1.00001]), M.TIE_TARGET) < M.MARGIN


def test_the_tie_rounds_to_even():
    table = M.tie_table()
    assert np.float32(2 * 2 ** M.TIE_TARGET) == np.float32(5.)
    for sym in (True, False):
        omega = M.mt_ref(table, M.TIE_TARGET, 1, sym, *REAL)[0]
        assert omega.tolist() == [2., 2.]
    assert O.roundf_np(np.float32([2.5]))[0] == 3.                    # what roundf would give


# ------------------------------------------------------------------------------------------------ the cases are what they claim
def test_the_hand_tables_give_the_values_worked_out_by_hand():
    for tabs, _, values in M.HAND.values():
        for k, want in values.items():
            got = M.alpha_ref(torch.tensor([float(k)]), True, *tabs)[0]
            assert got == want, (k, got, want)
            if k % 2 == 0:
                assert M.alpha_ref(torch.tensor([k / 2.]), False, *tabs)[0] == want, k      # the doubled form lands on the same omega
    # table C at the knot in front of its cliff: the segment behind the knot would not give 1
    otab, atab = M.HAND_C
    assert atab[2] - ((atab[2] - atab[1]) / (otab[2] - otab[1])) * (otab[2] - 4.) != 1.
    # the issue's own list on table A, the non-integer omega through the oracle alone
    got = O.alpha_mult_from_tables(torch.tensor([0., 1., 3., 16., .5]), True, *M.HAND_A)
    assert got.tolist() == [0., .5, 1.625, 4., .25]


def test_every_knot_case_is_in_the_case_lists():
    for tabs, omegas in ((M.HAND_A, M.HAND_A_OMEGAS), (M.HAND_B, M.HAND_B_OMEGAS), (REAL, M.omegas_covering(True, REAL[0]))):
        for sym in (True, False):
            kinds = {M.segment_of(k, sym, tabs[0])[1] for k in omegas}
            want = {'at_knot', 'between', 'beyond_last'} | ({'below_first'} if tabs[0][0] > 0 else set())
            assert kinds >= want, (sym, kinds)
            # omega 0: on the first knot (distance 0) or below it (the wrapped segment with a distance)
            assert M.segment_of(0, sym, tabs[0]) == (0, 'below_first' if tabs[0][0] > 0 else 'at_knot')
    # table B: first, middle and last segment each hold a tested omega strictly inside
    inside = {M.segment_of(k, True, M.HAND_B[0]) for k in M.HAND_B_OMEGAS}
    assert {(1, 'between'), (3, 'between'), (4, 'between')} <= inside


def test_the_real_table_has_every_reachable_segment_hit():
    """omega is an integer, so 51 of the 100 segments of the real table cannot be reached at all (40 lie inside (0, 0.955], 11
    more hold no integer); under the doubled form only the 45 indices with an even integer count.  Every reachable one is hit, and the table
    built from the list gives exactly these omegas."""
    otab = REAL[0]
    assert len(M.reachable_segments(True, otab)) == 50 and len(M.reachable_segments(False, otab)) == 45
    for sym in (True, False):
        omegas = M.omegas_covering(sym, otab)
        hit = {M.segment_of(k, sym, otab)[0] for k in omegas}
        assert hit >= set(M.reachable_segments(sym, otab)), sym
        assert len(otab) in hit                                                  # beyond the table
        table, target = M.interp_table(omegas, 4)
        assert M.mt_ref(table, target, 1, sym, *REAL)[0].tolist() == [float(k) for k in omegas]
    for tabs, omegas, _ in M.HAND.values():
        table, target = M.interp_table(omegas, 3)
        assert M.mt_ref(table, target, 1, True, *tabs)[0].tolist() == [float(k) for k in omegas]


def test_every_edge_row_takes_its_branch():
    table, target = M.edge_table()
    name = {n: i for i, n in enumerate(M.EDGE_NAMES)}
    want = [float(r[1]) for r in M.ORD_ROWS + M.EDGE_ROWS]
    sym1 = dict(zip(M.ROWS, M.mt_ref(table, target, 1, True, *REAL)))
    pos1 = dict(zip(M.ROWS, M.mt_ref(table, target, 1, False, *REAL)))
    sym0 = dict(zip(M.ROWS, M.mt_ref(table, target, 0, True, *REAL)))
    assert sym1['omega'].tolist() == want
    fmax = np.float32(M.F32_MAX)
    for z in ('std0', 'std_denormal'):
        c = name[z]
        assert sym1['omega'][c] == 0 and sym1['delta'][c] == fmax and sym0['delta'][c] == fmax
        assert sym1['cmin'][c] == sym1['cmax'][c] == np.float32(0.3) / fmax                  # both bounds mu / FLT_MAX
    c = name['b0']
    assert sym1['delta'][c] == 0 and sym1['cmin'][c] == math.inf
    c = name['b0_mean0']
    assert np.isnan(sym1['cmin'][c]) and np.isnan(sym1['cmax'][c]) and pos1['cmin'][c] == 0
    c = name['mean_neg']
    assert pos1['delta'][c] == pos1['alpha'][c] * np.float32(0.5) / 6 and pos1['cmax'][c] == 6     # mu0 == 0: no mean anywhere
    assert sym1['cmin'][c] + sym1['cmax'][c] < 0                                                   # the symmetric range keeps it
    c = name['far_mean']
    assert math.floor(sym1['cmin'][c]) < -65536
    c = name['huge']
    assert sym1['delta'][c] == math.inf and sym0['delta'][c] == math.inf and sym1['cmin'][c] == -1.5
    c = name['denormal']
    assert 0 < sym1['delta'][c] < np.finfo(np.float32).tiny and np.isfinite(sym1['cmin'][c])
    c = name['nan_mean']
    assert np.isnan(pos1['delta'][c]) and np.isnan(pos1['cmax'][c]) and pos1['cmin'][c] == 0       # torch.max keeps the NaN
    assert np.isnan(sym1['cmin'][c]) and not np.isnan(sym1['delta'][c])
    assert sym1['cmin'][name['ninf_mean']] == -math.inf and sym1['cmin'][name['inf_mean']] == math.inf
    assert np.isnan(sym1['delta'][name['nan_b']]) and sym1['delta'][name['inf_b']] == math.inf
    assert np.isnan(sym0['delta'][name['nan_min']]) and sym0['delta'][name['inf_max']] == math.inf
    assert sym0['delta'][name['max_eq_min']] == 0
    # the table's window start is the clamp (far_mean / ninf_mean / the NaN bounds all ask for less than -65536)
    assert sym1['wstart'][0] == -65536 and pos1['wstart'][0] == 0 and sym0['wstart'][0] == -64


def test_poisoned_and_constant_tables_are_what_they_claim():
    for nm, v in M.POISON_STD:
        table, target = M.poison_table(v)
        omega = M.mt_ref(table, target, 1, True, *REAL)[0]
        if nm in ('std_nan', 'std_neg'):
            assert np.isnan(omega).all(), nm                            # the sum is poisoned, as in the reference
        elif nm == 'std_inf':
            assert np.isnan(omega[1]) and bool((np.delete(omega, 1) == 0).all())
        else:
            assert omega[1] == 48 and bool((np.delete(omega, 1) == 0).all())
    for C in (1, 2, 65):
        rows = dict(zip(M.ROWS, M.mt_ref(M.constant_table(C), 4, 1, True, *REAL)))
        # psum == 0: every omega is 0 / 0 - the library's NaN rows where the reference raises
        assert np.isnan(rows['omega']).all() and np.isnan(rows['alpha']).all() and np.isnan(rows['cmax']).all()
        assert bool((rows['delta'] == np.float32(M.F32_MAX)).all()) and bool((rows['wstart'] == -65536).all())
        with pytest.raises(IndexError):
            _oracle_parts(M.constant_table(C), 4, 1, True, REAL)


def test_every_wstart_case_is_decided_by_its_slot():
    for C, slots in M.WSTART_SLOTS.items():
        for slot in slots:
            rows = dict(zip(M.ROWS, M.mt_ref(M.wstart_table(C, slot), 4, 1, True, *REAL)))
            cmin = rows['cmin']
            assert int(np.argmin(cmin)) == slot, (C, slot)
            others = np.delete(cmin, slot)
            assert math.floor(cmin[slot]) < math.floor(others.min()) and cmin[slot] > -65536, (C, slot)
            assert rows['wstart'][0] == math.floor(cmin[slot])
            assert M.mt_ref(M.wstart_table(C, slot), 4, 1, False, *REAL)[5][0] == 0         # the non-negative range: exactly 0
    plain = M.mt_ref(M.wstart_table(1025, 700, 'none'), 4, 1, True, *REAL)
    assert plain[5][0] > -65536
    for kind in ('clamp', 'nan', 'ninf'):
        rows = dict(zip(M.ROWS, M.mt_ref(M.wstart_table(1025, 700, kind), 4, 1, True, *REAL)))
        c = rows['cmin'][700]
        assert {'clamp': math.isfinite(c) and c < -65536, 'nan': np.isnan(c), 'ninf': c == -math.inf}[kind]
        assert not (np.delete(rows['cmin'], 700) < -65536).any() and not np.isnan(np.delete(rows['cmin'], 700)).any()
        assert rows['wstart'][0] == -65536
