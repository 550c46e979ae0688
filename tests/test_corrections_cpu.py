"""tests/_corrections.py checked without a GPU: the restatement of the two correction chains against the pinned oracle, and the
premises the device tests (test_corrections_table_gpu.py) rest on - that the dyadic inputs make every partial sum exact, that
the hand-built records and tables tell the right expression from the plausible wrong ones, and that the class shapes reach the
load shapes they are listed for (cnnq_plan_describe is host code)."""
import ctypes

import numpy as np
import pytest
import torch

import _corrections as K
from cnn_quantization_amd import _lib as L
from oracle import quant_oracle as O

F = np.float32


def describe(N, C, HW, aligned, fine):
    out = (ctypes.c_int32 * 12)()
    assert L.load().cnnq_plan_describe(N, C, HW, aligned, fine, out) == 0
    return dict(zip(K.PLAN_WORDS, list(out)))


def test_constants_are_the_library_s():
    assert (K.STAT_MEAN, K.STAT_STD, K.NSTAT) == (L.STAT_MEAN, L.STAT_STD, L.NSTAT)
    assert (K.QP_SCALE, K.QP_ZP, K.QP_QMAX, K.NQP) == (L.QP_SCALE, L.QP_ZP, L.QP_QMAX, L.NQP)


@pytest.mark.parametrize('case', K.CLASSES, ids=K.class_id)
def test_class_shapes_reach_their_load_shapes(case):
    (N, C, H, W), off, want = case
    got = describe(N, C, H * W, int(off == 0), 0)
    assert {k: got[k] for k in want} == want, got
    assert got['G'] == got['S'] * got['nb'] == L.load().cnnq_pc_groups(N, C, H * W, int(off == 0))
    fine = describe(N, C, H * W, int(off == 0), 1)
    assert (fine['vec'], fine['A'], fine['J'], fine['mode']) == (got['vec'], got['A'], got['J'], got['mode'])


def test_every_load_shape_and_fold_is_listed():
    """the five with_shape instances, crossed with mode 1 / 2 where the planner can produce both (the straddling shape and
    J = 2 exist in mode 2 alone: cpc <= 1024 there)"""
    seen = {(w['vec'], w['A'], w['J'], w['mode']) for _, _, w in K.CLASSES}
    assert seen == {(1, 1, 4, 1), (1, 1, 4, 2), (4, 4, 1, 2), (4, 1, 1, 1), (4, 1, 1, 2), (4, 1, 2, 2), (4, 1, 4, 1), (4, 1, 4, 2)}
    # uneven sample ranges: N / S is no integer
    assert any(s[0] % w['S'] for s, _, w in K.CLASSES if 'S' in w)


@pytest.mark.parametrize('case', K.CLASSES, ids=K.class_id)
def test_dyadic_inputs_make_every_sum_exact(case):
    shape = case[0]
    N, C, H, W = shape
    x, qp = K.dyadic(shape, seed=C + H)
    y2, _ = K.dyadic(shape, seed=C + H + 1000)
    q = K.qdq32(x, qp)
    x8, y8, q4 = x.astype(np.float64) * 8, y2.astype(np.float64) * 8, q.astype(np.float64) * 4
    for t, bound in ((x8, 64), (y8, 64), (q4, 4 * 512 - 1)):
        assert np.array_equal(t, np.rint(t)) and np.abs(t).max() <= bound
    bits = x.view(np.uint32).reshape(-1)
    assert bits[0] == 0 and bits[1] == 0x80000000                       # +0.0 and -0.0
    if C > 1:
        assert (x[:, C - 1] < 0).all()
    assert {float(v) for v in qp[K.QP_SCALE]} <= {0.25, 0.5, 1.} and {float(v) for v in qp[K.QP_QMAX]} <= {0., 3., 15., 255.}
    assert np.array_equal(qp[K.QP_ZP], np.rint(qp[K.QP_ZP])) and qp[K.QP_ZP].min() >= 0 and qp[K.QP_ZP].max() <= 8
    for relu_first in (0, 1):
        for second, s4 in ((y2, 8), (q, 4)):
            sums, mag = K.sums64(x, second, relu_first)
            xi = K.rows(np.maximum(x8, 0) if relu_first else x8).astype(np.int64)
            si = K.rows(second.astype(np.float64) * s4).astype(np.int64)
            assert np.array_equal(sums[0] * 8, xi.sum(1)) and np.array_equal(sums[1] * s4, si.sum(1))
            assert np.array_equal(sums[2], (xi > 0).sum(1))
            assert np.array_equal(mag[0] * 8, np.abs(xi).sum(1)) and np.array_equal(mag[1] * s4, np.abs(si).sum(1))
            if C > 1:
                assert sums[2][C - 1] == 0
    # the float32 quad sum of k_bcorr_sums' one-channel float4 path is exact on them
    for t in (x, K.relu32(x), y2, q):
        flat = t.reshape(-1)
        quad = flat[:flat.size // 4 * 4].reshape(-1, 4)
        s32 = (quad[:, 0] + quad[:, 1]) + (quad[:, 2] + quad[:, 3])
        assert s32.dtype == F and np.array_equal(s32.astype(np.float64), quad.astype(np.float64).sum(1))


@pytest.mark.parametrize('name', ['relu_first', 'full_range', 'one_channel_dead'])
def test_bias_restatement_vs_oracle(golden, name):
    """bias32 / apply32 on float64 sums against the pinned oracle (torch's float32 reductions) and the recorded reference output,
    with the tolerances of test_act_bias_correction_vs_oracle / _golden"""
    g = golden('bca')
    out, out_q, relu_first = g.t(name + '/out'), g.t(name + '/out_q'), bool(g.np(name + '/relu_first'))
    sums, _ = K.sums64(out, out_q, relu_first)
    got = K.apply32(out_q, K.bias32(sums))
    ref = O.act_bias_correction(out, out_q.clone(), relu_first).numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)
    assert np.array_equal(got == 0, ref == 0)
    np.testing.assert_allclose(got, g.np(name + '/corrected'), rtol=1e-5, atol=1e-5)
    if name == 'one_channel_dead':
        assert (sums[2] == 0).any()


@pytest.mark.parametrize('wshape', [(16, 8, 3, 3), (10, 64), (24, 3, 7, 7), (300, 5, 1, 1)])
@pytest.mark.parametrize('vc,bc', [(False, True), (True, False), (True, True)])
def test_weight_restatement_vs_oracle(wshape, vc, bc):
    """weight32 on float64 statistics against the pinned oracle, on the inputs and with the tolerances of
    test_weight_correction_vs_oracle"""
    gen = torch.Generator().manual_seed(21)
    w = torch.randn(wshape, generator=gen) * 0.05 + 0.01
    wq = O.weights_per_channel_qdq(w, 4)
    ref = O.weight_correction(w, wq, vcorr=vc, bcorr=bc).numpy()
    w2, q2 = w.view(wshape[0], -1).double(), wq.view(wshape[0], -1).double()
    got = K.weight32(q2.float(), w2.mean(1), w2.std(1), q2.mean(1), q2.std(1), vc, bc)
    np.testing.assert_allclose(got.reshape(wshape), ref, rtol=2e-5, atol=2e-7)


def test_named_records_tell_the_roundings_apart():
    a, b, n = K.NAMED['two_roundings']
    assert F(a) - F(b) != F(a - b) and F(a) - F(b) == 0 and F(a - b) == 1
    assert F(2. ** 24 + 1) == F(2. ** 24)
    sums = np.asarray([K.NAMED[k] for k in K.NAMES], dtype=np.float64).T.copy()
    bias = dict(zip(K.NAMES, K.bias32(sums)))
    wrong = dict(zip(K.NAMES, K.bias32_wrong(sums)))
    wrong_n = dict(zip(K.NAMES, K.bias32_wrong_count(sums)))
    assert bias['two_roundings'] == 0 and wrong['two_roundings'] == F(0.25)
    assert bias['count_2p24_plus_1'] == 1 and wrong_n['count_2p24_plus_1'] == F(0.99999994)
    assert bias['count_zero'] == F(5.) / F(1e-8) and np.isfinite(bias['count_zero'])
    assert bias['equal_sums'] == 0 and not np.signbit(bias['equal_sums'])
    assert np.isnan(bias['nan_record']) and bias['negative'] == F(-7.) / (F(7.) + F(1e-8)) == F(-1.)


@pytest.mark.parametrize('C', K.MERGE_C)
@pytest.mark.parametrize('G', K.MERGE_G)
def test_merge_records(G, C):
    part, named = K.merge_records(G, C, rot=G)
    assert part.shape == (G, 3, C) and part.dtype == np.float64
    live = ~np.isnan(part)
    assert np.array_equal(part[live], np.rint(part[live])) and np.abs(part[live]).max() < 2. ** 40
    total = part.sum(0)
    assert len(named) == (C if C <= 6 else 12)
    for ch, name in named.items():
        assert K.same(total[:, ch], np.asarray(K.NAMED[name], dtype=np.float64)), (ch, name)
    if C > 12:
        assert set(named.values()) == set(K.NAMES)
    # every record differs from the one a wrong stride would read in its place: next group, next row, next channel
    plain = [c for c in range(C) if c not in named]
    if plain:
        p = part[:, :, plain]
        assert (p[1:] != p[:-1]).all() and (p[:, 1:] != p[:, :-1]).all()
        assert all(part[g, r, c] == K.record_value(g, c, r) for g in (0, G - 1) for r in range(3) for c in (plain[0], plain[-1]))
    if len(plain) > 1 and plain[1] == plain[0] + 1:
        assert (part[:, :, plain[1]] != part[:, :, plain[0]]).all()
    # dropping any one record of a plain channel moves its sums
    assert (np.abs(part[:, :, plain]) >= 1).all() if plain else True


def test_hand_built_bias_and_y():
    b = K.hand_bias(8)
    assert (b > 0).any() and (b < 0).any() and np.isinf(b).any() and np.isnan(b).any()
    zeros = b.view(np.uint32)[b == 0]
    assert set(int(z) for z in zeros) == {0, 0x80000000}
    assert K.same(K.hand_bias(3, rot=6), K.BIAS_VALUES[[6, 7, 0]])
    y = K.hand_y((3, 8, 7, 7), seed=1)
    flat = y.reshape(-1)
    tiny = np.finfo(F).tiny
    assert (flat > 1).any() and (flat < -1).any() and np.isnan(flat).any()
    assert ((flat > 0) & (flat < tiny)).any() and ((flat < 0) & (flat > -tiny)).any()
    assert set(int(z) for z in flat.view(np.uint32)[flat == 0]) == {0, 0x80000000}
    # the -1000 channel carries every positive q across zero; the inf and NaN channels follow the reference expression
    out = K.apply32(y, b)
    pos = y[:, 4] > 0
    assert pos.any() and (out[:, 4][pos] < 0).all() and K.same(out[:, 4][~pos], y[:, 4][~pos])
    assert np.isinf(out[:, 5][y[:, 5] > 0]).all() and np.isnan(out[:, 5][~(y[:, 5] > 0)]).all()
    assert np.isnan(out[:, 6]).all()
    # a bias of -0.0 leaves every bit; +0.0 turns a -0.0 element into +0.0 (-0 + 0 * +0) and leaves the rest
    assert K.same(out[:, 3], y[:, 3]) and np.array_equal(out[:, 2], y[:, 2], equal_nan=True)
    assert not np.signbit(out[:, 2][y[:, 2] == 0]).any()
    y[0, 2, 0, 0] = F(-0.)
    assert not K.same(K.apply32(y, b)[:, 2], y[:, 2])


@pytest.mark.parametrize('C,HW', K.WEIGHT_CASES)
def test_weight_cases_have_something_at_stake(C, HW):
    wq, mean_w, std_w, mean_q, std_q = K.weight_case(C, HW, seed=C + HW)
    assert wq.shape == (C, HW) and wq.dtype == F
    args = (wq, mean_w, std_w, mean_q, std_q)
    assert K.same(K.weight32(*args, False, False), wq)
    kinds = [K.WEIGHT_KINDS[c % len(K.WEIGHT_KINDS)] for c in range(C)]
    for c, kind in enumerate(kinds[:12]):
        if kind == 'std_q_zero':
            assert std_q[c] == 0
        if kind == 'std_w_zero':
            assert std_w[c] == 0 and K.same(K.weight32(*args, True, False)[c], np.full(HW, mean_q[c], dtype=F))
        if kind == 'mean_q_is_element':
            assert (wq[c] == mean_q[c]).any()
    if C * HW < 27:
        return
    right, fma, assoc = (f(*args, True, True) for f in (K.weight32, K.weight32_fma, K.weight32_assoc))
    assert not K.same(right, fma) and not K.same(right, assoc)
    assert not K.same(K.weight32(*args, True, False), K.weight32_fma(*args, True, False))
    assert not K.same(K.weight32(*args, False, True), K.weight32_assoc(*args, False, True))
    # and by more than a sign of zero or a NaN: low bits of ordinary values in the channels with ordinary tables
    plain = [c for c, kind in enumerate(kinds) if kind == 'plain']
    for wrong in (fma, assoc) if len(plain) * HW >= 64 else ():
        d = (right[plain] != wrong[plain]) & np.isfinite(right[plain]) & np.isfinite(wrong[plain])
        assert d.any()
    t = K.stat_table(C, mean_w, std_w)
    assert np.isnan(np.delete(t, [K.STAT_MEAN, K.STAT_STD], axis=0)).all() and K.same(t[K.STAT_MEAN], mean_w)
